#!/usr/bin/env python
"""Diagonal 2-qubit Matrix ops inside tile sweeps: two layers of (a ring of n ZZ phases, n Rx gates) on three paths — apply_ops on
the default path, what a HipBuilder caller pays (a fresh handle, tile = 1 + relabelling, tile_auto), and tile = 2 with compiled
segments, tile_fma and tile_merge — with ZZ written as a 4x4 diagonal Matrix op ("diag") and as CNOT . Rz . CNOT ("cnot").

  python tools/bench_diag_items.py [n] [rounds] [--parent-lib /path/to/libqip_hip.so]

One process per run; with --parent-lib the two libraries alternate.  Round 0 primes the code-object cache and is dropped; per
library and spelling the medians (and the range) of the other rounds are printed as one JSON document, ms per run of the circuit
and launches."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBS = {"new": os.path.join(ROOT, "rustqip_amd", "lib", "libqip_hip.so")}


def worker(n, spelling):
    sys.path.insert(0, ROOT)
    import numpy as np

    import rustqip_amd as q
    from rustqip_amd import circuits
    from rustqip_amd.builder import HipBuilder

    ops = circuits.qaoa_ring(n, 2, spelling)
    out = {"spelling": spelling, "gates": len(ops)}

    def timed(st, reps):
        ms = []
        for _ in range(reps):
            st.sync()
            t0 = time.perf_counter()
            st.apply_ops(ops)
            st.sync()
            ms.append(1e3 * (time.perf_counter() - t0))
        return ms

    def launches(st):
        st.set_option("profile", 1)
        st.profile_reset()
        st.apply_ops(ops)
        st.sync()
        k = sum(v["launches"] for key, v in st.profile().items() if key != "tile_sweep_parts")
        st.set_option("profile", 0)
        return k

    with q.HipState(n, np.complex128) as st:
        st.init_basis(0)
        st.apply_ops(circuits.h_layer(n))
        # a. the default path
        st.set_option("tile_auto", 0)
        out["default_launches"] = launches(st)
        out["default_ms"] = timed(st, 3)
        # c. tile = 2, compiled segments, tile_fma + tile_merge
        for k, v in (("tile", 2), ("tile_jit", 1), ("tile_fma", 1), ("tile_merge", 1)):
            st.set_option(k, v)
        out["tile2_launches"] = launches(st)
        out["tile2_ms"] = timed(st, 3)
        out["norm"] = st.norm_sqr()
    # b. what a HipBuilder / calculate_state caller pays: a fresh handle, tile = 1 + relabelling, one batch (tile_auto: compiled wide
    # sweeps when the disk cache holds them — a "second process" — else the interpreter)
    b = HipBuilder()
    with q.HipState(n, np.complex128) as st:
        st.set_option("tile", b.tile)
        st.set_option("tile_relabel", b.tile_relabel)
        st.init_basis(0)
        st.set_option("tile_auto", 0)
        st.apply_ops(circuits.h_layer(n))
        st.set_option("tile_auto", 1)
        st.sync()
        t0 = time.perf_counter()
        st.apply_ops(ops)
        st.sync()
        out["builder_ms"] = [1e3 * (time.perf_counter() - t0)]
        st.set_option("tile_auto", 0)
        out["builder_launches"] = launches(st)
    print("RESULT " + json.dumps(out), flush=True)


def main():
    args = [a for a in sys.argv[1:]]
    if "--parent-lib" in args:
        LIBS["parent"] = os.path.abspath(args[args.index("--parent-lib") + 1])
        del args[args.index("--parent-lib"): args.index("--parent-lib") + 2]
    n = int(args[0]) if args else 30
    rounds = int(args[1]) if len(args) > 1 else 6
    res = {}
    for r in range(rounds):
        for spelling in ("diag", "cnot"):
            for lib in sorted(LIBS, reverse=True):  # ("parent", "new")
                env = dict(os.environ, QIP_HIP_LIB=LIBS[lib])
                p = subprocess.run([sys.executable, __file__, "--worker", str(n), spelling], env=env, capture_output=True, text=True, timeout=170)
                if p.returncode != 0:
                    print("FAILED", lib, spelling, p.returncode, p.stdout[-2000:], p.stderr[-2000:], flush=True)
                    return 1  # nothing more on the GPU after a failure
                line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
                d = json.loads(line[7:])
                print(r, lib, line, flush=True)
                res.setdefault((lib, spelling), []).append(d)
    summary = {}
    for (lib, spelling), runs in res.items():
        runs = runs[1:]  # round 0 primes the caches of the run-time compiler
        s = {}
        for key in ("default_ms", "tile2_ms", "builder_ms"):
            per_run = [min(d[key]) for d in runs]
            s[key] = {"median": round(statistics.median(per_run), 2), "min": round(min(per_run), 2), "max": round(max(per_run), 2), "runs": len(per_run)}
        for key in ("default_launches", "tile2_launches", "builder_launches", "gates"):
            s[key] = runs[-1][key]
        summary[f"{lib}/{spelling}"] = s
    print(json.dumps(summary, indent=1))
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--worker":
        worker(int(sys.argv[2]), sys.argv[3])
    else:
        sys.exit(main())
