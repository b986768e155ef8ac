#!/usr/bin/env python
"""apply_op / apply_op_overwrite for Complex<f64> / Complex<f32> on device slices (qip_hip_apply_op_device, the call of all of the
reference's benches: qip/benches/state_bench.rs:141-155) at n = 28 (4 GiB in, 4 GiB out for Complex<f64>), and the launch-bound
sizes n = 12 / 20 call by call and as 64 calls inside one hipGraph.  Algorithmic bytes per row: sizeof(P) x (input read + output
write, + output read when accumulating).  HIP events on the stream the kernel is launched on.  The check column compares with
the literal kernel (option force_generic) at n = 28 and with the CPU oracle at n <= 20, bit for bit.

  python tools/bench_complex_slices.py [--no-graph]   (--no-graph: a library whose call synchronises cannot be captured)

Ops whose payload lives in the library's device-resident cache (a dense op on >= 4 qubits, every SparseMatrix):

  python tools/bench_complex_slices.py --payloads [n] [rounds] [--parent-lib libqip_hip.so] [--tuning-lib libqip_hip.so]

One process per library and round, the libraries alternating; per shape the median and the range over the rounds of the wall
time per call (a call and a stream synchronisation) and of the HIP-event time.  --parent-lib: the parent commit's build (its
calls only launch, as this tree's do: they are recorded into the hipGraph too).  --tuning-lib: a -DQIP_HIP_TUNING build of this tree, run with option slice_read_once = 0 — every
cached payload through the literal pointer launch (k_gather_cplx), the yardstick of the read-once kernels.  The launch-bound
shapes (a dense 8-qubit op at n = 8, a sparse 16-qubit op at n = 16) are timed call by call, as host time per call without a
synchronisation beside that of an op whose table travels in the kernel arguments (the difference is the hash and the compare of
the payload), and as 64 calls in one hipGraph."""
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rustqip_amd as q  # noqa: E402
from oracle import qip_oracle as O  # noqa: E402  (the check of the small sizes only)
from rustqip_amd import _ffi  # noqa: E402
from rustqip_amd.ops import MatrixOp  # noqa: E402


def gpu_time(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def bits(t):
    return torch.view_as_real(t).view(torch.int64 if t.dtype == torch.complex128 else torch.int32)


def main():
    graphs = "--no-graph" not in sys.argv
    s2 = float(np.sqrt(0.5))
    h = [s2, s2, s2, -s2]
    rng = np.random.default_rng(3)
    cv = lambda c: rng.standard_normal(c) + 1j * rng.standard_normal(c)  # noqa: E731
    print("| n | P | op | accumulate | GPU us / call | algorithmic GB/s | of 8 TB/s | check |\n|---|---|---|---|---|---|---|---|")
    n = 28
    big = [("H on qubit 0", MatrixOp.new_matrix([0], h)), ("H on qubit 14", MatrixOp.new_matrix([14], h)),
           ("H on qubit n-1", MatrixOp.new_matrix([n - 1], h)),
           ("CNOT(5 -> 20)", MatrixOp.new_control([5], [20], MatrixOp.new_matrix([20], [0, 1, 1, 0]))),
           ("dense on qubits 3, n-2", MatrixOp.new_matrix([3, n - 2], cv(16))),
           ("dense on qubits 2, 9, 17", MatrixOp.new_matrix([2, 9, 17], cv(64))),
           ("controlled (6) dense on qubits 12, 21", MatrixOp.new_control([6], [12, 21], MatrixOp.new_matrix([12, 21], cv(16)))),
           ("Swap(1, n-4)", MatrixOp.new_swap([1], [n - 4]))]
    shapes = [(n, dt, name, op, acc) for dt in (np.complex128, np.complex64) for name, op in big for acc in (True, False)]
    shapes += [(m, dt, "H on qubit 0, ones in (state_bench.rs:141-155)", MatrixOp.new_matrix([0], h), True) for m in (12, 20)
               for dt in (np.complex128, np.complex64)]
    bufs = {}
    for n, dt, name, op, acc in shapes:
        N = 1 << n
        tdt = torch.complex128 if dt == np.complex128 else torch.complex64
        if (n, dt) not in bufs:  # (one input, one output and one comparison buffer per size and type)
            bufs.clear()
            torch.manual_seed(5)
            d_in = torch.ones(N, dtype=tdt, device="cuda") if n <= 20 else torch.randn(N, dtype=tdt, device="cuda")
            bufs[(n, dt)] = (d_in, torch.zeros(N, dtype=tdt, device="cuda"), torch.zeros(N, dtype=tdt, device="cuda") if n > 20 else None)
        d_in, d_out, d_ref = bufs[(n, dt)]
        cop = op.to_c(_ffi.QIP_C64 if dt == np.complex128 else _ffi.QIP_C32)  # (built once, as the reference's benches do)
        d_out.zero_()
        sec = gpu_time(lambda: q.apply_op_device(n, cop, d_in, d_out, accumulate=acc), 200 if n <= 20 else 10)
        by = np.dtype(dt).itemsize * N * (3 if acc else 2)
        graph_us = None
        if n <= 20 and graphs:  # 64 calls recorded into ONE hipGraph (the call is a plain kernel launch on the given stream)
            side = torch.cuda.Stream()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                q.apply_op_device(n, cop, d_in, d_out, accumulate=acc, stream=side.cuda_stream)
                side.synchronize()
                with torch.cuda.graph(g, stream=side):
                    for _ in range(64):
                        q.apply_op_device(n, cop, d_in, d_out, accumulate=acc, stream=side.cuda_stream)
            graph_us = gpu_time(g.replay, 50) / 64 * 1e6
        # check: one more call from a zeroed output
        d_out.zero_()
        q.apply_op_device(n, cop, d_in, d_out, accumulate=acc)
        torch.cuda.synchronize()
        if n <= 20:
            want = np.zeros(N, dtype=dt)
            O.apply_op(n, op, np.ones(N, dtype=dt), want, accumulate=acc)
            ok = np.array_equal(d_out.cpu().numpy().view(np.uint8), want.view(np.uint8))
            against = "the oracle"
        else:
            d_ref.zero_()
            q.set_global_option("force_generic", 1)
            try:
                q.apply_op_device(n, cop, d_in, d_ref, accumulate=acc)
                torch.cuda.synchronize()
            finally:
                q.set_global_option("force_generic", 0)
            ok = bool(torch.equal(bits(d_out), bits(d_ref)))
            against = "the literal kernel"
        note = "" if n > 20 else ("; not captured" if graph_us is None else "; %.2f us / call inside a 64-call hipGraph" % graph_us)
        print(f"| {n} | {np.dtype(dt).name} | {name} | {int(acc)} | {sec*1e6:.1f} | {by/sec/1e9:.0f} | {by/sec/8e12*100:.1f} % | "
              f"{'bit-equal to ' + against if ok else 'DIFFERS from ' + against}{note} |", flush=True)


def payload_shapes(n, rng):
    cv = lambda c: rng.standard_normal(c) + 1j * rng.standard_normal(c)  # noqa: E731
    pos = lambda *ps: [n - 1 - p for p in ps]  # noqa: E731  (index positions -> qubits)
    shapes = [("dense 4", MatrixOp.new_matrix(pos(3, 9, 17, n - 2), cv(256))),
              ("dense 5", MatrixOp.new_matrix(pos(3, 9, 14, 17, n - 2), cv(1024))),
              ("dense 6", MatrixOp.new_matrix(pos(3, 7, 9, 14, 17, n - 2), cv(4096))),
              ("controlled (pos 6) dense 4", MatrixOp.new_control(pos(6), pos(3, 9, 17, n - 2), MatrixOp.new_matrix(pos(3, 9, 17, n - 2), cv(256))))]
    for k in (6, 8, 16):
        idx = pos(*range(2, 2 + k)) if k == 16 else pos(*([3, 7, 9, 14, 17, n - 2] + [11, 20])[:k])
        for e in (1, 2, 4):
            cols = rng.integers(0, 1 << k, size=(1 << k, e))
            cols[:, 0] = rng.permutation(1 << k)
            vals = cv((1 << k) * e).reshape(1 << k, e)
            shapes.append((f"sparse {k}, {e} per row", MatrixOp.new_sparse(idx, [list(zip(c.tolist(), v.tolist())) for c, v in zip(cols, vals)])))
    return shapes


def wall_and_event(fn, reps):
    """(seconds per call of `fn` + a synchronisation, HIP-event seconds per call of `reps` calls back to back)"""
    fn()
    torch.cuda.synchronize()
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    return statistics.median(walls), gpu_time(fn, reps)


def payload_worker(n):
    """every shape once in this process's library; one JSON document"""
    read_once = os.environ.get("QIP_BENCH_READ_ONCE")
    if read_once is not None:
        q.set_global_option("slice_read_once", int(read_once))
    capturable = os.environ.get("QIP_BENCH_CAPTURE", "1") == "1"
    rng = np.random.default_rng(7)
    out = {}
    shapes = payload_shapes(n, rng)
    for dt in (np.complex128, np.complex64):
        N = 1 << n
        tdt = torch.complex128 if dt == np.complex128 else torch.complex64
        torch.manual_seed(5)
        d_in, d_out = torch.randn(N, dtype=tdt, device="cuda"), torch.zeros(N, dtype=tdt, device="cuda")
        for name, op in shapes:
            cop = op.to_c(_ffi.QIP_C64 if dt == np.complex128 else _ffi.QIP_C32)
            for acc in (True, False):
                d_out.zero_()
                wall, ev = wall_and_event(lambda: q.apply_op_device(n, cop, d_in, d_out, accumulate=acc), 3)
                out[f"{n}|{np.dtype(dt).name}|{name}|{int(acc)}"] = {"wall_us": wall * 1e6, "event_us": ev * 1e6}
        del d_in, d_out
        torch.cuda.empty_cache()
    # launch-bound: the reference's own bench shapes
    small = [(8, "dense 8", MatrixOp.new_matrix(list(range(8)), rng.standard_normal(1 << 16) + 1j * rng.standard_normal(1 << 16))),
             (16, "sparse 16, 1 per row", MatrixOp.new_sparse(list(range(16)), [[(int(c), 1.0)] for c in rng.permutation(1 << 16)])),
             (16, "H on qubit 0 (kernel arguments)", MatrixOp.new_matrix([0], [np.sqrt(0.5)] * 3 + [-np.sqrt(0.5)]))]
    for m, name, op in small:
        d_in, d_out = torch.ones(1 << m, dtype=torch.complex128, device="cuda"), torch.zeros(1 << m, dtype=torch.complex128, device="cuda")
        cop = op.to_c(_ffi.QIP_C64)
        call = lambda stream=0: q.apply_op_device(m, cop, d_in, d_out, stream=stream)  # noqa: E731
        wall, ev = wall_and_event(call, 50)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(200):
            call()
        host = (time.perf_counter() - t0) / 200  # (no synchronisation: what the host spends per call, unless the call itself waits)
        torch.cuda.synchronize()
        rec = {"wall_us": wall * 1e6, "event_us": ev * 1e6, "host_us": host * 1e6}
        if capturable:
            side = torch.cuda.Stream()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                call(side.cuda_stream)
                side.synchronize()
                with torch.cuda.graph(g, stream=side):
                    for _ in range(64):
                        call(side.cuda_stream)
            rec["graph_us"] = gpu_time(g.replay, 50) / 64 * 1e6
        out[f"{m}|complex128|{name}|1"] = rec
    print("PAYLOADS " + json.dumps(out), flush=True)


def payload_main(args):
    libs = {"new": None}
    for flag, key in (("--parent-lib", "parent"), ("--tuning-lib", "literal")):
        if flag in args:
            libs[key] = os.path.abspath(args[args.index(flag) + 1])
            del args[args.index(flag): args.index(flag) + 2]
    n = int(args[0]) if args else 28
    rounds = int(args[1]) if len(args) > 1 else 5
    runs = {k: [] for k in libs}
    for r in range(rounds):
        for lib in sorted(libs, reverse=True):  # ("parent", "new", "literal")
            env = dict(os.environ)
            if libs[lib]:
                env["QIP_HIP_LIB"] = libs[lib]
            if lib == "literal":
                env["QIP_BENCH_READ_ONCE"] = "0"
            p = subprocess.run([sys.executable, __file__, "--payload-worker", str(n)], env=env, capture_output=True, text=True, timeout=280)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("PAYLOADS ")]
            if p.returncode != 0 or not line:
                print("FAILED", lib, r, p.returncode, p.stdout[-2000:], p.stderr[-2000:], flush=True)
                return 1  # nothing more on the GPU after a failure
            runs[lib].append(json.loads(line[0][len("PAYLOADS "):]))
            print(f"round {r} {lib} done", file=sys.stderr, flush=True)
    stat = lambda vs: "%.1f (%.1f - %.1f)" % (statistics.median(vs), min(vs), max(vs))  # noqa: E731
    order = [k for k in ("parent", "new", "literal") if k in libs]
    print(f"medians of {rounds} rounds (min - max), us per call\n")
    print("| n | P | op | accumulate | " + " | ".join(f"{k}: wall | {k}: HIP events" for k in order) + " | new: algorithmic GB/s (events) |")
    print("|---|---|---|---|" + "---|---|" * len(order) + "---|")
    for key in runs["new"][0]:
        m, dt, name, acc = key.split("|")
        cells = []
        for k in order:
            cells += [stat([run[key]["wall_us"] for run in runs[k]]), stat([run[key]["event_us"] for run in runs[k]])]
        by = np.dtype(dt).itemsize * (1 << int(m)) * (3 if acc == "1" else 2)
        ev = statistics.median([run[key]["event_us"] for run in runs["new"]])
        print(f"| {m} | {dt} | {name} | {acc} | " + " | ".join(cells) + (f" | {by / ev / 1e3:.0f} |" if int(m) > 20 else " | — |"))
    print("\nlaunch-bound shapes: host us per call without a synchronisation; us per call inside a 64-call hipGraph\n")
    print("| n | op | " + " | ".join(f"{k}: host" for k in order) + " | " + " | ".join(f"{k}: in a graph" for k in order) + " |")
    print("|---|---|" + "---|" * (2 * len(order)))
    for key in runs["new"][0]:
        if "host_us" not in runs["new"][0][key]:
            continue
        m, dt, name, acc = key.split("|")
        cells = [stat([run[key]["host_us"] for run in runs[k]]) for k in order]
        cells += [stat([run[key]["graph_us"] for run in runs[k]]) for k in order]
        print(f"| {m} | {name} | " + " | ".join(cells) + " |")
    return 0


if __name__ == "__main__":
    if "--payload-worker" in sys.argv:
        payload_worker(int(sys.argv[sys.argv.index("--payload-worker") + 1]))
    elif "--payloads" in sys.argv:
        sys.exit(payload_main([a for a in sys.argv[1:] if a != "--payloads"]))
    else:
        main()
