#!/usr/bin/env python3
"""Time linear_combination, inner_products and the Krylov solvers of HipState (include/qip_hipx.h) beside the calls that were
there before, in one process.

For Complex<f64> and Complex<f32> at each `--n` (default 28 and 30), on dense random states (Gaussian amplitudes drawn on the
device by torch, normalised, wrapped by the handles); a count that needs more states than the device's free memory holds is
left out and the page says so:

  (a) one combination pass of 1, 2, 3, 4, 8 and 16 sources into a further state, with and without the norm: the time, and the
      share of 8 TB/s that (count + 1) vectors in that time are;
  (b) inner_products of 1, 4 and 16 bras against as many single `inner` calls (pauli_matrix_elements with the empty term);
  (c) the Lanczos update w <- w - a v - b v', |w|^2 as ONE combination of three sources with its norm (4 vectors) against the
      same update through the calls of the parent commit: two accumulating apply_pauli_sum calls with the empty term and norm_sqr
      (7 vectors);
  (d) one reorthogonalised Lanczos step with 7 basis vectors behind it on a transverse-field Ising chain, call by call;
  (e) at `--evolve-n` (default 24): krylov_evolve over t = 0.5 with the fewest substeps (1, 2, 4, ...) that bring the state within
      `--accuracy` (default 1e-3, 2-norm, relative) of a reference, against first-order Trotter `evolve` with the fewest steps
      (doubling, at most 2048) that do.  The reference is krylov_evolve in Complex<f64> with 64 substeps.

Every figure is the median of `--repeats` host-clock timings around a call that is complete when it returns (or ends in a
synchronise), after one warm-up call; the raw timings go to `--raw` as JSON lines.  Before any time is reported the combination
is held to the parent's route through apply_pauli_sum and the inner products to `inner`.  Writes a markdown page (default
profiles/krylov.md) and prints it.

    python tools/bench_krylov.py [--n 28 30] [--repeats 5] [--out profiles/krylov.md] [--commit NAME]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # (before the library: the states are drawn by torch on the device the library then wraps)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rustqip_amd as q  # noqa: E402

COUNTS = (1, 2, 3, 4, 8, 16)
INNER_COUNTS = (1, 4, 16)
PEAK = 8e12  # bytes per second, the HBM peak the shares are of
RAW = []


def timed(name, n, dtype, fn, repeats):
    """median of `repeats` host-clock timings of fn(), in ms, after one warm-up call"""
    fn()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    RAW.append({"n": n, "dtype": np.dtype(dtype).name, "call": name, "ms": times})
    return statistics.median(times)


def ising(n):
    terms = [{i: "Z", i + 1: "Z"} for i in range(n - 1)] + [{i: "X"} for i in range(n)]
    return terms, np.array([-1.0] * (n - 1) + [-1.5] * n)


class States:
    """`count` random normalised device states behind library handles (torch owns the memory and the streams)"""

    def __init__(self, n, dtype, count, seed=31):
        torch.manual_seed(seed)
        tdtype = torch.complex128 if dtype == np.complex128 else torch.complex64
        self.amps, self.streams, self.handles = [], [], []
        for _ in range(count):
            x = torch.randn(1 << n, dtype=tdtype, device="cuda")
            x /= torch.linalg.vector_norm(x)
            self.amps.append(x)
            self.streams.append(torch.cuda.Stream())
        torch.cuda.synchronize()
        for x, s in zip(self.amps, self.streams):
            self.handles.append(q.HipState(n, dtype, wrap_ptr=x.data_ptr(), stream=s.cuda_stream))

    def close(self):
        for h in self.handles:
            h.close()
        self.handles, self.amps = [], []
        torch.cuda.empty_cache()


def passes(n, dtype, repeats):
    """(rows of the page, notes) for one size and precision"""
    bytes_per = (1 << n) * np.dtype(dtype).itemsize
    free, _ = torch.cuda.mem_get_info()
    room = int(free * 0.9 // bytes_per)
    most = max(c for c in COUNTS if c + 1 <= room) if room >= 2 else 0
    notes = []
    if most < COUNTS[-1]:
        notes.append(f"{room} states of {bytes_per / 2 ** 30:.0f} GiB fit the free memory: counts above {most} were left out.")
    if most == 0:
        return [], notes
    u = 2.0 ** -53 if dtype == np.complex128 else 2.0 ** -24
    st = States(n, dtype, most + 1)
    dst, src = st.handles[0], st.handles[1:]
    rows = []
    try:
        # ---- the checks: the combination against the parent's route, the inner products against `inner` -----------------------
        if most >= 3:
            a, b = -0.37, -0.81
            dst.linear_combination([src[0], src[1], src[2]], [1.0, a, b])
            src[0].apply_pauli_sum(src[1], [{}], [a], accumulate=True)
            src[0].apply_pauli_sum(src[2], [{}], [b], accumulate=True)
            worst, _ = dst.max_abs_diff(src[0])
            assert worst <= 8 * u * 4 * 2.0 ** (-n / 2), f"the combination is {worst} from the parent's route"  # (amplitudes of size 2^(-n/2))
        got, want = dst.inner_products(src[:2]), [src[0].inner(dst), src[1].inner(dst)]
        assert np.max(np.abs(got - np.array(want))) <= 2e-12, (got, want)
        # ---- (a) ---------------------------------------------------------------------------------------------------------
        rng = np.random.default_rng(7)
        for count in [c for c in COUNTS if c <= most]:
            cs = rng.standard_normal(count) + 1j * rng.standard_normal(count)
            for norm in (False, True):
                ms = timed(f"(a) combination of {count}, norm={norm}", n, dtype, lambda: dst.linear_combination(src[:count], cs, want_norm=norm), repeats)
                share = (count + 1) * bytes_per / (ms * 1e-3) / PEAK
                rows.append((f"(a) linear_combination, {count} source(s){', with the norm' if norm else ''}", ms, f"{100 * share:.0f} % of 8 TB/s over {count + 1} vectors"))
        # ---- (b) ---------------------------------------------------------------------------------------------------------
        for count in [c for c in INNER_COUNTS if c <= most]:
            ms = timed(f"(b) inner_products of {count}", n, dtype, lambda: dst.inner_products(src[:count]), repeats)
            single = timed(f"(b) {count} inner calls", n, dtype, lambda: [s.inner(dst) for s in src[:count]], repeats)
            rows.append((f"(b) inner_products, {count} bra(s)", ms, f"{count} `inner` call(s): {single:.3f} ms, {single / ms:.2f}x; "
                         f"{100 * (count + 1) * bytes_per / (ms * 1e-3) / PEAK:.0f} % of 8 TB/s over {count + 1} vectors"))
        # ---- (c) ---------------------------------------------------------------------------------------------------------
        if most >= 3:
            w, v, vp = src[0], src[1], src[2]
            fused = timed("(c) fused update", n, dtype, lambda: w.linear_combination([w, v, vp], [1.0, -0.3, -0.2], want_norm=True), repeats)

            def parent():
                w.apply_pauli_sum(v, [{}], [-0.3], accumulate=True)
                w.apply_pauli_sum(vp, [{}], [-0.2], accumulate=True)
                return w.norm_sqr()

            old = timed("(c) parent update", n, dtype, parent, repeats)
            rows.append(("(c) Lanczos update, one combination of three with the norm", fused, "4 vectors"))
            rows.append(("(c) the same through two accumulating empty-term apply_pauli_sum calls and norm_sqr", old, f"7 vectors; {old / fused:.2f}x the fused update"))
        # ---- (d) ---------------------------------------------------------------------------------------------------------
        if most >= 8:
            terms, cs = ising(n)
            basis, w = src[:7], src[7]
            v = basis[-1]
            parts = [
                ("apply_pauli_sum, the chain's %d terms in %d passes" % (len(terms), q.pauli_sum_passes(n, terms)), lambda: w.apply_pauli_sum(v, terms, cs)),
                ("inner_products, 1 bra (alpha)", lambda: w.inner_products([v])),
                ("linear_combination of 3 with the norm (the update)", lambda: w.linear_combination([w, v, basis[-2]], [1.0, -0.3, -0.2], want_norm=True)),
                ("inner_products, 7 bras (reorthogonalisation)", lambda: w.inner_products(basis)),
                ("linear_combination of 8 with the norm (reorthogonalisation)", lambda: w.linear_combination([w] + basis, [1.0] + [1e-9] * 7, want_norm=True)),
                ("scale (normalisation)", lambda: w.scale(1.0001)),
            ]
            total = 0.0
            for name, fn in parts:
                ms = timed(f"(d) {name}", n, dtype, fn, repeats)
                total += ms
                rows.append((f"(d) Lanczos step: {name}", ms, ""))
            rows.append(("(d) Lanczos step: the sum of its calls", total, ""))
    finally:
        st.close()
    return rows, notes


def evolve_rows(n, repeats, accuracy, t=0.5, m=15):
    """(e): rows for both precisions"""
    terms, cs = ising(n)
    rows = []
    ref_states = States(n, np.complex128, m + 2, seed=5)
    psi, basis = ref_states.handles[0], ref_states.handles[1:]
    start = ref_states.amps[0].clone()
    estimate = psi.krylov_evolve(terms, cs, t, basis, substeps=64)
    reference = ref_states.amps[0].clone()
    ref_states.close()
    for dtype in (np.complex128, np.complex64):
        tdtype = torch.complex128 if dtype == np.complex128 else torch.complex64
        st = States(n, dtype, m + 2, seed=6)
        psi, basis, amps = st.handles[0], st.handles[1:], st.amps[0]
        try:
            def reset():
                psi.sync()
                amps.copy_(start.to(tdtype))
                torch.cuda.synchronize()

            def error():
                psi.sync()
                return float(torch.linalg.vector_norm(amps.to(torch.complex128) - reference))

            substeps = 1
            while True:
                reset()
                est = psi.krylov_evolve(terms, cs, t, basis, substeps=substeps)
                err = error()
                if err <= accuracy or substeps >= 64:
                    break
                substeps *= 2

            def run_krylov():
                reset()
                psi.krylov_evolve(terms, cs, t, basis, substeps=substeps)

            ms = timed(f"(e) krylov_evolve, {substeps} substeps", n, dtype, run_krylov, max(1, min(repeats, 3)))
            rows.append((f"(e) {np.dtype(dtype).name}: krylov_evolve, m = {m}, {substeps} substep(s) (with the reset of the state)", ms,
                         f"error {err:.2e}, its own estimate {est:.2e}; {substeps * m} applications of H"))
            steps = 16
            while True:
                reset()
                psi.evolve(terms, cs, t / steps, steps)
                err = error()
                if err <= accuracy or steps >= 2048:
                    break
                steps *= 2

            def run_trotter():
                reset()
                psi.evolve(terms, cs, t / steps, steps)
                psi.sync()

            trot = timed(f"(e) evolve, {steps} steps", n, dtype, run_trotter, max(1, min(repeats, 3)))
            reached = "" if err <= accuracy else " (NOT reached at the cap of 2048 steps)"
            rows.append((f"(e) {np.dtype(dtype).name}: first-order Trotter evolve, {steps} steps{reached} (with the reset of the state)", trot,
                         f"error {err:.2e}; {trot / ms:.1f}x krylov_evolve's time"))
        finally:
            st.close()
    return rows, estimate


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, nargs="+", default=[28, 30])
    ap.add_argument("--evolve-n", type=int, default=24)
    ap.add_argument("--accuracy", type=float, default=1e-3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "krylov.md"))
    ap.add_argument("--raw", default=None, help="JSON lines of every timing (default: the page's name with .jsonl)")
    ap.add_argument("--commit", default="(not named)", help="the commit of the tree that ran, for the page")
    args = ap.parse_args()
    if not torch.cuda.is_available() or q.device_count() < 1:
        raise SystemExit("bench_krylov needs a HIP device")
    torch.cuda.init()
    lines = ["# linear_combination, inner_products and the Krylov solvers", "",
             f"`tools/bench_krylov.py --n {' '.join(str(n) for n in args.n)} --repeats {args.repeats}` on the tree of {args.commit}: a host clock "
             f"around each call (every one is complete when it returns), medians of {args.repeats} after a warm-up call, one process, dense "
             "Gaussian states drawn on the device; the combination was held to the parent's route through apply_pauli_sum and the inner "
             "products to `inner` before anything was reported.", ""]
    for n in args.n:
        for dtype in (np.complex128, np.complex64):
            rows, notes = passes(n, dtype, args.repeats)
            lines += [f"## n = {n}, {np.dtype(dtype).name}", ""] + notes + ([""] if notes else [])
            if rows:
                lines += ["| call | ms | |", "|---|---:|---|"] + [f"| {name} | {ms:.3f} | {what} |" for name, ms, what in rows] + [""]
            print("\n".join(lines[-(len(rows) + 6):]), flush=True)
    if args.evolve_n > 0:
        rows, estimate = evolve_rows(args.evolve_n, args.repeats, args.accuracy)
        lines += [f"## Evolution over t = 0.5 at n = {args.evolve_n}, transverse-field Ising chain, accuracy {args.accuracy:g}", "",
                  f"Reference: krylov_evolve in complex128 with 64 substeps (its own estimate of its error: {estimate:.1e}).", "",
                  "| call | ms | |", "|---|---:|---|"] + [f"| {name} | {ms:.3f} | {what} |" for name, ms, what in rows] + [""]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    with open(args.raw or os.path.splitext(args.out)[0] + ".jsonl", "w") as f:
        for rec in RAW:
            f.write(json.dumps(rec) + "\n")
    print(text)


if __name__ == "__main__":
    main()
