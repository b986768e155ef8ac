#!/usr/bin/env python3
"""Time HipState.reduced_density_matrix (include/qip_hipx.h) beside a norm_sqr pass and beside Pauli tomography, in one process.

For Complex<f64> and Complex<f32> at n qubits (default 30), on a dense random state (Gaussian amplitudes drawn on the device by
torch, normalised, wrapped by the handle, which launches on a torch stream so that torch's HIP events time its work):

  (a) norm_sqr: one read of the vector, the yardstick;
  (b) reduced_density_matrix for k = 1 .. 6 and three classes of index positions — the lowest k bits (bit 0 is the half of a packed
      Complex<f32> element), the top k bits, k scattered bits — with the ratio to (a) and the bytes of the vector over the time;
  (c) the route a tree without the call has: the 4^k Pauli strings on the k scattered qubits through expect_pauli (2^k X/Y masks:
      that many groups of passes), rho = 2^-k sum_P <P> P rebuilt on the host.

Every figure is the median of `--repeats` HIP-event timings (an event before and after the call on the handle's stream) after one
warm-up call; (c) takes `--tomo-repeats`.  The raw timings go to `--raw` as JSON lines.  Before any time is reported the matrix of
(c) is held to the matrix of (b) within 1e-10, the diagonal to measure_probs and the trace to norm_sqr.  Writes a markdown page and
prints it.

    python tools/bench_density.py [--n 30] [--repeats 7] [--tomo-repeats 3] [--out profiles/reduced_density_table.md] [--commit NAME]"""
import argparse
import itertools
import json
import os
import statistics
import sys

import numpy as np
import torch  # (before the library: the state is drawn by torch on the device the library then wraps)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rustqip_amd as q  # noqa: E402

RAW = []
PAULI = {"I": np.eye(2), "X": np.array([[0, 1], [1, 0]]), "Y": np.array([[0, -1j], [1j, 0]]), "Z": np.diag([1.0, -1.0])}


def position_classes(n, k):
    """(name, amplitude-index positions in outcome-bit order) of the three classes"""
    scattered = [b for b in (11, 0, n - 1, 6, (2 * n) // 3, n // 2 + 1) if b < n]
    return (("lowest bits", list(range(k))), ("top bits", list(range(n - k, n))), ("scattered", scattered[:k]))


def tomography(st, indices):
    """rho of the qubits `indices` from the 4^k expectation values: bit i of the row index is qubit indices[i]"""
    k = len(indices)
    strings = list(itertools.product("IXYZ", repeat=k))
    values = st.expect_pauli([{qb: p for qb, p in zip(indices, s) if p != "I"} for s in strings])
    rho = np.zeros((1 << k, 1 << k), dtype=np.complex128)
    for s, v in zip(strings, values):
        m = np.ones((1, 1))
        for p in s:  # qubit indices[0] is the least significant bit: the last Kronecker factor
            m = np.kron(PAULI[p], m)
        rho += v * m
    return rho / (1 << k)


class Timer:
    def __init__(self, st, stream):
        self.st, self.stream = st, stream

    def once(self, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(self.stream)
        fn()
        e1.record(self.stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def __call__(self, name, dtype, fn, repeats):
        fn()
        self.st.sync()
        times = [self.once(fn) for _ in range(repeats)]
        RAW.append({"dtype": np.dtype(dtype).name, "call": name, "ms": times})
        return statistics.median(times)


def measure(n, dtype, repeats, tomo_repeats, kmax):
    torch.manual_seed(30)
    amps = torch.randn(1 << n, dtype=torch.complex128 if dtype == np.complex128 else torch.complex64, device="cuda")
    amps /= torch.linalg.vector_norm(amps)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    nbytes = (1 << n) * (16 if dtype == np.complex128 else 8)
    rows, tomo = [], []
    with q.HipState(n, dtype, wrap_ptr=amps.data_ptr(), stream=stream.cuda_stream) as st:
        timed = Timer(st, stream)
        norm2 = st.norm_sqr()
        base = timed("(a) norm_sqr", dtype, st.norm_sqr, repeats)
        for k in range(1, kmax + 1):
            for name, pos in position_classes(n, k):
                indices = [n - 1 - b for b in pos]
                rho = st.reduced_density_matrix(indices)
                tol = 1e-12 if dtype == np.complex128 else 1e-6  # (measure_probs and norm_sqr form f32 products on an f32 state)
                assert np.max(np.abs(np.diag(rho).real - st.measure_probs(indices))) <= tol and abs(np.trace(rho).real - norm2) <= tol
                t = timed(f"(b) k = {k}, {name}", dtype, lambda: st.reduced_density_matrix(indices), repeats)
                rows.append((k, name, pos, t))
            name, pos = position_classes(n, k)[2]
            indices = [n - 1 - b for b in pos]
            worst = float(np.max(np.abs(tomography(st, indices) - st.reduced_density_matrix(indices))))
            assert worst <= 1e-10, (k, worst)
            t = timed(f"(c) tomography, k = {k}", dtype, lambda: tomography(st, indices), tomo_repeats)
            tomo.append((k, 4 ** k, q.expect_pauli_passes(n, [{qb: p for qb, p in zip(indices, s) if p != "I"} for s in itertools.product("IXYZ", repeat=k)]), t, worst))
    del amps
    torch.cuda.empty_cache()
    return base, nbytes, rows, tomo


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=30)
    ap.add_argument("--kmax", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--tomo-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reduced_density_table.md"))
    ap.add_argument("--raw", default=None, help="JSON lines of every timing (default: the page's name with .jsonl)")
    ap.add_argument("--commit", default="(not named)", help="the commit of the tree that ran, for the page")
    args = ap.parse_args()
    if not torch.cuda.is_available() or q.device_count() < 1:
        raise SystemExit("bench_density needs a HIP device")
    torch.cuda.init()
    lines = [f"# reduced_density_matrix beside a norm_sqr pass and Pauli tomography, n = {args.n}", "",
             f"`tools/bench_density.py --n {args.n} --repeats {args.repeats} --tomo-repeats {args.tomo_repeats}` on the tree of {args.commit}: "
             f"HIP events around each call on the handle's stream, medians of {args.repeats} ({args.tomo_repeats} for tomography) after a "
             "warm-up call, one process, a dense Gaussian state drawn on the device; the tomography matrix equalled the call's within "
             "1e-10 before anything was timed.", ""]
    for dtype in (np.complex128, np.complex64):
        base, nbytes, rows, tomo = measure(args.n, dtype, args.repeats, args.tomo_repeats, args.kmax)
        lines += [f"## {np.dtype(dtype).name}", "", f"norm_sqr: {base:.3f} ms ({nbytes / base * 1e-9:.2f} TB/s).", "",
                  "| k | positions | ms | / norm_sqr | TB/s | tomography ms (strings, passes) | tomography / call |", "|---:|---|---:|---:|---:|---:|---:|"]
        tomo_of = {k: (count, passes, t) for k, count, passes, t, _ in tomo}
        for k, name, pos, t in rows:
            count, passes, tt = tomo_of[k]
            extra = f"{tt:.1f} ({count}, {passes}) | {tt / t:.0f}x" if name == "scattered" else " | "
            lines.append(f"| {k} | {name} {pos} | {t:.3f} | {t / base:.2f} | {nbytes / t * 1e-9:.2f} | {extra} |")
        lines.append("")
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
