#!/usr/bin/env python3
"""Time HipState.apply_diagonal / expect_diagonal (include/qip_hipx.h) beside the general Pauli calls on the same terms, in one
process.

For Complex<f64> and Complex<f32> at n qubits (default 30), on a dense random state (Gaussian amplitudes drawn on the device by
torch, normalised, wrapped by the handle, which launches on a torch stream so that torch's HIP events time its work), and six
sets of Z-string terms — 1, 4 and 16 random Z strings (one rotation pass each: where the new call starts to pay), the n-term
ZZ ring, the n (n - 1) / 2 terms of the complete graph, and all two- and three-body terms:

  (a) the floors: a one-term rotation pass (one read and one write of the vector) and norm_sqr (one read);
  (b) one apply_diagonal call against apply_pauli_rotations on the same terms with the angles gamma * c_t;
  (c) one expect_diagonal call against expect_pauli on the same terms.

The term arrays are marshalled once, outside the timed region: a timing brackets the C call alone (its own host work — term
checks, the sort by low mask, the table's upload — included).  Every figure is the median of `--repeats` HIP-event timings (an
event before and after the call on the handle's stream) after one warm-up call; calls of more than a second are repeated three
times.  The raw timings go to `--raw` as JSON lines.  Before any time is reported the new calls are held to the general ones on
the complete graph: on a 13-qubit state, and on the state and at the size that are timed, on the device (check_at_size: a second
handle, max_abs_diff, the bars of tests/diagonal_ref.py restated).  Writes a markdown page (default profiles/diagonal.md)
and prints it.

    python tools/bench_diagonal.py [--n 30] [--repeats 7] [--out profiles/diagonal.md] [--commit NAME] [--only-diagonal]

--only-diagonal times the two new calls and the floors alone: the comparison of builds with another tile width
(-DQIP_DIAG_TILE_BITS=11 / 13 for csrc/qip_pauli.hip, loaded through QIP_HIP_LIB)."""
import argparse
import ctypes as C
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
from rustqip_amd import _ffi  # noqa: E402
from rustqip_amd.state import _check, _pauli_terms  # noqa: E402

RAW = []
_DBLP = C.POINTER(C.c_double)


def term_sets(n):
    rng = np.random.default_rng(1416)
    strings = [{n - 1 - b: "Z" for b in range(n) if (z >> b) & 1} for z in (int(v) for v in rng.integers(1, 1 << n, 16))]
    ring = [{i: "Z", (i + 1) % n: "Z"} for i in range(n)]
    pairs = [{a: "Z", b: "Z"} for a, b in itertools.combinations(range(n), 2)]
    triples = [{a: "Z", b: "Z", c: "Z"} for a, b, c in itertools.combinations(range(n), 3)]
    return (("1 random Z string", strings[:1]), ("4 random Z strings", strings[:4]), ("16 random Z strings", strings),
            ("ZZ ring", ring), ("complete graph", pairs), ("all 2- and 3-body terms", pairs + triples))


class Calls:
    """the four calls on one term set with the arrays marshalled once"""

    def __init__(self, st, terms, coeffs, gamma):
        self.st, self.count = st, len(terms)
        self.start, self.qubits, self.paulis, _ = _pauli_terms(st.n, terms)
        self.coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
        self.angles = np.ascontiguousarray(gamma * self.coeffs)
        self.gamma = float(gamma)
        self.moments = (C.c_double * 2)()
        self.values = np.empty(self.count, dtype=np.float64)

    def apply_diagonal(self):
        _check(_ffi.lib.qipx_state_apply_diagonal(self.st._h, self.start, self.qubits, self.paulis, self.coeffs.ctypes.data_as(_DBLP),
                                                  self.count, self.gamma))

    def rotations(self):
        _check(_ffi.lib.qipx_state_apply_pauli_rotations(self.st._h, self.start, self.qubits, self.paulis,
                                                         self.angles.ctypes.data_as(_DBLP), self.count))

    def expect_diagonal(self):
        _check(_ffi.lib.qipx_state_expect_diagonal(self.st._h, self.start, self.qubits, self.paulis, self.coeffs.ctypes.data_as(_DBLP),
                                                   self.count, self.moments))

    def expect_pauli(self):
        _check(_ffi.lib.qipx_state_expect_pauli(self.st._h, self.start, self.qubits, self.paulis, self.count,
                                                self.values.ctypes.data_as(_DBLP)))


class Timer:
    def __init__(self, st, stream, repeats):
        self.st, self.stream, self.repeats = st, stream, repeats

    def once(self, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(self.stream)
        fn()
        e1.record(self.stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def __call__(self, name, dtype, fn):
        fn()
        self.st.sync()
        times = [self.once(fn)]
        times += [self.once(fn) for _ in range((3 if times[0] > 1000.0 else self.repeats) - 1)]
        RAW.append({"dtype": np.dtype(dtype).name, "call": name, "ms": times})
        return statistics.median(times)


def check_small():
    """n = 13, the complete graph: the new calls against the general ones (unit vector: absolute bars)"""
    n = 13
    rng = np.random.default_rng(7)
    x = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    x /= np.linalg.norm(x)
    _, terms = term_sets(n)[4]
    coeffs = rng.standard_normal(len(terms))
    for dtype, bar in ((np.complex128, 1e-12), (np.complex64, 1e-5)):
        with q.HipState(n, dtype) as a, q.HipState(n, dtype) as b:
            a.upload(x)
            b.upload(x)
            m1, _ = a.expect_diagonal(terms, coeffs)
            assert abs(m1 - b.expectation(terms, coeffs)) <= 1e-10, (m1, b.expectation(terms, coeffs))
            a.apply_diagonal(terms, coeffs, 0.3)
            b.apply_pauli_rotations(terms, 0.3 * coeffs)
            worst, _ = a.max_abs_diff(b)
            assert worst <= bar * len(terms), worst


TILE_BITS = 12


def check_at_size(st, n, dtype, amps):
    """The complete graph on the timed state itself: apply_diagonal against apply_pauli_rotations on a copy (max_abs_diff on the
    device), expect_diagonal against expect_pauli.  With u the state's unit roundoff, T terms, L = 12, A = sum |gamma c_t|,
    A1 = sum |c_t| (the bars of tests/diagonal_ref.py, and the rotation call's element bar 24 u |psi_j| per term for x = 0):
        |difference_j| <= [12 u + (T + L + 8) 2^-53 A + 24 u T] max |psi|
        |m1 - c . expect_pauli| <= [(T + L + c(n) + 6) 2^-53 + 1e-12] A1 |psi|^2,   c(n) = 16 max(1, 2^(n-24)) + 10 + min(4096, 2^(n-12))"""
    u = 2.0 ** -53 if dtype == np.complex128 else 2.0 ** -24
    terms = term_sets(n)[4][1]
    coeffs = np.random.default_rng(77).standard_normal(len(terms))
    gamma, count = 0.3, len(terms)
    a1 = float(np.sum(np.abs(coeffs)))
    biggest = float(amps.abs().max())
    torch.cuda.synchronize()
    with q.HipState(n, dtype) as twin:
        twin.copy_from(st)
        norm = st.norm_sqr()
        m1, _ = st.expect_diagonal(terms, coeffs)
        want = st.expectation(terms, coeffs)
        chain = 16 * max(1, 1 << max(n - 24, 0)) + 10 + min(4096, 1 << max(n - TILE_BITS, 0))
        bar1 = ((count + TILE_BITS + chain + 6) * 2.0 ** -53 + 1e-12) * a1 * norm
        assert abs(m1 - want) <= bar1, (m1, want, bar1)
        st.apply_diagonal(terms, coeffs, gamma)
        twin.apply_pauli_rotations(terms, gamma * coeffs)
        worst, _ = st.max_abs_diff(twin)
        bar = (12 * u + (count + TILE_BITS + 8) * 2.0 ** -53 * abs(gamma) * a1 + 24 * u * count) * biggest
        assert worst <= bar, (worst, bar)
    return worst / bar, abs(m1 - want) / bar1


def measure(n, dtype, repeats, only_diagonal):
    rng = np.random.default_rng(3031)
    torch.manual_seed(31)
    amps = torch.randn(1 << n, dtype=torch.complex128 if dtype == np.complex128 else torch.complex64, device="cuda")
    amps /= torch.linalg.vector_norm(amps)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    rows = []
    with q.HipState(n, dtype, wrap_ptr=amps.data_ptr(), stream=stream.cuda_stream) as st:
        held = check_at_size(st, n, dtype, amps)
        timed = Timer(st, stream, repeats)
        one = Calls(st, [{0: "Z", n // 2: "Z"}], [1.0], 0.37)
        floor_rw = timed("(a) one-term rotation pass", dtype, one.rotations)
        floor_r = timed("(a) norm_sqr", dtype, st.norm_sqr)
        for name, terms in term_sets(n):
            calls = Calls(st, terms, rng.standard_normal(len(terms)), 0.3)
            row = {"set": name, "terms": len(terms)}
            row["apply_diagonal"] = timed(f"(b) apply_diagonal, {name}", dtype, calls.apply_diagonal)
            row["expect_diagonal"] = timed(f"(c) expect_diagonal, {name}", dtype, calls.expect_diagonal)
            if not only_diagonal:
                row["rotation_passes"] = q.pauli_rotation_passes(n, terms)
                row["rotations"] = timed(f"(b) apply_pauli_rotations, {name}", dtype, calls.rotations)
                row["expect_passes"] = q.expect_pauli_passes(n, terms)
                row["expect_pauli"] = timed(f"(c) expect_pauli, {name}", dtype, calls.expect_pauli)
            rows.append(row)
        assert abs(float(torch.linalg.vector_norm(amps)) - 1.0) <= 1e-4
    del amps
    torch.cuda.empty_cache()
    return floor_rw, floor_r, rows, held


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diagonal.md"))
    ap.add_argument("--raw", default=None, help="JSON lines of every timing (default: the page's name with .jsonl)")
    ap.add_argument("--commit", default="(not named)", help="the commit of the tree that ran, for the page")
    ap.add_argument("--only-diagonal", action="store_true", help="the two new calls and the floors alone")
    args = ap.parse_args()
    if not torch.cuda.is_available() or q.device_count() < 1:
        raise SystemExit("bench_diagonal needs a HIP device")
    torch.cuda.init()
    check_small()
    lines = [f"# apply_diagonal and expect_diagonal beside the general Pauli calls, n = {args.n}", "",
             f"`tools/bench_diagonal.py --n {args.n} --repeats {args.repeats}` on the tree of {args.commit}: HIP events around each C call "
             f"on the handle's stream (term arrays marshalled beforehand), medians of {args.repeats} after a warm-up call (3 for calls over a "
             "second), one process, a dense Gaussian state drawn on the device; on a 13-qubit state and on the timed state itself the new "
             "calls agreed with the general ones before anything was timed.", ""]
    for dtype in (np.complex128, np.complex64):
        floor_rw, floor_r, rows, held = measure(args.n, dtype, args.repeats, args.only_diagonal)
        lines += [f"## {np.dtype(dtype).name}", "",
                  f"Floors: a one-term rotation pass (read + write) {floor_rw:.3f} ms, norm_sqr (read) {floor_r:.3f} ms.  Held at n = {args.n} on "
                  f"the complete graph before timing: apply_diagonal against the rotations at {held[0]:.3f} of the bar, the first moment "
                  f"against expect_pauli at {held[1]:.3f} of its bar.", ""]
        if args.only_diagonal:
            lines += ["| terms | T | apply_diagonal ms | / floor | expect_diagonal ms | / norm_sqr |", "|---|---:|---:|---:|---:|---:|"]
            for r in rows:
                lines.append(f"| {r['set']} | {r['terms']} | {r['apply_diagonal']:.3f} | {r['apply_diagonal'] / floor_rw:.2f} | "
                             f"{r['expect_diagonal']:.3f} | {r['expect_diagonal'] / floor_r:.2f} |")
        else:
            lines += ["| terms | T | apply_diagonal ms | / floor | apply_pauli_rotations ms (passes) | speed-up | expect_diagonal ms | / norm_sqr | "
                      "expect_pauli ms (passes) | speed-up |", "|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|"]
            for r in rows:
                lines.append(f"| {r['set']} | {r['terms']} | {r['apply_diagonal']:.3f} | {r['apply_diagonal'] / floor_rw:.2f} | "
                             f"{r['rotations']:.3f} ({r['rotation_passes']}) | {r['rotations'] / r['apply_diagonal']:.2f}x | "
                             f"{r['expect_diagonal']:.3f} | {r['expect_diagonal'] / floor_r:.2f} | "
                             f"{r['expect_pauli']:.3f} ({r['expect_passes']}) | {r['expect_pauli'] / r['expect_diagonal']:.2f}x |")
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
