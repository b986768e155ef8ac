#!/usr/bin/env python3
"""Time HipState.apply_pauli_rotations (include/qip_hipx.h) beside one in-place single-qubit gate pass, in one process.

For Complex<f64> and Complex<f32> at n qubits (default 30), on a dense random state (Gaussian amplitudes drawn on the device by
torch, normalised, wrapped by the handle, which launches on a torch stream so that torch's HIP events time its work):

  (a) H on one qubit through apply_op: one read and one write of the vector, the yardstick;
  (b) one term per class of x mask: x = 0, bit 0 alone, bit 0 clear and low, the top bit, all bits — and its ratio to (a);
  (c) 1, 4, 16 and 32 terms that share one x mask, one pass each (option "rotate_group" raised to 32), for x = 0 and for a pair
      mask: what the kernel capacities cost — the default of "rotate_group" is the largest capacity whose pass stays within 1.5x
      of the single-term pass in every row;
  (d) a QAOA ring cost layer, n ZZ terms, as one call, against circuits.qaoa_ring's cost part ("diag" spelling) through
      apply_ops;
  (e) one Jordan-Wigner double excitation on qubits (3, 11, 19, 27) — 8 strings of one x mask with Z chains between — as one
      call, against the same strings lowered to basis changes, CNOT ladders and an Rz through apply_ops, first call and warm.

Every figure is the median of `--repeats` HIP-event timings (an event before and after the call on the handle's stream) after
one warm-up call; the raw timings go to `--raw` as JSON lines.  Before any time is reported a batch is held to its single-term
calls (exactly), and on a 12-qubit state the lowered circuits of (d) and (e) to the rotations.  Writes a markdown page (default
profiles/pauli_rotation.md) and prints it.

    python tools/bench_rotate.py [--n 30] [--repeats 7] [--out profiles/pauli_rotation.md] [--commit NAME]"""
import argparse
import cmath
import json
import math
import os
import statistics
import sys

import numpy as np
import torch  # (before the library: the state is drawn by torch on the device the library then wraps)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rustqip_amd as q  # noqa: E402
from rustqip_amd import circuits  # noqa: E402

CAPACITIES = (1, 4, 16, 32)
RAW = []


def term_of_masks(n, x, z):
    """X on x & ~z, Z on z & ~x, Y on x & z (masks over amplitude-index bits; qubit q is bit n - 1 - q)"""
    term = {}
    for b in range(n):
        bx, bz = (x >> b) & 1, (z >> b) & 1
        if bx or bz:
            term[n - 1 - b] = "Y" if bx and bz else ("X" if bx else "Z")
    return term


def lowered(term, theta):
    """exp(-i theta P) as basis changes (Y -> Z: S^dagger then H; X -> Z: H), a CNOT ladder onto the last qubit, Rz, and back"""
    qs = sorted(term)
    s2 = math.sqrt(0.5)
    h, sdg, s = [s2, s2, s2, -s2], [1, 0, 0, -1j], [1, 0, 0, 1j]
    pre, post = [], []
    for qb in qs:
        if term[qb] == "X":
            pre.append(q.make_matrix_op([qb], h))
            post.append(q.make_matrix_op([qb], h))
        elif term[qb] == "Y":
            pre += [q.make_matrix_op([qb], sdg), q.make_matrix_op([qb], h)]
            post += [q.make_matrix_op([qb], h), q.make_matrix_op([qb], s)]
    ladder = [q.make_control_op([a], q.make_matrix_op([b], circuits.X)) for a, b in zip(qs[:-1], qs[1:])]
    rz = q.make_matrix_op([qs[-1]], [cmath.rect(1, -theta), 0, 0, cmath.rect(1, theta)])
    return pre + ladder + [rz] + ladder[::-1] + post


def double_excitation(p, qq, r, s, theta):
    """the 8 strings of a Jordan-Wigner double excitation on qubits p < qq < r < s (Z chains on p+1 .. qq-1 and r+1 .. s-1) and
    their angles: one x mask"""
    chain = {k: "Z" for k in list(range(p + 1, qq)) + list(range(r + 1, s))}
    terms, angles = [], []
    for pattern, sign in (("XXXY", 1), ("XXYX", 1), ("XYXX", -1), ("YXXX", -1), ("YYYX", 1), ("YYXY", 1), ("YXYY", -1), ("XYYY", -1)):
        t = dict(chain)
        t.update(zip((p, qq, r, s), pattern))
        terms.append(t)
        angles.append(sign * theta / 8)
    return terms, angles


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

    def __call__(self, name, dtype, fn, warm=True):
        if warm:
            fn()
            self.st.sync()
        times = [self.once(fn) for _ in range(self.repeats)]
        RAW.append({"dtype": np.dtype(dtype).name, "call": name, "ms": times})
        return statistics.median(times)


def check_lowering():
    """at n = 12 (the double excitation on qubits 1, 4, 7, 10): the lowered circuits equal the rotations"""
    n = 12
    x = np.random.default_rng(5).standard_normal(1 << n) + 1j * np.random.default_rng(6).standard_normal(1 << n)
    x /= np.linalg.norm(x)
    terms, angles = double_excitation(1, 4, 7, 10, 0.9)
    with q.HipState(n) as a, q.HipState(n) as b:
        a.upload(x)
        b.upload(x)
        a.apply_pauli_rotations(terms, angles)
        b.apply_ops([op for t, th in zip(terms, angles) for op in lowered(t, th)])
        worst, _ = a.max_abs_diff(b)
        assert worst <= 1e-12, worst
        ring = [{i: "Z", (i + 1) % n: "Z"} for i in range(n)]
        a.apply_pauli_rotations(ring, [0.3] * n)
        b.apply_ops(circuits.qaoa_ring(n, 1)[:n])
        worst, _ = a.max_abs_diff(b)
        assert worst <= 1e-12, worst


def measure(n, dtype, repeats):
    rng = np.random.default_rng(3030)
    torch.manual_seed(30)
    amps = torch.randn(1 << n, dtype=torch.complex128 if dtype == np.complex128 else torch.complex64, device="cuda")
    amps /= torch.linalg.vector_norm(amps)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    full, top = (1 << n) - 1, 1 << (n - 1)
    zs = [int(v) for v in rng.integers(1, 1 << n, 64)]
    pair_x = top | 0x10412  # a pair mask with bit 0 clear: Complex<f32> moves 16-byte elements
    rows, ratios = [], {}
    with q.HipState(n, dtype, wrap_ptr=amps.data_ptr(), stream=stream.cuda_stream) as st:
        timed = Timer(st, stream, repeats)
        # the check: a batch leaves the bits of its single-term calls (the state stays a unit vector throughout)
        some = [term_of_masks(n, x, z) for x, z in ((0, zs[0]), (0, 0), (1, zs[1]), (1, zs[2]), (pair_x, zs[3]), (pair_x, zs[4]), (full, zs[5]))]
        thetas = [0.3, -0.8, 1.1, 2.0, -2.9, 0.6, 1.7]
        before = amps.clone()
        torch.cuda.synchronize()  # (torch's copies run on its own stream, the handle's work on `stream`)
        st.apply_pauli_rotations(some, thetas)
        st.sync()
        batch = amps.clone()
        amps.copy_(before)
        torch.cuda.synchronize()
        for t, th in zip(some, thetas):
            st.apply_pauli_rotations([t], [th])
        st.sync()
        differ = int(torch.count_nonzero(torch.view_as_real(batch) != torch.view_as_real(amps)))
        assert differ == 0, f"a batch differs from its single-term calls in {differ} components"
        assert abs(float(torch.linalg.vector_norm(amps)) - 1.0) <= 1e-4
        del before, batch
        torch.cuda.empty_cache()
        hgate = q.make_matrix_op([n // 2], circuits.H)
        base = timed("(a) H through apply_op", dtype, lambda: st.apply_op(hgate))
        rows.append(("(a) H on one qubit, apply_op", 1, 1, base))
        for name, x, z in (("(b) one term, x = 0", 0, zs[5]), ("(b) one term, x = bit 0 alone", 1, zs[6]), ("(b) one term, x = 0x12 (bit 0 clear, low)", 0x12, zs[7]),
                           ("(b) one term, x = the top bit", top, zs[8]), ("(b) one term, x = all bits", full, zs[9])):
            terms = [term_of_masks(n, x, z)]
            t = timed(name, dtype, lambda: st.apply_pauli_rotations(terms, [0.37]))
            ratios[name] = t / base
            rows.append((name, 1, 1, t))
        st.set_option("rotate_group", 32)
        worst = {c: 0.0 for c in CAPACITIES}
        for name, x in (("x = 0", 0), (f"x = {pair_x:#x}", pair_x)):
            one = None
            for count in CAPACITIES:
                terms = [term_of_masks(n, x, z) for z in zs[10:10 + count]]
                angles = list(rng.uniform(-3, 3, count))
                assert q.pauli_rotation_passes(n, terms, 32) == 1
                t = timed(f"(c) {count} terms, {name}", dtype, lambda: st.apply_pauli_rotations(terms, angles))
                one = t if one is None else one
                worst[count] = max(worst[count], t / one)
                rows.append((f"(c) {count} term(s), {name}, one pass", count, 1, t))
        default = max(c for c in CAPACITIES if worst[c] <= 1.5)
        st.set_option("rotate_group", default)
        # (d) a QAOA ring cost layer
        ring = [{i: "Z", (i + 1) % n: "Z"} for i in range(n)]
        gammas = [0.3] * n
        rows.append((f"(d) QAOA ring cost layer, one call, group {default}", n, q.pauli_rotation_passes(n, ring, default),
                     timed("(d) ring, rotations", dtype, lambda: st.apply_pauli_rotations(ring, gammas))))
        st.set_option("rotate_group", 32)
        rows.append(("(d) QAOA ring cost layer, one call, group 32", n, q.pauli_rotation_passes(n, ring, 32),
                     timed("(d) ring, rotations, group 32", dtype, lambda: st.apply_pauli_rotations(ring, gammas))))
        st.set_option("rotate_group", default)
        ring_ops = circuits.qaoa_ring(n, 1)[:n]
        rows.append((f"(d) the same through apply_ops: {len(ring_ops)} diagonal 4x4 ops, warm", len(ring_ops), None,
                     timed("(d) ring, apply_ops", dtype, lambda: st.apply_ops(ring_ops))))
        # (e) a Jordan-Wigner double excitation
        terms, angles = double_excitation(3, 11, 19, 27, 0.9) if n >= 28 else double_excitation(1, n // 3, 2 * n // 3, n - 2, 0.9)
        rows.append((f"(e) double excitation, 8 strings, one call, group {default}", 8, q.pauli_rotation_passes(n, terms, default),
                     timed("(e) excitation, rotations", dtype, lambda: st.apply_pauli_rotations(terms, angles))))
        low = [op for t, th in zip(terms, angles) for op in lowered(t, th)]
        cold = timed.once(lambda: st.apply_ops(low))
        RAW.append({"dtype": np.dtype(dtype).name, "call": "(e) excitation, apply_ops, first call", "ms": [cold]})
        rows.append((f"(e) the same lowered: {len(low)} ops through apply_ops, first call", len(low), None, cold))
        rows.append((f"(e) the same lowered: {len(low)} ops through apply_ops, warm", len(low), None,
                     timed("(e) excitation, apply_ops", dtype, lambda: st.apply_ops(low), warm=False)))
    del amps
    torch.cuda.empty_cache()
    return base, rows, ratios, worst, default


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pauli_rotation.md"))
    ap.add_argument("--raw", default=None, help="JSON lines of every timing (default: the page's name with .jsonl)")
    ap.add_argument("--commit", default="(not named)", help="the commit of the tree that ran, for the page")
    args = ap.parse_args()
    if not torch.cuda.is_available() or q.device_count() < 1:
        raise SystemExit("bench_rotate needs a HIP device")
    torch.cuda.init()
    check_lowering()
    lines = [f"# apply_pauli_rotations beside one gate pass, n = {args.n}", "",
             f"`tools/bench_rotate.py --n {args.n} --repeats {args.repeats}` on the tree of {args.commit}: HIP events around each call on the "
             f"handle's stream, medians of {args.repeats} after a warm-up call, one process, a dense Gaussian state drawn on the device; a "
             "batch equalled its single-term calls bit for bit before anything was timed.", ""]
    chosen = []
    for dtype in (np.complex128, np.complex64):
        base, rows, ratios, worst, default = measure(args.n, dtype, args.repeats)
        chosen.append(default)
        lines += [f"## {np.dtype(dtype).name}", "", "| call | terms / ops | passes | ms | / gate pass | per term ms |", "|---|---:|---:|---:|---:|---:|"]
        for name, terms, passes, ms in rows:
            lines.append(f"| {name} | {terms} | {'' if passes is None else passes} | {ms:.3f} | {ms / base:.2f} | {ms / terms:.3f} |")
        lines += ["", "One pass of capacity G against the single-term pass of the same x mask (the worse of x = 0 and the pair mask): "
                  + ", ".join(f"G = {c}: {worst[c]:.2f}x" for c in CAPACITIES) + f"; the largest within 1.5x: {default}.", ""]
    lines.append(f"Default of option \"rotate_group\" from this run: {min(chosen)} (the smaller of the two precisions' choices).")
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
