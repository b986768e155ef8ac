#!/usr/bin/env python3
"""Time the two-state Pauli calls and HipState.adjoint_gradient (include/qip_hipx.h) beside the calls they are built next to,
in one process.

For Complex<f64> and Complex<f32> at n qubits (default 30), on dense random states (Gaussian amplitudes drawn on the device by
torch, normalised, wrapped by the handles):

  (a) dst <- H src for 1, 4, 16 and 32 terms that share one x mask, one pass each (option "sum_group" raised to 32), for x = 0
      and for a pair mask, against ONE apply_pauli_rotations pass of one term of the same mask: what the kernel capacities
      cost — the default of "sum_group" is the largest capacity whose pass stays within 1.5x of the single-term pass in every
      row.  A sum pass touches three vectors (read src, read and write dst; the first pass of a storing call two), a rotation two;
  (b) <bra| P |ket> for 1 and 16 terms of one x mask against expect_pauli of the same terms: two vectors read against one;
  (c) adjoint_gradient for an ansatz of T = 16 random strings and an observable of 30 terms (15 of a ZZ chain, 15 random
      strings) from |0..0>, against
      parameter shift through the calls that were there before: 2T runs of init_basis + apply_pauli_rotations + expectation.

Every figure is the median of `--repeats` host-clock timings around a call that ends in a synchronise of the handle's stream,
after one warm-up call (parameter shift: one timing after a warm-up energy); the raw timings go to `--raw` as JSON lines.
Before any time is reported the sum of a two-term call is held to apply_pauli_rotations, the matrix elements of one state to
expect_pauli, and the adjoint gradient to the parameter-shift gradient.  Writes a markdown page (default
profiles/adjoint_gradient.md) and prints it.

    python tools/bench_adjoint.py [--n 30] [--repeats 5] [--out profiles/adjoint_gradient.md] [--commit NAME]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch  # (before the library: the states are drawn by torch on the device the library then wraps)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rustqip_amd as q  # noqa: E402

CAPACITIES = (1, 4, 16, 32)
T_ANSATZ, OBS_TERMS = 16, 30
RAW = []


def term_of_masks(n, x, z):
    """X on x & ~z, Z on z & ~x, Y on x & z (masks over amplitude-index bits; qubit q is bit n - 1 - q)"""
    term = {}
    for b in range(n):
        bx, bz = (x >> b) & 1, (z >> b) & 1
        if bx or bz:
            term[n - 1 - b] = "Y" if bx and bz else ("X" if bx else "Z")
    return term


def timed(name, dtype, fn, sync, repeats, warm=True):
    """median of `repeats` host-clock timings of fn() + sync(), in ms"""
    if warm:
        fn()
        sync()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        sync()
        times.append((time.perf_counter() - t0) * 1e3)
    RAW.append({"dtype": np.dtype(dtype).name, "call": name, "ms": times})
    return statistics.median(times)


def measure(n, dtype, repeats):
    rng = np.random.default_rng(3131)
    torch.manual_seed(31)
    tdtype = torch.complex128 if dtype == np.complex128 else torch.complex64
    u = 2.0 ** -53 if dtype == np.complex128 else 2.0 ** -24
    a_amps = torch.randn(1 << n, dtype=tdtype, device="cuda")
    a_amps /= torch.linalg.vector_norm(a_amps)
    b_amps = torch.randn(1 << n, dtype=tdtype, device="cuda")
    b_amps /= torch.linalg.vector_norm(b_amps)
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    top = 1 << (n - 1)
    zs = [int(v) for v in rng.integers(1, 1 << n, 64)]
    pair_x = (top | 0x10412) & ((1 << n) - 1) & ~1  # a pair mask with bit 0 clear: Complex<f32> moves 16-byte elements
    rows = []
    with q.HipState(n, dtype, wrap_ptr=a_amps.data_ptr(), stream=sa.cuda_stream) as a, \
            q.HipState(n, dtype, wrap_ptr=b_amps.data_ptr(), stream=sb.cuda_stream) as b:
        def both():
            a.sync()
            b.sync()

        # ---- the checks ---------------------------------------------------------------------------------------------------
        theta, term = 0.7, term_of_masks(n, pair_x, zs[0])
        b.apply_pauli_sum(a, [{}, term], [math.cos(theta), -1j * math.sin(theta)])
        a.apply_pauli_rotations([term], [theta])
        worst, _ = a.max_abs_diff(b)
        assert worst <= 32 * u * 8 * 2.0 ** (-n / 2), f"the two-term sum is {worst} from the rotation"  # (amplitudes of size 2^(-n/2))
        some = [term_of_masks(n, x, z) for x, z in ((0, zs[1]), (0, 0), (1, zs[2]), (pair_x, zs[3]), (pair_x, zs[4]))]
        own, exp = a.pauli_matrix_elements(a, some), a.expect_pauli(some)
        assert np.max(np.abs(own.real - exp)) <= 2e-12 and np.max(np.abs(own.imag)) <= 1e-12, (own, exp)
        # ---- (a) the sum's passes ------------------------------------------------------------------------------------------
        b.set_option("sum_group", 32)
        worst = {c: 0.0 for c in CAPACITIES}
        for name, x in (("x = 0", 0), (f"x = {pair_x:#x}", pair_x)):
            one_term = [term_of_masks(n, x, zs[10])]
            rot = timed(f"(a) one rotation pass, {name}", dtype, lambda: a.apply_pauli_rotations(one_term, [0.37]), a.sync, repeats)
            rows.append((f"(a) apply_pauli_rotations, 1 term, {name}: the yardstick", 1, rot, rot))
            one = None
            for count in CAPACITIES:
                terms = [term_of_masks(n, x, z) for z in zs[10:10 + count]]
                cs = rng.standard_normal(count) + 1j * rng.standard_normal(count)
                assert q.pauli_sum_passes(n, terms, 32) == 1
                t = timed(f"(a) sum, {count} terms, {name}, store", dtype, lambda: b.apply_pauli_sum(a, terms, cs), both, repeats)
                one = t if one is None else one
                worst[count] = max(worst[count], t / one)
                rows.append((f"(a) apply_pauli_sum, {count} term(s), {name}, one storing pass", count, t, rot))
                if count in (1, 16):
                    t = timed(f"(a) sum, {count} terms, {name}, accumulate", dtype, lambda: b.apply_pauli_sum(a, terms, cs, accumulate=True), both, repeats)
                    rows.append((f"(a) apply_pauli_sum, {count} term(s), {name}, one accumulating pass", count, t, rot))
        default = max(c for c in CAPACITIES if worst[c] <= 1.5)
        b.set_option("sum_group", default)
        # ---- (b) matrix elements -------------------------------------------------------------------------------------------
        b_amps.normal_()
        b_amps /= torch.linalg.vector_norm(b_amps)
        torch.cuda.synchronize()
        for name, x in (("x = 0", 0), (f"x = {pair_x:#x}", pair_x)):
            for count in (1, 16):
                terms = [term_of_masks(n, x, z) for z in zs[10:10 + count]]
                base = timed(f"(b) expect_pauli, {count} terms, {name}", dtype, lambda: a.expect_pauli(terms), a.sync, repeats)
                rows.append((f"(b) expect_pauli, {count} term(s), {name}: the yardstick", count, base, base))
                t = timed(f"(b) matrix elements, {count} terms, {name}", dtype, lambda: b.pauli_matrix_elements(a, terms), both, repeats)
                rows.append((f"(b) pauli_matrix_elements, {count} term(s), {name}", count, t, base))
        # ---- (c) the gradient ----------------------------------------------------------------------------------------------
        string = lambda: "".join(rng.choice(list("IXYZ"), n))  # noqa: E731
        rot_terms, angles = [string() for _ in range(T_ANSATZ)], rng.uniform(-3, 3, T_ANSATZ)
        # half the observable a ZZ ring segment (from |0..0> random strings alone have expectation zero, and a gradient of zeros
        # checks nothing), half random strings
        obs = [{i: "Z", i + 1: "Z"} for i in range(OBS_TERMS // 2)] + [string() for _ in range(OBS_TERMS - OBS_TERMS // 2)]
        cs = rng.standard_normal(OBS_TERMS)

        def energy(th):
            a.init_basis(0)
            a.apply_pauli_rotations(rot_terms, th)
            return a.expectation(obs, cs)

        def shift_gradient():
            out = np.zeros(T_ANSATZ)
            for k in range(T_ANSATZ):
                d = np.zeros(T_ANSATZ)
                d[k] = math.pi / 4
                out[k] = energy(angles + d) - energy(angles - d)
            return out

        result = {}

        def adjoint():
            a.init_basis(0)
            result["adjoint"] = a.adjoint_gradient(rot_terms, angles, obs, cs, b)

        t_adj = timed("(c) adjoint_gradient", dtype, adjoint, both, max(1, min(repeats, 3)))
        energy(angles)  # (warm)
        t_shift = timed("(c) parameter shift", dtype, lambda: result.update(shift=shift_gradient()), both, 1, warm=False)
        e_adj, g_adj = result["adjoint"]
        S = float(np.sum(np.abs(cs)))
        bar_e = S * ((24 * T_ANSATZ + OBS_TERMS + 8) * u + 1e-12)
        bar = 2 * S * ((48 * T_ANSATZ + OBS_TERMS + 8) * u + 1e-12) + 2 * bar_e  # the adjoint's bar plus parameter shift's two energies
        apart = float(np.max(np.abs(g_adj - result["shift"])))
        print(f"{np.dtype(dtype).name}: E = {e_adj:+.12f}, adjoint gradient {np.array2string(g_adj, precision=6)}, "
              f"parameter shift {np.array2string(result['shift'], precision=6)}", flush=True)
        assert apart <= bar and abs(e_adj - energy(angles)) <= 2 * bar_e, (apart, bar, e_adj)
        assert float(np.max(np.abs(g_adj))) > 1e-3, "the gradient is too small to check anything"
        passes = 3 * T_ANSATZ + q.pauli_sum_passes(n, obs, default) + T_ANSATZ + 1
        rows.append((f"(c) adjoint_gradient, T = {T_ANSATZ}, {OBS_TERMS}-term observable ({passes} passes over one or two vectors)", T_ANSATZ, t_adj, t_shift))
        rows.append((f"(c) parameter shift: {2 * T_ANSATZ} x (init_basis, {T_ANSATZ} rotations, expectation): the yardstick", T_ANSATZ, t_shift, t_shift))
        extra = f"The two gradients are {apart:.2e} apart (bar {bar:.2e}, largest component {float(np.max(np.abs(g_adj))):.3f}); parameter shift / adjoint = {t_shift / t_adj:.1f}x."
    del a_amps, b_amps
    torch.cuda.empty_cache()
    return rows, worst, default, extra, t_shift / t_adj


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adjoint_gradient.md"))
    ap.add_argument("--raw", default=None, help="JSON lines of every timing (default: the page's name with .jsonl)")
    ap.add_argument("--commit", default="(not named)", help="the commit of the tree that ran, for the page")
    args = ap.parse_args()
    if not torch.cuda.is_available() or q.device_count() < 1:
        raise SystemExit("bench_adjoint needs a HIP device")
    torch.cuda.init()
    lines = [f"# apply_pauli_sum, pauli_matrix_elements and adjoint_gradient, n = {args.n}", "",
             f"`tools/bench_adjoint.py --n {args.n} --repeats {args.repeats}` on the tree of {args.commit}: a host clock around each call "
             f"and a synchronise of the streams it used, medians of {args.repeats} after a warm-up call, one process, dense Gaussian states "
             "drawn on the device; the sum was held to a rotation, the matrix elements to expect_pauli and the adjoint gradient to "
             "parameter shift before anything was reported.", ""]
    chosen, ratios = [], []
    for dtype in (np.complex128, np.complex64):
        rows, worst, default, extra, ratio = measure(args.n, dtype, args.repeats)
        chosen.append(default)
        ratios.append(ratio)
        lines += [f"## {np.dtype(dtype).name}", "", "| call | terms | ms | / its yardstick |", "|---|---:|---:|---:|"]
        for name, terms, ms, base in rows:
            lines.append(f"| {name} | {terms} | {ms:.3f} | {ms / base:.2f} |")
        lines += ["", "One storing sum pass of capacity G against the single-term pass of the same x mask (the worse of x = 0 and the pair "
                  "mask): " + ", ".join(f"G = {c}: {worst[c]:.2f}x" for c in CAPACITIES) + f"; the largest within 1.5x: {default}.", "", extra, ""]
    lines.append(f"Default of option \"sum_group\" from this run: {min(chosen)} (the smaller of the two precisions' choices).  Parameter shift "
                 f"over adjoint: {ratios[0]:.1f}x (complex128), {ratios[1]:.1f}x (complex64).")
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
