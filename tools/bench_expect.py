#!/usr/bin/env python3
"""Time HipState.expect_pauli (include/qip_hipx.h) beside norm_sqr, in one process.

For Complex<f64> and Complex<f32> at n qubits (default 30), on a dense random state (Gaussian amplitudes drawn on the device by
torch, normalised, wrapped by the handle):

  (a) norm_sqr: one read of the vector, the yardstick;
  (b) one Z-only term (x = 0);
  (c) one term each with x = bit 0, x = the top bit, x = all bits;
  (d) 4, 16 and 32 terms that share one x mask, one pass each (option "expect_group" raised to 32), for x = 0 and for a pair
      mask: what the kernel capacities 1, 4, 16, 32 cost — the default of "expect_group" is the largest capacity whose pass
      stays within 1.5x of the single-term pass in every row;
  (e) a 1000-term list over about 60 distinct x masks, with its number of passes, at the default group.

Every timed call ends in a synchronise of its own (the results go back to the host), so a host clock around it is the time;
medians over `--repeats` after one warm-up call.  Before any time is reported a batch is held to its single-term calls (exactly)
and the empty term to norm_sqr.  Writes a markdown page (default profiles/expect_pauli.md) and prints it.

    python tools/bench_expect.py [--n 30] [--repeats 7] [--out profiles/expect_pauli.md]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch  # (before the library: the state is drawn by torch on the device the library then wraps)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rustqip_amd as q  # noqa: E402

CAPACITIES = (1, 4, 16, 32)


def term_of_masks(n, x, z):
    """X on x & ~z, Z on z & ~x, Y on x & z (masks over amplitude-index bits; qubit q is bit n - 1 - q)"""
    term = {}
    for b in range(n):
        bx, bz = (x >> b) & 1, (z >> b) & 1
        if bx or bz:
            term[n - 1 - b] = "Y" if bx and bz else ("X" if bx else "Z")
    return term


def timed(fn, repeats):
    fn()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def measure(n, dtype, repeats):
    rng = np.random.default_rng(3030)
    torch.manual_seed(30)
    amps = torch.randn(1 << n, dtype=torch.complex128 if dtype == np.complex128 else torch.complex64, device="cuda")
    amps /= torch.linalg.vector_norm(amps)
    torch.cuda.synchronize()
    full, top = (1 << n) - 1, 1 << (n - 1)
    zs = [int(v) for v in rng.integers(1, 1 << n, 64)]
    pair_x = top | 0x10412  # a pair mask with bit 0 clear: Complex<f32> reads 16-byte elements
    rows = []
    with q.HipState(n, dtype, wrap_ptr=amps.data_ptr()) as st:
        # the checks: a batch is its single-term calls, the empty term is the norm
        some = [term_of_masks(n, x, z) for x, z in ((0, zs[0]), (0, 0), (1, zs[1]), (pair_x, zs[2]), (pair_x, zs[3]), (full, zs[4]))]
        batch = st.expect_pauli(some)
        assert np.array_equal(batch, np.array([st.expect_pauli([t])[0] for t in some])), "a batch differs from its single-term calls"
        assert abs(batch[1] - st.norm_sqr()) <= 1e-6 and abs(batch[1] - 1.0) <= 1e-5, batch[1]
        base = timed(st.norm_sqr, repeats)
        rows.append(("(a) norm_sqr", 1, 1, base))
        single = {}
        for name, x, z in (("(b) one Z-only term", 0, zs[5]), ("(c) one term, x = bit 0", 1, zs[6]), ("(c) one term, x = the top bit", top, zs[7]),
                           ("(c) one term, x = all bits", full, zs[8])):
            terms = [term_of_masks(n, x, z)]
            single[x] = timed(lambda: st.expect_pauli(terms), repeats)
            rows.append((name, 1, 1, single[x]))
        st.set_option("expect_group", 32)
        worst = {c: 0.0 for c in CAPACITIES}
        for name, x in (("x = 0", 0), (f"x = {pair_x:#x}", pair_x)):
            one = None
            for count in CAPACITIES:
                terms = [term_of_masks(n, x, z) for z in zs[10:10 + count]]
                assert q.expect_pauli_passes(n, terms, 32) == 1
                t = timed(lambda: st.expect_pauli(terms), repeats)
                one = t if one is None else one
                worst[count] = max(worst[count], t / one)
                rows.append((f"(d) {count} term(s), {name}, one pass", count, 1, t))
        default = max(c for c in CAPACITIES if worst[c] <= 1.5)
        st.set_option("expect_group", default)
        xs = sorted({int(v) for v in rng.integers(0, 1 << n, 59)} | {0})
        picks = [xs[int(rng.integers(0, len(xs)))] for _ in range(1000)]
        many = [term_of_masks(n, x, int(rng.integers(0, 1 << n))) for x in picks]
        passes = q.expect_pauli_passes(n, many, default)
        rows.append((f"(e) 1000 terms over {len(set(picks))} x masks, group {default}", 1000, passes,
                     timed(lambda: st.expect_pauli(many), max(repeats // 2, 1))))
    del amps
    torch.cuda.empty_cache()
    return base, rows, worst, default


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expect_pauli.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available() or q.device_count() < 1:
        raise SystemExit("bench_expect needs a HIP device")
    torch.cuda.init()
    lines = [f"# expect_pauli beside norm_sqr, n = {args.n}", "",
             f"`tools/bench_expect.py --n {args.n} --repeats {args.repeats}`: host clock around calls that end in a synchronise, medians of "
             f"{args.repeats} after a warm-up call, one process, a dense Gaussian state drawn on the device; a batch equalled its "
             "single-term calls bit for bit and the empty term equalled norm_sqr before anything was timed.", ""]
    chosen = []
    for dtype in (np.complex128, np.complex64):
        base, rows, worst, default = measure(args.n, dtype, args.repeats)
        chosen.append(default)
        lines += [f"## {np.dtype(dtype).name}", "", "| call | terms | passes | ms | / norm_sqr | per term ms |", "|---|---:|---:|---:|---:|---:|"]
        for name, terms, passes, ms in rows:
            lines.append(f"| {name} | {terms} | {passes} | {ms:.3f} | {ms / base:.2f} | {ms / terms:.3f} |")
        lines += ["", "One pass of capacity G against the single-term pass of the same x mask (the worse of x = 0 and the pair mask): "
                  + ", ".join(f"G = {c}: {worst[c]:.2f}x" for c in CAPACITIES) + f"; the largest within 1.5x: {default}.", ""]
    lines.append(f"Default of option \"expect_group\" from this run: {min(chosen)} (the smaller of the two precisions' choices).")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
