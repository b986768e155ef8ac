#!/usr/bin/env python
"""Time the fused pass of the noise-channel calls (include/qip_hipx.h: qipx_state_apply_reduce, qipx_state_apply_channels) in one
process, beside the two calls it replaces, at n = 30 and n = 26 in both precisions:

  (a) HipState.apply_reduce for 1-qubit -> 1-qubit, 2-qubit -> 1-qubit and 2-qubit -> overlapping 2-qubit steps at high positions,
      at lane-id bits and with index bit 0;
  (b) in the same run, a dense apply_op on the same qubits plus reduced_density_matrix on the next ones;
  (c) a chain of n single-qubit amplitude-damping channels (one per qubit) through HipState.apply_channels, beside the composed
      loop (reduced_density_matrix, the selection rule on the host, apply_op) a caller would write without it.

apply_reduce always runs the fused kernel, so (a) measures it for every shape; apply_channels runs the steps that (a) showed slower
than (b) in the composed form (csrc/qip_channel_plan.h: chan_fuses), so (c) is the chain as a caller gets it.

Every contender is a call that is complete when it returns (apply_op is followed by a sync), so the clock is the host's: the
time a caller waits, host round trips included.  Each contender is warmed up once, then `--repeats` rounds in which the
contenders of a shape take turns; the page gives the median and the spread (min .. max).  The operators are unitary, so the
state keeps its norm over the repeats.

    python tools/bench_noise.py [--n 30 26] [--repeats 7] [--out table.md] [--jsonl profiles/noise.jsonl]

--out gets the table that profiles/noise.md carries below its text, --jsonl every timing (profiles/noise.jsonl)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rustqip_amd as q  # noqa: E402
from rustqip_amd import noise  # noqa: E402

RAW = []


def unitary(k, seed):
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((1 << k, 1 << k)) + 1j * rng.standard_normal((1 << k, 1 << k))
    return np.linalg.qr(m)[0]


def shapes(n):
    """(name, positions acted on, positions reduced next)"""
    out = []
    for where, (p0, p1, p2) in (("high", (n - 1, n - 2, n - 3)), ("lane bits", (3, 4, 2)), ("bit 0", (0, 8, 9))):
        out.append((f"1 -> 1, {where}", [p0], [p1]))
        out.append((f"2 -> 1, {where}", [p0, p1], [p2]))
        out.append((f"2 -> 2 overlapping, {where}", [p0, p1], [p1, p2]))
    return out


def take_turns(st, repeats, group):
    """group: [(name, fn)]; {name: [ms, ...]}"""
    def once(fn):
        st.sync()
        t0 = time.perf_counter()
        fn()
        st.sync()
        return 1e3 * (time.perf_counter() - t0)

    for _, fn in group:
        once(fn)
    times = {name: [] for name, _ in group}
    for _ in range(repeats):
        for name, fn in group:
            times[name].append(once(fn))
    return times


def summary(ts):
    return statistics.median(ts), min(ts), max(ts)


def composed_chain(st, chans, us):
    """what a caller writes without apply_channels: one density pass, the rule on the host, one apply per channel"""
    for ch, u in zip(chans, us):
        rho = st.reduced_density_matrix(ch.qubits)
        w = np.array([float(np.real(np.trace(np.conj(K).T @ K @ rho))) for K in ch.kraus])
        r, cum = u * float(np.sum(w)), np.cumsum(w)
        hits = np.nonzero(r < cum)[0]
        i = int(hits[0]) if len(hits) else int(np.max(np.nonzero(w > 0)[0]))
        k = np.sqrt(float(np.real(np.trace(rho))) / w[i]) * ch.kraus[i]
        st.apply_op(q.make_matrix_op(ch.qubits[::-1], k.reshape(-1)))
    st.sync()


def bench(n, dtype, repeats, lines):
    name = "Complex<f64>" if dtype == np.complex128 else "Complex<f32>"
    with q.HipState(n, dtype) as st:
        st.init_basis(0)
        h = np.array([1, 1, 1, -1]) / np.sqrt(2.0)
        st.apply_ops([q.make_matrix_op([qb], h) for qb in range(n)])
        st.sync()
        lines.append(f"\n### n = {n}, {name}\n")
        lines.append("| step | fused pass (a) | apply_op | reduced_density | composed (b) | (a) / (b) |")
        lines.append("|---|---|---|---|---|---|")
        for i, (what, apos, bpos) in enumerate(shapes(n)):
            a, b = [n - 1 - p for p in apos], [n - 1 - p for p in bpos]
            m = unitary(len(a), i)
            op = q.make_matrix_op(a[::-1], m.reshape(-1))
            times = take_turns(st, repeats, [
                ("fused", lambda: st.apply_reduce(a, m, b)),
                ("apply", lambda: st.apply_op(op)),
                ("density", lambda: st.reduced_density_matrix(b)),
                ("composed", lambda: (st.apply_op(op), st.reduced_density_matrix(b))),
            ])
            f, ap, de, co = (summary(times[k]) for k in ("fused", "apply", "density", "composed"))
            RAW.append({"n": n, "dtype": name, "step": what, "positions": [apos, bpos], "ms": times})
            cell = lambda s: f"{s[0]:.2f} ({s[1]:.2f} .. {s[2]:.2f})"  # noqa: E731
            lines.append(f"| {what} | {cell(f)} | {cell(ap)} | {cell(de)} | {cell(co)} | {f[0] / co[0]:.2f} |")
        chans = [noise.amplitude_damping(qb, 0.05) for qb in range(n)]
        us = np.random.default_rng(n).random(n)
        times = take_turns(st, max(repeats // 2, 3), [("apply_channels", lambda: st.apply_channels(chans, us)),
                                                     ("composed loop", lambda: composed_chain(st, chans, us))])
        RAW.append({"n": n, "dtype": name, "step": f"chain of {n} amplitude-damping channels", "ms": times})
        c, l = summary(times["apply_channels"]), summary(times["composed loop"])
        lines.append(f"\nChain of {n} single-qubit amplitude-damping channels, one per qubit ({st.channel_passes(chans)[0]} passes against "
                     f"{2 * n}): apply_channels {c[0]:.1f} ms ({c[1]:.1f} .. {c[2]:.1f}), composed loop {l[0]:.1f} ms ({l[1]:.1f} .. {l[2]:.1f}), "
                     f"ratio {c[0] / l[0]:.2f}.")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[30, 26])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None, help="the measured table as markdown")
    ap.add_argument("--jsonl", default=None, help="every timing, one record per line")
    args = ap.parse_args()
    lines = ["## Measured: the fused pass beside the two calls it replaces (ms: median (min .. max))"]
    for n in args.n:
        for dtype in (np.complex128, np.complex64):
            bench(n, dtype, args.repeats, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    if args.jsonl:
        os.makedirs(os.path.dirname(os.path.abspath(args.jsonl)), exist_ok=True)
        with open(args.jsonl, "w") as f:
            for rec in RAW:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
