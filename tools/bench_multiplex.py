#!/usr/bin/env python
"""Time HipState.apply_multiplexed (include/qip_hipx.h: qipx_state_apply_multiplexed) in one process, both precisions:

  shapes   k = 1, 2; m = 1, 4, 10, 16; the select bits all high, all inside the wave row (m <= 6 - k) or mixed; a target inside the
           row or outside it
  (a)      one dense gate pass of the same k on the same targets through apply_op: the in-place floor every shape is given relative to
  (b)      the same map as 2^m controlled gates (X-conjugated) through default apply_ops, m = 2 and 4
  (c)      the same map as one block-diagonal dense op through apply_op, m + k <= 6
  (d)      multiplex.prepare_register on a whole state of k = 10 and 19 qubits beside upload of the same amplitudes (m + 2k <= 20
           holds the last Ry pass of a register to 18 select qubits: 19 is the largest register)

HIP events around each call on the handle's stream (the call's host work, rounding and staging its table, included), every contender
warmed up once, then `--repeats` rounds in which the contenders of a group take turns; the page gives the median and the spread
(min .. max) of each.  Before a shape is timed the call is held bit for bit against tests/multiplex_ref.py's spec on a sub-cube of
the timed state that is closed under the map (the select and target positions and two more, every other index bit fixed).

    python tools/bench_multiplex.py [--n 30 26] [--repeats 5] [--out profiles/multiplex.md] [--commit NAME]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch  # (before the library: the state is drawn by torch on the device the library then wraps)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import multiplex_ref as R  # noqa: E402
import rustqip_amd as q  # noqa: E402
from rustqip_amd import circuits, multiplex  # noqa: E402

RAW = []


def time_group(st, stream, repeats, tag, group):
    """group: [(name, fn)]: each warmed up once, then `repeats` rounds in which they take turns; {name: (median, min, max)}"""
    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _, fn in group:
        fn()
    st.sync()
    times = {name: [] for name, _ in group}
    for _ in range(repeats):
        for name, fn in group:
            times[name].append(once(fn))
    for name, ts in times.items():
        RAW.append({"case": tag, "call": name, "ms": ts})
        print(f"{tag} {name}: {statistics.median(ts):.3f} ms", flush=True)
    return {name: (statistics.median(ts), min(ts), max(ts)) for name, ts in times.items()}


def held_to_spec(st, n, spos, tpos, table, rng):
    """the call on the timed state, compared bit for bit with the spec on a closed sub-cube"""
    extra = [p for p in rng.permutation(n) if p not in spos and p not in tpos][:2]
    cube = sorted(list(spos) + list(tpos) + [int(p) for p in extra])
    fixed = int(rng.integers(0, 1 << n)) & ~sum(1 << p for p in cube)
    j = np.arange(1 << len(cube), dtype=np.uint64)
    idx = np.full_like(j, fixed)
    for i, p in enumerate(cube):
        idx |= ((j >> np.uint64(i)) & np.uint64(1)) << np.uint64(p)
    sub = lambda ps: [len(cube) - 1 - cube.index(p) for p in ps]  # noqa: E731  (the sub-cube's qubits)
    before = st.download_indices(idx)
    st.apply_multiplexed([n - 1 - p for p in spos], [n - 1 - p for p in tpos], table)
    after = st.download_indices(idx)
    want = R.apply_multiplexed_spec(len(cube), before, sub(spos), sub(tpos), table)
    assert np.array_equal(after.view(np.uint8), want.view(np.uint8)), ("the call differs from the spec", n, spos, tpos)


def shapes(n):
    """(label, select positions, target positions)"""
    out = []
    for k in (1, 2):
        for tname, tpos in (("row", [2, 4][:k]), ("outside", [n - 8, n - 12][:k])):
            for m in (1, 4, 10, 16):
                if m + 2 * k > 20:
                    continue
                free_high = [p for p in range(n - 1, 5, -1) if p not in tpos]
                free_row = [p for p in (0, 1, 3, 5, 2, 4) if p not in tpos]
                out.append((f"k={k} target {tname} m={m} select high", free_high[:m], tpos))
                if m <= 6 - k and tname == "row":
                    out.append((f"k={k} target {tname} m={m} select in row", free_row[:m], tpos))
                if m >= 4:
                    half = m // 2
                    out.append((f"k={k} target {tname} m={m} select mixed", free_row[: min(half, len(free_row))] + free_high[: m - min(half, len(free_row))], tpos))
    return out


def controlled_route(select, targets, table):
    ops = []
    for xv, g in enumerate(table):
        flips = [q.make_matrix_op([s], circuits.X) for i, s in enumerate(select) if not (xv >> i) & 1]
        ops += flips + [q.make_control_op(list(select), q.make_matrix_op(list(targets)[::-1], g))] + flips
    return ops


def measure(n, dtype, repeats):
    rng = np.random.default_rng(1618)
    torch.manual_seed(33)
    amps = torch.randn(1 << n, dtype=torch.complex128 if dtype == np.complex128 else torch.complex64, device="cuda")
    amps /= torch.linalg.vector_norm(amps)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    tag = f"{np.dtype(dtype).name} n={n}"
    rows, others = [], []
    with q.HipState(n, dtype, wrap_ptr=amps.data_ptr(), stream=stream.cuda_stream) as st:
        floors = {}
        for label, spos, tpos in shapes(n):
            select, targets = [n - 1 - p for p in spos], [n - 1 - p for p in tpos]
            table = R.unitary_table(rng, len(spos), len(tpos))
            held_to_spec(st, n, spos, tpos, table, rng)
            gate = q.make_matrix_op(targets[::-1], table[0])
            res = time_group(st, stream, repeats, tag, [
                (f"gate pass {tpos}", lambda: st.apply_op(gate)),
                (label, lambda: st.apply_multiplexed(select, targets, table)),
            ])
            floors[tuple(tpos)] = res[f"gate pass {tpos}"]
            rows.append((label, res[label], res[f"gate pass {tpos}"]))
        for k, tpos in ((1, [2]), (1, [n - 8]), (2, [2, n - 12])):
            for m in (2, 4):
                spos = [n - 1, 0, n - 3, 5][:m]
                select, targets = [n - 1 - p for p in spos], [n - 1 - p for p in tpos]
                table = R.unitary_table(rng, m, k)
                group = [(f"apply_multiplexed m={m} k={k} targets {tpos}", lambda: st.apply_multiplexed(select, targets, table))]
                route = st.compile_ops(controlled_route(select, targets, table))
                group.append((f"(b) {1 << m} controlled gates through apply_ops", lambda route=route: st.apply_compiled(route)))
                if m + k <= 6:
                    dense = q.make_matrix_op(R.index_order(select, targets), R.block_diagonal(table))
                    group.append((f"(c) one block-diagonal dense op on {m + k} qubits", lambda dense=dense: st.apply_op(dense)))
                res = time_group(st, stream, repeats, tag, group)
                others.append(list(res.items()))
    del amps
    torch.cuda.empty_cache()
    return rows, others


def measure_prepare(dtype, repeats):
    out = []
    for k in (10, 19):
        psi = R.random_amplitudes(np.random.default_rng(k), k)
        stream = torch.cuda.Stream()
        buf = torch.zeros(1 << k, dtype=torch.complex128 if dtype == np.complex128 else torch.complex64, device="cuda")
        torch.cuda.synchronize()
        with q.HipState(k, dtype, wrap_ptr=buf.data_ptr(), stream=stream.cuda_stream) as st:
            qubits = list(range(k))[::-1]
            host = psi.astype(dtype)

            def prepare():
                st.init_basis(0)
                multiplex.prepare_register(st, qubits, psi)

            res = time_group(st, stream, repeats, f"{np.dtype(dtype).name} prepare k={k}", [
                (f"(d) prepare_register k={k}", prepare), (f"(d) upload of 2^{k} amplitudes", lambda: st.upload(host))])
            prepare()
            got = st.download()
            assert np.linalg.norm(got.astype(np.complex128) - psi) <= (9 * k + 8) * R.UNIT[dtype]
            out.append(list(res.items()))
    return out


def fmt(t):
    return f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, nargs="+", default=[30, 26])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multiplex.md"))
    ap.add_argument("--raw", default=None, help="JSON lines of every timing (default: the page's name with .jsonl)")
    ap.add_argument("--commit", default="(not named)", help="the commit of the tree that ran, for the page")
    args = ap.parse_args()
    if not torch.cuda.is_available() or q.device_count() < 1:
        raise SystemExit("bench_multiplex needs a HIP device")
    torch.cuda.init()
    lines = [f"# apply_multiplexed beside a gate pass, controlled gates and a block-diagonal dense op, n = {args.n}", "",
             f"`tools/bench_multiplex.py --n {' '.join(map(str, args.n))} --repeats {args.repeats}` on the tree of {args.commit}: HIP events "
             "around each call on the handle's stream (the call's host work — rounding and staging its table — included), every contender "
             f"warmed up, then {args.repeats} rounds in which the contenders of a group take turns; median (min .. max) in ms, one "
             "process, a dense Gaussian state drawn on the device.  Every shape was bit-equal to the spec on a closed sub-cube of the "
             "timed state before timing.  Positions are index positions (qubit q = position n-1-q); the row is positions 0..5.", ""]
    RAW.append({"commit": args.commit})
    for n in args.n:
        for dtype in (np.complex128, np.complex64):
            rows, others = measure(n, dtype, args.repeats)
            lines += [f"## {np.dtype(dtype).name}, n = {n}", "", "| shape | call ms | (a) gate pass ms | call / (a) |", "|---|---:|---:|---:|"]
            for label, t, floor in rows:
                lines.append(f"| {label} | {fmt(t)} | {fmt(floor)} | {t[0] / floor[0]:.2f} |")
            lines += ["", "the same map by other routes", "", "| route | ms | / call |", "|---|---:|---:|"]
            for group in others:
                call = group[0][1][0]
                for name, t in group:
                    lines.append(f"| {name} | {fmt(t)} | {t[0] / call:.2f} |")
            lines.append("")
    for dtype in (np.complex128, np.complex64):
        lines += [f"## prepare_register, {np.dtype(dtype).name}", "", "| route | ms |", "|---|---:|"]
        for group in measure_prepare(dtype, args.repeats):
            for name, t in group:
                lines.append(f"| {name} | {fmt(t)} |")
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
