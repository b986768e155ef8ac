#!/usr/bin/env python
"""Time HipState.apply_function (include/qip_hipx.h: qipx_state_apply_function) in one process at n = 30, both precisions:

  (a) one call per shape — XOR and ADD with m = 16, k = 12 (6 out positions outside the wave row), a phase table on 16 qubits
      (k = 0), a two-pass XOR (7 out positions outside the row) — beside one H gate pass on the same state, the in-place floor;
  (b) the same map as a SparseMatrix op on m + k = 8 and 12 qubits through apply_op, beside the call;
  (c) an 8-bit classical.add beside the Toffoli ripple-carry adder (one carry qubit) through default apply_ops.

HIP events around each call on the handle's stream, every contender warmed up once, then `--repeats` rounds in which the
contenders of a group take turns; the page gives the median and the spread (min .. max) of each.  Before anything is timed the
call is held against the SparseMatrix op on the timed state itself (IEEE-equal).

    python tools/bench_function.py [--n 30] [--repeats 7] [--out profiles/classical_function.md] [--commit NAME]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch  # (before the library: the state is drawn by torch on the device the library then wraps)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rustqip_amd as q  # noqa: E402
from rustqip_amd import circuits, classical  # noqa: E402

RAW = []


def sparse_rows(m, k, values, mode):
    """the map on m + k op qubits (in register first, bit i = op qubit i) as SparseMatrix rows: new[r] = old[column]"""
    size = m + k
    j = np.arange(1 << size, dtype=np.uint64)
    gather = lambda lo, cnt: sum((((j >> np.uint64(size - 1 - (lo + i))) & np.uint64(1)) << np.uint64(i)) for i in range(cnt))  # noqa: E731
    x, y = gather(0, m), gather(m, k)
    v = np.asarray(values, dtype=np.uint64)[x]
    y2 = (y ^ v) if mode == "xor" else ((y + v) & np.uint64((1 << k) - 1))
    to = j.copy()
    for i in range(k):
        bit = np.uint64(size - 1 - (m + i))
        to = (to & ~(np.uint64(1) << bit)) | (((y2 >> np.uint64(i)) & np.uint64(1)) << bit)
    rows = [None] * (1 << size)
    for col, r in enumerate(to):
        rows[int(r)] = [(col, 1.0)]
    return rows


def ripple_carry_adder(a, b, carry):
    """b <- a + b mod 2^len(b): MAJ upwards, UMA downwards (Cuccaro et al. 2004, without the carry-out)"""
    cnot = lambda c, t: q.make_control_op([c], q.make_matrix_op([t], circuits.X))  # noqa: E731
    toffoli = lambda c1, c2, t: q.make_control_op([c1, c2], q.make_matrix_op([t], circuits.X))  # noqa: E731
    cs = [carry] + list(a[:-1])
    ops = []
    for c, bi, ai in zip(cs, b, a):
        ops += [cnot(ai, bi), cnot(ai, c), toffoli(c, bi, ai)]
    for c, bi, ai in reversed(list(zip(cs, b, a))):
        ops += [toffoli(c, bi, ai), cnot(ai, c), cnot(c, bi)]
    return ops


def time_group(st, stream, repeats, dtype, group):
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
        RAW.append({"dtype": np.dtype(dtype).name, "call": name, "ms": ts})
        print(f"{np.dtype(dtype).name} {name}: {statistics.median(ts):.3f} ms", flush=True)
    return {name: (statistics.median(ts), min(ts), max(ts)) for name, ts in times.items()}


def measure(n, dtype, repeats):
    rng = np.random.default_rng(2718)
    torch.manual_seed(32)
    amps = torch.randn(1 << n, dtype=torch.complex128 if dtype == np.complex128 else torch.complex64, device="cuda")
    amps /= torch.linalg.vector_norm(amps)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    pos = lambda ps: [n - 1 - p for p in ps]  # noqa: E731  (index positions -> qubits)
    out = {}
    with q.HipState(n, dtype, wrap_ptr=amps.data_ptr(), stream=stream.cuda_stream) as st:
        # held before timing: the call against the SparseMatrix op on a copy of the timed state
        ins, outs = pos([20, 3, 9]), pos([14, 2, 25, 7, 0])
        values = rng.integers(0, 32, size=8, dtype=np.uint64)
        with q.HipState(n, dtype) as twin:
            twin.copy_from(st)
            twin.apply_op(q.make_sparse_matrix_op(ins + outs, sparse_rows(3, 5, values, "add")))
            st.apply_function(ins, outs, values=values, mode="add")
            assert st.max_abs_diff(twin) == (0.0, 0)
        # (a)
        in16 = pos(list(range(14, 30)))
        out12 = pos([0, 1, 2, 3, 4, 5, 6, 8, 9, 11, 12, 13])
        v12 = rng.integers(0, 1 << 12, size=1 << 16, dtype=np.uint64)
        ph16 = rng.uniform(-3, 3, size=1 << 16)
        out2p = pos([6, 7, 8, 9, 10, 11, 12, 2])
        v2p = rng.integers(0, 1 << 8, size=8, dtype=np.uint64)
        h = q.make_matrix_op([0], circuits.H)
        assert st.function_passes(in16, out12) == 1 and st.function_passes(pos([20, 21, 22]), out2p) == 2
        out["a"] = time_group(st, stream, repeats, dtype, [
            ("H gate pass", lambda: st.apply_op(h)),
            ("XOR m=16 k=12", lambda: st.apply_function(in16, out12, values=v12)),
            ("ADD m=16 k=12", lambda: st.apply_function(in16, out12, values=v12, mode="add")),
            ("XOR m=16 k=12 with phases", lambda: st.apply_function(in16, out12, values=v12, phases=ph16)),
            ("phase table m=16 k=0", lambda: st.apply_function(in16, [], phases=ph16)),
            ("XOR m=3, 7 out positions outside the row (2 passes)", lambda: st.apply_function(pos([20, 21, 22]), out2p, values=v2p)),
            ("H gate pass (again)", lambda: st.apply_op(h)),
        ])
        # (b)
        out["b"] = {}
        for m, k in ((3, 5), (5, 7)):
            qs = [int(v) for v in rng.permutation(n)[: m + k]]
            vals = rng.integers(0, 1 << k, size=1 << m, dtype=np.uint64)
            for mode in ("xor", "add"):
                if mode == "add" and sum(1 for t in qs[m:] if n - 1 - t >= 6) > 6:
                    continue
                op = q.make_sparse_matrix_op(qs, sparse_rows(m, k, vals, mode))
                res = time_group(st, stream, repeats, dtype, [
                    (f"SparseMatrix op {mode} m+k={m + k}", lambda op=op: st.apply_op(op)),
                    (f"apply_function {mode} m+k={m + k}", lambda qs=qs, vals=vals, mode=mode, m=m: st.apply_function(qs[:m], qs[m:], values=vals, mode=mode)),
                    (f"SparseMatrix op {mode} m+k={m + k} (again)", lambda op=op: st.apply_op(op)),
                ])
                out["b"][(m + k, mode, st.function_passes(qs[:m], qs[m:], mode))] = list(res.values())
        # (c)
        # (the registers interleaved on index positions 0 .. 15, b on the even ones: five of its positions outside the row; an
        # ADD holds at most six there, so an 8-bit out register needs two of its qubits inside the six low index bits)
        a, b = pos([1 + 2 * i for i in range(8)]), pos([2 * i for i in range(8)])
        adder = st.compile_ops(ripple_carry_adder(a, b, pos([16])[0]))
        out["c"] = time_group(st, stream, repeats, dtype, [
            ("Toffoli ripple-carry adder, 48 ops through apply_ops", lambda: st.apply_compiled(adder)),
            ("classical.add, 8 bits", lambda: classical.add(st, a, b)),
            ("Toffoli ripple-carry adder (again)", lambda: st.apply_compiled(adder)),
        ])
    del amps
    torch.cuda.empty_cache()
    return out


def fmt(t):
    return f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classical_function.md"))
    ap.add_argument("--raw", default=None, help="JSON lines of every timing (default: the page's name with .jsonl)")
    ap.add_argument("--commit", default="(not named)", help="the commit of the tree that ran, for the page")
    args = ap.parse_args()
    if not torch.cuda.is_available() or q.device_count() < 1:
        raise SystemExit("bench_function needs a HIP device")
    torch.cuda.init()
    lines = [f"# apply_function beside a gate pass, SparseMatrix ops and a Toffoli adder, n = {args.n}", "",
             f"`tools/bench_function.py --n {args.n} --repeats {args.repeats}` on the tree of {args.commit}: HIP events around each call on "
             f"the handle's stream (the call's host work — building and staging its table — included), every contender warmed up, then "
             f"{args.repeats} rounds in which the contenders of a group take turns; median (min .. max) in ms, one process, a dense "
             "Gaussian state drawn on the device.  The call was IEEE-equal to the SparseMatrix op on the timed state before timing.", ""]
    for dtype in (np.complex128, np.complex64):
        res = measure(args.n, dtype, args.repeats)
        floor = res["a"]["H gate pass"][0]
        lines += [f"## {np.dtype(dtype).name}", "", "(a) one call per shape", "", "| call | ms | / H gate pass |", "|---|---:|---:|"]
        for name, t in res["a"].items():
            lines.append(f"| {name} | {fmt(t)} | {t[0] / floor:.2f} |")
        lines += ["", "(b) the same map as a SparseMatrix op through apply_op", "",
                  "| m + k | mode | passes | SparseMatrix op ms | apply_function ms | SparseMatrix op again ms | op / call |", "|---:|---|---:|---:|---:|---:|---:|"]
        for (mk, mode, passes), (sp, fn, sp2) in res["b"].items():
            lines.append(f"| {mk} | {mode} | {passes} | {fmt(sp)} | {fmt(fn)} | {fmt(sp2)} | {min(sp[0], sp2[0]) / fn[0]:.2f}x |")
        lines += ["", "(c) an 8-bit in-place addition", "", "| route | ms |", "|---|---:|"]
        for name, t in res["c"].items():
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
