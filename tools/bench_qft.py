#!/usr/bin/env python
"""Time HipState.apply_qft (include/qip_hipx.h: qipx_state_apply_qft) in one process, both precisions:

  shapes   m = 12 on index bits 0..11 (one pass) and on the top 12 bits (two tile passes), m = 16 on the top bits, m = n;
           natural order and QIPX_QFT_REVERSED
  (a)      one H gate pass (apply_op) in the same group: the per-pass floor; the page gives call / (passes x (a))
  (b)      apply_ops(fourier.qft_ops(..)) on the same register, every shape in three modes: the default (the interpreter's
           sweeps), run-time-compiled sweeps that are IEEE-equal to gate by gate (tile = 1 + tile_jit), and the 1e-12 mode
           (tile = 2 + tile_jit + tile_fma + tile_merge)

HIP events around each call on the handle's stream (the call's host work, building and staging its twiddle tables, included),
every contender warmed up once, then `--repeats` rounds in which the contenders of a group take turns; the page gives the median
and the spread (min .. max) of each.  Before a shape is timed the call is compared with (b) in the default mode from the same
input on 4096 random indices.

    python tools/bench_qft.py [--n 30 26] [--repeats 5] [--out profiles/qft.md] [--commit NAME]"""
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
from rustqip_amd import circuits, fourier  # noqa: E402

RAW = []
MODES = (("(b) compiled sweeps, IEEE-equal", (("tile", 1), ("tile_jit", 1))),
         ("(b) compiled sweeps, tile_fma + tile_merge", (("tile", 2), ("tile_jit", 1), ("tile_fma", 1), ("tile_merge", 1))))


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


def shapes(n):
    """(label, index positions of the register, LSB first, reversed order?)"""
    out = []
    for label, pos in (("m=12 on index bits 0..11", list(range(12))),
                       (f"m=12 on index bits {n - 12}..{n - 1}", list(range(n - 12, n))),
                       (f"m=16 on index bits {n - 16}..{n - 1}", list(range(n - 16, n))),
                       (f"m=n={n}", list(range(n)))):
        for reversed in (False, True):
            out.append((label + (" reversed" if reversed else " natural"), pos, reversed))
    return out


def home(st, amps):
    """the state back in the torch tensor (a natural-order call of several passes leaves it in the scratch buffer)"""
    if st.device_ptr() != amps.data_ptr():
        st.swap_buffers()
    assert st.device_ptr() == amps.data_ptr()


def held_to_the_circuit(st, amps, keep, n, qubits, reversed, ops, rng, tol):
    idx = rng.integers(0, 1 << n, size=4096).astype(np.uint64)
    st.sync()
    home(st, amps)
    keep.copy_(amps)
    torch.cuda.synchronize()  # (the handle's stream is non-blocking: it would not wait for this copy)
    st.apply_qft(qubits, reversed=reversed)
    got = st.download_indices(idx)
    st.sync()
    home(st, amps)
    amps.copy_(keep)
    torch.cuda.synchronize()
    st.apply_compiled(ops)
    want = st.download_indices(idx)
    err = float(np.max(np.abs(got - want)))
    assert err <= tol, ("apply_qft differs from the lowered circuit", n, qubits, reversed, err)
    return err


def measure(n, dtype, repeats):
    rng = np.random.default_rng(2718)
    torch.manual_seed(34)
    tdtype = torch.complex128 if dtype == np.complex128 else torch.complex64
    amps = torch.randn(1 << n, dtype=tdtype, device="cuda")
    amps /= torch.linalg.vector_norm(amps)
    keep = torch.empty_like(amps)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    tag = f"{np.dtype(dtype).name} n={n}"
    tol = 1e-12 if dtype == np.complex128 else 1e-5
    rows = []
    gate = q.make_matrix_op([7], circuits.H)
    with q.HipState(n, dtype, wrap_ptr=amps.data_ptr(), stream=stream.cuda_stream) as st:
        for label, pos, reversed in shapes(n):
            qubits = [n - 1 - p for p in pos]
            passes = st.qft_passes(qubits, reversed=reversed)
            lowered = fourier.qft_ops(qubits, reversed=reversed)
            ops = st.compile_ops(lowered)
            err = held_to_the_circuit(st, amps, keep, n, qubits, reversed, ops, rng, tol)
            group = [("(a) H gate pass", lambda: st.apply_op(gate)),
                     (label, lambda: st.apply_qft(qubits, reversed=reversed)),
                     (f"(b) {len(lowered)} ops, default apply_ops", lambda: st.apply_compiled(ops))]
            res = time_group(st, stream, repeats, tag, group)
            row = {"label": label, "passes": passes, "ops": len(lowered), "err": err, "call": res[label], "floor": res["(a) H gate pass"],
                   "default": res[group[2][0]]}
            for mode, options in MODES:  # (compiled once while the group warms up, then timed)
                for k, v in options:
                    st.set_option(k, v)
                row[mode] = time_group(st, stream, repeats, tag, [(mode, lambda: st.apply_compiled(ops))])[mode]
                for k, _ in options:
                    st.set_option(k, 0)
            rows.append(row)
    del amps, keep
    torch.cuda.empty_cache()
    return rows


def fmt(t):
    return f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, nargs="+", default=[30, 26])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dtypes", nargs="+", default=["complex128", "complex64"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qft.md"))
    ap.add_argument("--raw", default=None, help="JSON lines of every timing (default: the page's name with .jsonl)")
    ap.add_argument("--commit", default="(not named)", help="the commit of the tree that ran, for the page")
    args = ap.parse_args()
    if not torch.cuda.is_available() or q.device_count() < 1:
        raise SystemExit("bench_qft needs a HIP device")
    torch.cuda.init()
    lines = [f"# apply_qft beside a gate pass and the lowered circuit through apply_ops, n = {args.n}", "",
             f"`tools/bench_qft.py --n {' '.join(map(str, args.n))} --repeats {args.repeats}` on the tree of {args.commit}: HIP events "
             "around each call on the handle's stream (the call's host work — building and staging its twiddle tables — included), every "
             f"contender warmed up, then {args.repeats} rounds in which the contenders of a group take turns; median (min .. max) in ms, "
             "one process, a dense Gaussian state drawn on the device.  Every shape agreed with the lowered circuit on 4096 random "
             "indices (1e-12 / 1e-5) before timing.  `per pass` = call / (passes x (a)); `best (b) / call` takes the fastest of the three "
             "modes of (b), and LOSES marks a call that is not faster than it.", ""]
    RAW.append({"commit": args.commit})
    for n in args.n:
        for name in args.dtypes:
            dtype = np.complex128 if name == "complex128" else np.complex64
            rows = measure(n, dtype, args.repeats)
            lines += [f"## {name}, n = {n}", "",
                      "| shape | passes | call ms | (a) H gate pass ms | per pass | (b) default apply_ops ms | (b) compiled, IEEE-equal ms | "
                      "(b) compiled, tile_fma + tile_merge ms | best (b) / call | |",
                      "|---|---:|---:|---:|---:|---:|---:|---:|---:|---|"]
            for r in rows:
                best = min([r["default"][0]] + [r[mode][0] for mode, _ in MODES])
                lines.append(f"| {r['label']} ({r['ops']} ops) | {r['passes']} | {fmt(r['call'])} | {fmt(r['floor'])} | "
                             f"{r['call'][0] / (r['passes'] * r['floor'][0]):.2f} | {fmt(r['default'])} | {fmt(r[MODES[0][0]])} | "
                             f"{fmt(r[MODES[1][0]])} | {best / r['call'][0]:.2f} | {'LOSES' if r['call'][0] >= best else ''} |")
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
