#!/usr/bin/env python3
"""Time HipState.soft_measure_many (include/qip_hipx.h) beside a loop of single soft_measure calls, in one process.

For Complex<f64> and Complex<f32> at n qubits (default 30), on a dense random state (Gaussian amplitudes drawn on the device by
torch, normalised, wrapped by the handle) and on a peaked one (init_basis(0), then H on three qubits: eight amplitudes, every
sample lands in a few chunks), the batch is timed for count in {1, 256, 65 536, 2^20} and
a loop of 64 single calls next to each, the two alternating.  Every timed call ends in a synchronise of its own (both return
results to the host), so a host clock around it is the time; medians over `--repeats` after one warm-up round.  Before any time
is reported the batch is held to the single calls on those 64 samples.  Writes a markdown table (default
profiles/sample_many.md) and prints it.

    python tools/bench_sample.py [--n 30] [--repeats 7] [--out profiles/sample_many.md]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch  # (before the library: the dense state is drawn by torch on the device the library then wraps)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rustqip_amd as q  # noqa: E402
from rustqip_amd import circuits  # noqa: E402

COUNTS = (1, 256, 65536, 1 << 20)
SINGLES = 64


def make_state(n, dtype, kind):
    """(handle, what keeps its memory alive)"""
    if kind == "peaked":
        st = q.HipState(n, dtype)
        st.init_basis(0)
        st.apply_ops([q.make_matrix_op([t], circuits.H) for t in (0, n // 2, n - 1)])
        st.sync()
        return st, None
    torch.manual_seed(30)
    amps = torch.randn(1 << n, dtype=torch.complex128 if dtype == np.complex128 else torch.complex64, device="cuda")
    amps /= torch.linalg.vector_norm(amps)
    torch.cuda.synchronize()
    return q.HipState(n, dtype, wrap_ptr=amps.data_ptr()), amps


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def measure(n, dtype, kind, repeats):
    idx = sorted({0, n // 2, n - 1}, reverse=True)
    rng = np.random.default_rng(2030)
    rows = []
    st, keep = make_state(n, dtype, kind)
    with st:
        singles_rs = rng.uniform(0, 1, SINGLES)
        want = np.array([st.soft_measure(idx, float(r)) for r in singles_rs], dtype=np.uint64)
        got = st.soft_measure_many(idx, singles_rs)
        assert np.array_equal(got, want), "soft_measure_many differs from the single calls"
        for count in COUNTS:
            rs = rng.uniform(0, 1, count)
            rs[:min(count, SINGLES)] = singles_rs[:min(count, SINGLES)]
            assert np.array_equal(st.soft_measure_many(idx, rs)[:SINGLES], want[:count])  # (also the warm-up: scratch grown)
            batch, single = [], []
            for _ in range(repeats):
                batch.append(timed(lambda: st.soft_measure_many(idx, rs)))
                single.append(timed(lambda: [st.soft_measure(idx, float(r)) for r in singles_rs]) / SINGLES)
            b, s = statistics.median(batch), statistics.median(single)
            rows.append((kind, np.dtype(dtype).name, count, b, s, b / s))
    del keep
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_many.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available() or q.device_count() < 1:
        raise SystemExit("bench_sample needs a HIP device")
    torch.cuda.init()
    rows = []
    for dtype in (np.complex128, np.complex64):
        for kind in ("dense", "peaked"):
            rows += measure(args.n, dtype, kind, args.repeats)
    lines = [f"# soft_measure_many beside single soft_measure calls, n = {args.n}", "",
             f"`tools/bench_sample.py --n {args.n} --repeats {args.repeats}`: host clock around calls that end in a synchronise, medians of "
             f"{args.repeats} after a warm-up, the batch and a loop of {SINGLES} single calls alternating in one process; the batch "
             "equalled the single calls on those samples before anything was timed.", "",
             "| state | dtype | samples | batch ms | one single call ms | batch / single | per sample, batch |",
             "|---|---|---:|---:|---:|---:|---:|"]
    for kind, dt, count, b, s, ratio in rows:
        lines.append(f"| {kind} | {dt} | {count} | {b:.3f} | {s:.3f} | {ratio:.2f} | {b / count * 1e3:.3f} us |")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
