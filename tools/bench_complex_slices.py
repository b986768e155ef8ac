#!/usr/bin/env python
"""apply_op / apply_op_overwrite for Complex<f64> / Complex<f32> on device slices (qip_hip_apply_op_device, the call of all of the
reference's benches: qip/benches/state_bench.rs:141-155) at n = 28 (4 GiB in, 4 GiB out for Complex<f64>), and the launch-bound
sizes n = 12 / 20 call by call and as 64 calls inside one hipGraph.  Algorithmic bytes per row: sizeof(P) x (input read + output
write, + output read when accumulating).  HIP events on the stream the kernel is launched on.  The check column compares with
the literal kernel (option force_generic) at n = 28 and with the CPU oracle at n <= 20, bit for bit.

  python tools/bench_complex_slices.py [--no-graph]   (--no-graph: a library whose call synchronises cannot be captured)"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rustqip_amd as q  # noqa: E402
from oracle import qip_oracle as O  # noqa: E402  (the check of the small sizes only)
from rustqip_amd import _ffi  # noqa: E402
from rustqip_amd.ops import MatrixOp  # noqa: E402


def gpu_time(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def bits(t):
    return torch.view_as_real(t).view(torch.int64 if t.dtype == torch.complex128 else torch.int32)


def main():
    graphs = "--no-graph" not in sys.argv
    s2 = float(np.sqrt(0.5))
    h = [s2, s2, s2, -s2]
    rng = np.random.default_rng(3)
    cv = lambda c: rng.standard_normal(c) + 1j * rng.standard_normal(c)  # noqa: E731
    print("| n | P | op | accumulate | GPU us / call | algorithmic GB/s | of 8 TB/s | check |\n|---|---|---|---|---|---|---|---|")
    n = 28
    big = [("H on qubit 0", MatrixOp.new_matrix([0], h)), ("H on qubit 14", MatrixOp.new_matrix([14], h)),
           ("H on qubit n-1", MatrixOp.new_matrix([n - 1], h)),
           ("CNOT(5 -> 20)", MatrixOp.new_control([5], [20], MatrixOp.new_matrix([20], [0, 1, 1, 0]))),
           ("dense on qubits 3, n-2", MatrixOp.new_matrix([3, n - 2], cv(16))),
           ("dense on qubits 2, 9, 17", MatrixOp.new_matrix([2, 9, 17], cv(64))),
           ("controlled (6) dense on qubits 12, 21", MatrixOp.new_control([6], [12, 21], MatrixOp.new_matrix([12, 21], cv(16)))),
           ("Swap(1, n-4)", MatrixOp.new_swap([1], [n - 4]))]
    shapes = [(n, dt, name, op, acc) for dt in (np.complex128, np.complex64) for name, op in big for acc in (True, False)]
    shapes += [(m, dt, "H on qubit 0, ones in (state_bench.rs:141-155)", MatrixOp.new_matrix([0], h), True) for m in (12, 20)
               for dt in (np.complex128, np.complex64)]
    bufs = {}
    for n, dt, name, op, acc in shapes:
        N = 1 << n
        tdt = torch.complex128 if dt == np.complex128 else torch.complex64
        if (n, dt) not in bufs:  # (one input, one output and one comparison buffer per size and type)
            bufs.clear()
            torch.manual_seed(5)
            d_in = torch.ones(N, dtype=tdt, device="cuda") if n <= 20 else torch.randn(N, dtype=tdt, device="cuda")
            bufs[(n, dt)] = (d_in, torch.zeros(N, dtype=tdt, device="cuda"), torch.zeros(N, dtype=tdt, device="cuda") if n > 20 else None)
        d_in, d_out, d_ref = bufs[(n, dt)]
        cop = op.to_c(_ffi.QIP_C64 if dt == np.complex128 else _ffi.QIP_C32)  # (built once, as the reference's benches do)
        d_out.zero_()
        sec = gpu_time(lambda: q.apply_op_device(n, cop, d_in, d_out, accumulate=acc), 200 if n <= 20 else 10)
        by = np.dtype(dt).itemsize * N * (3 if acc else 2)
        graph_us = None
        if n <= 20 and graphs:  # 64 calls recorded into ONE hipGraph (the call is a plain kernel launch on the given stream)
            side = torch.cuda.Stream()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                q.apply_op_device(n, cop, d_in, d_out, accumulate=acc, stream=side.cuda_stream)
                side.synchronize()
                with torch.cuda.graph(g, stream=side):
                    for _ in range(64):
                        q.apply_op_device(n, cop, d_in, d_out, accumulate=acc, stream=side.cuda_stream)
            graph_us = gpu_time(g.replay, 50) / 64 * 1e6
        # check: one more call from a zeroed output
        d_out.zero_()
        q.apply_op_device(n, cop, d_in, d_out, accumulate=acc)
        torch.cuda.synchronize()
        if n <= 20:
            want = np.zeros(N, dtype=dt)
            O.apply_op(n, op, np.ones(N, dtype=dt), want, accumulate=acc)
            ok = np.array_equal(d_out.cpu().numpy().view(np.uint8), want.view(np.uint8))
            against = "the oracle"
        else:
            d_ref.zero_()
            q.set_global_option("force_generic", 1)
            try:
                q.apply_op_device(n, cop, d_in, d_ref, accumulate=acc)
                torch.cuda.synchronize()
            finally:
                q.set_global_option("force_generic", 0)
            ok = bool(torch.equal(bits(d_out), bits(d_ref)))
            against = "the literal kernel"
        note = "" if n > 20 else ("; not captured" if graph_us is None else "; %.2f us / call inside a 64-call hipGraph" % graph_us)
        print(f"| {n} | {np.dtype(dt).name} | {name} | {int(acc)} | {sec*1e6:.1f} | {by/sec/1e9:.0f} | {by/sec/8e12*100:.1f} % | "
              f"{'bit-equal to ' + against if ok else 'DIFFERS from ' + against}{note} |", flush=True)


if __name__ == "__main__":
    main()
