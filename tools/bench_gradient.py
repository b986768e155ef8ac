#!/usr/bin/env python3
"""Time HipState.transition_matrix and HipState.circuit_gradient (include/qip_hipx.h) in one process; prints JSON lines.

(a) One transition pass at n qubits (default 30), Complex<f64> and Complex<f32>, k = 1, 2, 3 on three classes of index positions
    (the lowest k bits — bit 0 is the half of a packed Complex<f32> element —, the top k bits, k scattered bits), on two dense
    random states drawn on the device by torch and wrapped by two handles on one torch stream.  In the same run, as yardsticks:
    a single-term pauli_matrix_elements pass (the same two vectors) and reduced_density_matrix of the same positions (one
    vector).  Every figure is the median of `--repeats` HIP-event timings after one warm-up call.  Before anything is timed,
    tr M is held to inner() and M of (ket, ket) to reduced_density_matrix.
(b) End to end at `--n-e2e` qubits (default 28): a two-layer ry + CNOT-chain ansatz through circuit_gradient against parameter
    shift (two runs of the circuit through apply_ops and an expectation per parameter), and a circuit of Pauli rotations through
    circuit_gradient against the existing adjoint_gradient; wall-clock times of whole calls, with the planned blocks and
    passes and the kernel launches the profile option counts on both handles.

    python tools/bench_gradient.py [--n 30] [--n-e2e 28] [--repeats 7] [--raw profiles/circuit_gradient.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # (before the library: the states are drawn by torch on the device the library then wraps)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rustqip_amd as q  # noqa: E402
from rustqip_amd import parametric as G  # noqa: E402

OUT = []


def emit(**record):
    OUT.append(record)
    print(json.dumps(record), flush=True)


def position_classes(n, k):
    scattered = [b for b in (11, 0, n - 1, 6) if b < n]
    return (("lowest bits", list(range(k))), ("top bits", list(range(n - k, n))), ("scattered", scattered[:k]))


def draw(n, dtype, seed):
    torch.manual_seed(seed)
    amps = torch.randn(1 << n, dtype=torch.complex128 if dtype == np.complex128 else torch.complex64, device="cuda")
    amps /= torch.linalg.vector_norm(amps)
    return amps


def timed(stream, st, fn, repeats):
    fn()
    st.sync()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), times


def passes(n, dtype, repeats):
    name = np.dtype(dtype).name
    a, b = draw(n, dtype, 30), draw(n, dtype, 31)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    nbytes = (1 << n) * (16 if dtype == np.complex128 else 8)
    with q.HipState(n, dtype, wrap_ptr=a.data_ptr(), stream=stream.cuda_stream) as ket, \
            q.HipState(n, dtype, wrap_ptr=b.data_ptr(), stream=stream.cuda_stream) as bra:
        inner = bra.inner(ket)
        base, raw = timed(stream, ket, lambda: bra.pauli_matrix_elements(ket, [{0: "Z"}]), repeats)
        emit(part="a", dtype=name, n=n, call="pauli_matrix_elements, one term", ms=base, raw_ms=raw, tb_per_s=2 * nbytes / base * 1e-9)
        for k in (1, 2, 3):
            for cls, pos in position_classes(n, k):
                indices = [n - 1 - p for p in pos]
                m = bra.transition_matrix(ket, indices)
                assert abs(np.trace(m) - inner) <= 1e-12, (indices, np.trace(m), inner)
                assert np.max(np.abs(ket.transition_matrix(ket, indices) - ket.reduced_density_matrix(indices))) <= 1e-12
                t, raw = timed(stream, ket, lambda: bra.transition_matrix(ket, indices), repeats)
                d, draw_ms = timed(stream, ket, lambda: ket.reduced_density_matrix(indices), repeats)
                emit(part="a", dtype=name, n=n, call="transition_matrix", k=k, positions=cls, pos=pos, ms=t, raw_ms=raw,
                     over_matrix_element_pass=t / base, tb_per_s=2 * nbytes / t * 1e-9, reduced_density_ms=d, reduced_density_raw_ms=draw_ms)
    del a, b
    torch.cuda.empty_cache()


def launches(st):
    return int(sum(v["launches"] for v in st.profile().values()))


def wall(fn, repeats):
    fn()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), times


def end_to_end(n, dtype, repeats):
    name = np.dtype(dtype).name
    rng = np.random.default_rng(5)
    cnot = lambda c, t: q.make_control_op([c], q.make_matrix_op([t], [0, 1, 1, 0]))  # noqa: E731
    circuit = []
    for layer in range(2):
        circuit += [(G.ry(qb), layer * n + qb) for qb in range(n)] + [cnot(qb, qb + 1) for qb in range(n - 1)]
    params = rng.uniform(-1.5, 1.5, 2 * n)
    terms, coeffs = [{0: "Z", 1: "Z"}, {n - 1: "X"}, {n // 2: "Y"}], [0.9, 0.7, -0.4]
    rot_terms = [{0: "X", 1: "Y"}, {2: "Z"}, {n - 1: "Y", 0: "Z", 2: "X"}, {1: "X"}, {n - 1: "Z", 1: "Z"}, {n - 2: "Y"}, {5: "X", 11: "Y"},
                 {3: "X", n - 1: "X"}, {7: "Z", 8: "X", 20: "Y"}, {12: "Y"}, {n // 2: "X", 4: "Z"}, {9: "Z"}]
    angles = rng.uniform(-1.5, 1.5, len(rot_terms))
    rot_circuit = [(G.pauli_rotation(t), i) for i, t in enumerate(rot_terms)]
    with q.HipState(n, dtype) as st, q.HipState(n, dtype) as work:
        def fresh():
            st.init_basis(0)
            st.apply_ops([q.make_matrix_op([qb], [np.sqrt(0.5)] * 3 + [-np.sqrt(0.5)]) for qb in range(n)])

        def shift():
            grad = np.zeros(len(params))
            for p in range(len(params)):
                e = []
                for s in (np.pi / 2, -np.pi / 2):
                    th = params.copy()
                    th[p] += s
                    fresh()
                    st.apply_ops([item if isinstance(item, q.MatrixOp) else item[0].lower(th[item[1]]) for item in circuit])
                    e.append(st.expectation(terms, coeffs))
                grad[p] = (e[0] - e[1]) / 2
            return grad

        def adjoint():
            fresh()
            return st.circuit_gradient(circuit, params, terms, coeffs, work)

        plan = G.gradient_plan(circuit)
        g_shift, (_, g_adj) = shift(), adjoint()
        assert np.max(np.abs(g_shift - g_adj)) <= (1e-10 if dtype == np.complex128 else 1e-3), np.max(np.abs(g_shift - g_adj))
        for s in (st, work):
            s.set_option("profile", 1)
            s.profile_reset()
        before = getattr(work, "transition_passes", 0)
        adjoint()
        counts = {"blocks": len(plan), "planned_passes": sum(len(b["passes"]) for b in plan),
                  "transition_passes": getattr(work, "transition_passes", 0) - before, "launches_state": launches(st), "launches_work": launches(work)}
        for s in (st, work):
            s.set_option("profile", 0)
        t_adj, raw_adj = wall(adjoint, repeats)
        t_shift, raw_shift = wall(shift, max(1, repeats // 3))
        emit(part="b", dtype=name, n=n, circuit="two layers of ry + CNOT chain", parameters=len(params), gates=len(circuit),
             circuit_gradient_ms=t_adj, circuit_gradient_raw_ms=raw_adj, parameter_shift_ms=t_shift, parameter_shift_raw_ms=raw_shift,
             shift_over_adjoint=t_shift / t_adj, max_abs_difference=float(np.max(np.abs(g_shift - g_adj))), **counts)

        def new():
            fresh()
            return st.circuit_gradient(rot_circuit, angles, terms, coeffs, work)

        def old():
            fresh()
            return st.adjoint_gradient(rot_terms, angles, terms, coeffs, work)

        plan = G.gradient_plan(rot_circuit)
        (_, g_new), (_, g_old) = new(), old()
        assert np.max(np.abs(g_new - g_old)) <= (1e-10 if dtype == np.complex128 else 1e-3)
        t_new, raw_new = wall(new, repeats)
        t_old, raw_old = wall(old, repeats)
        emit(part="b", dtype=name, n=n, circuit="12 Pauli rotations", parameters=len(angles), blocks=len(plan),
             planned_passes=sum(len(b["passes"]) for b in plan), circuit_gradient_ms=t_new, circuit_gradient_raw_ms=raw_new,
             adjoint_gradient_ms=t_old, adjoint_gradient_raw_ms=raw_old, old_over_new=t_old / t_new,
             max_abs_difference=float(np.max(np.abs(g_new - g_old))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=30)
    ap.add_argument("--n-e2e", type=int, default=28)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--raw", default=None, help="also write the JSON lines to this file")
    ap.add_argument("--skip", default="", help="'a' or 'b': leave that part out")
    args = ap.parse_args()
    if not torch.cuda.is_available() or q.device_count() < 1:
        raise SystemExit("bench_gradient needs a HIP device")
    torch.cuda.init()
    for dtype in (np.complex128, np.complex64):
        if "a" not in args.skip:
            passes(args.n, dtype, args.repeats)
        if "b" not in args.skip:
            end_to_end(args.n_e2e, dtype, args.repeats)
    if args.raw:
        os.makedirs(os.path.dirname(os.path.abspath(args.raw)), exist_ok=True)
        with open(args.raw, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in OUT)


if __name__ == "__main__":
    main()
