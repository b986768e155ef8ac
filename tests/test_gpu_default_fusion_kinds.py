"""Option pair_floor on the default path (tile = 0, pair_floor = 1, n >= 22) with every tile item kind: fuzzed batches of
exact and rounded gates, with and without controls, on the bits where tile addressing changes, must give one launch per
gate's bits (pair_floor = 0) and the oracle's.  And an op that, launched alone, runs on matrix cores (launch_kq's fma chains
and three-product forms) must neither ride in a fused sweep as the register fold nor have exact gates moved past it.  Generators: tests/fuzz_ops.py; the host
premises of these batches are checked without a GPU in tests/test_tile_plan_cpu.py."""
from gpu_common import *  # noqa: F401,F403

from fuzz_ops import (DENSE3_CASES, FUZZ_SEEDS, SINGLE_VIA_TILE_DEFAULT, dense3_case, dense3_in_a_multi_gate_step, fused_coverage,
                      fuzz_default_batch, seeded_default_batch, unit_phase_case)
from oracle import window_parity as W
from rustqip_amd import _ffi
from rustqip_amd.ops import plan_tiles

pytestmark = pytest.mark.gpu

def _dt(dtype):
    return _ffi.QIP_C64 if dtype == np.complex128 else _ffi.QIP_C32


def _launches(prof, noop=True):
    return sum(v["launches"] for k, v in prof.items() if k != "tile_sweep_parts" and (noop or k != "noop_identity"))


def _run(n, x, ops, pair_floor, one_by_one=False):
    """ops applied to a fresh state holding x: (the whole vector, the profile)"""
    with q.HipState(n, x.dtype) as st:
        st.set_option("pair_floor", pair_floor)
        st.upload(x)
        st.set_option("profile", 1)
        st.profile_reset()
        if one_by_one:
            for op in ops:
                st.apply_op(op)
        else:
            st.apply_ops(ops)
        prof = st.profile()
        return st.download(), prof


def _why(a, b):
    bad = np.flatnonzero(a != b)
    return f"{bad.size} amplitudes differ, first at index {bad[0]}, max|d| = {np.max(np.abs(a - b)):.3e}" if bad.size else "equal"


# ---- 1. fuzzed default-path batches -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [22, 23])
def test_fuzzed_batches_of_every_kind_are_bit_equal_to_gate_by_gate_and_match_the_oracle(O, n):
    covered = {np.complex128: (set(), set()), np.complex64: (set(), set())}
    for seed in FUZZ_SEEDS:
        mixed = seed == 2  # dense 3-qubit gates with two or three targets below bit 6, dense 4-qubit breakers
        ops, tags = seeded_default_batch(n, seed)
        x32 = rand_state(n, 50 + seed, np.complex64)
        want = O.apply_ops_in_place(n, ops, x32.astype(np.complex128))  # both dtypes start from the same amplitudes
        for dtype in (np.complex128, np.complex64):
            x = x32.astype(dtype)
            fused, pf = _run(n, x, ops, 1)
            gbg, pg = _run(n, x, ops, 0)
            where = f"n={n} seed={seed} {np.dtype(dtype).name}"
            assert np.array_equal(fused, gbg), f"{where}: pair_floor 1 vs 0: {_why(fused, gbg)}"
            assert _launches(pf) < _launches(pg), (where, pf, pg)  # the default path really fused
            if dtype == np.complex128 and not mixed:  # every op launched alone is the oracle's fold: bit for bit
                assert np.array_equal(fused, want), f"{where}: oracle: {_why(fused, want)}"
            else:
                d = float(np.max(np.abs(fused - want)))
                assert d <= (TOL64 if dtype == np.complex128 else TOL32), (where, d)
            if not mixed:
                kinds, at = fused_coverage(plan_tiles(n, ops, 1, _dt(dtype)), tags)
                covered[dtype][0].update(kinds)
                covered[dtype][1].update(at)
    for dtype, (kinds, at) in covered.items():  # Complex<f64>: tile_p5 = 11 (bit 5 is a high tile bit); Complex<f32>: 5
        assert {(k, c) for k in range(5) for c in (False, True)} <= kinds, (dtype, sorted(kinds))  # (same premise on the CPU)
        assert {(k, b) for k in range(5) for b in (5, 11, 12)} <= at, (dtype, sorted(at))


# ---- 2. dense 3-qubit gates that run on matrix cores when launched alone ------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.complex128, np.complex64], ids=["c64", "c32"])
@pytest.mark.parametrize("name,n", DENSE3_CASES)
def test_dense3_on_matrix_cores_alone_is_not_fused(name, n, dtype):
    ops, i3, svt, mfma_alone = dense3_case(name, n, np.random.default_rng(7))
    plan = plan_tiles(n, ops, 1, _dt(dtype))
    assert len(plan) == 1 and dense3_in_a_multi_gate_step(plan, i3), plan  # premise: mode 1 puts it in ONE multi-gate step
    x = rand_state(n, 9, dtype)
    try:
        q.set_global_option("single_via_tile", svt)
        fused, pf = _run(n, x, ops, 1)
        gbg, pg = _run(n, x, ops, 0)
        alone, pa = _run(n, x, ops, 1, one_by_one=True)
        _, p3 = _run(n, x, ops[i3:i3 + 1], 1, one_by_one=True)
    finally:
        q.set_global_option("single_via_tile", SINGLE_VIA_TILE_DEFAULT)
    # premise: launched alone, the dense gate runs on matrix cores (or, five controls at n = 22, as a one-op tile sweep)
    assert ("k_gate_kq_mfma" in p3) == mfma_alone and ("k_tile_passes" in p3) == (not mfma_alone), p3
    assert np.array_equal(fused, gbg), f"pair_floor 1 vs 0: {_why(fused, gbg)}"
    assert np.array_equal(fused, alone), f"apply_ops vs apply_op one at a time: {_why(fused, alone)}"
    assert _launches(pg) == _launches(pa) == len(ops)
    if mfma_alone:
        # the dense gate runs on its own kernel; H neighbours in front of it still share one sweep where there are two
        assert _launches(pf) == (len(ops) - 1 if i3 == 2 else len(ops)), pf
        assert pf.get("k_gate_kq_mfma", {}).get("launches", 0) == 1, pf
    else:
        assert _launches(pf) == 1 and pf["k_tile_passes"]["launches"] == 1, pf  # the whole batch: ONE sweep


@pytest.mark.parametrize("dtype", [np.complex128, np.complex64], ids=["c64", "c32"])
def test_no_gate_is_moved_past_a_gate_on_matrix_cores(dtype):
    n = 22
    ops, i4 = unit_phase_case(n, np.random.default_rng(3))
    plan = plan_tiles(n, ops, 1, _dt(dtype))
    assert plan == [[0, 1, 3, 4], [i4]], plan  # premise: mode 1 moves S and Y past the dense gate
    x = rand_state(n, 10, dtype)
    fused, pf = _run(n, x, ops, 1)
    gbg, pg = _run(n, x, ops, 0)
    assert np.array_equal(fused, gbg), f"pair_floor 1 vs 0: {_why(fused, gbg)}"
    assert pg.get("k_gate_kq_mfma", {}).get("launches", 0) == 1, pg  # (alone: matrix cores)
    # H H | dense | S Y: the gates on either side still share a sweep each
    assert _launches(pf) == 3 and pf.get("k_tile_passes", {}).get("launches", 0) == 2, pf


# ---- 3. the n = 21 / 22 threshold -------------------------------------------------------------------------------------------

def test_fusion_starts_at_22_qubits():
    for n in (21, 22):
        ops, tags = fuzz_default_batch(n, np.random.default_rng(77), 120)
        x = rand_state(n, 78)
        fused, pf = _run(n, x, ops, 1)
        gbg, pg = _run(n, x, ops, 0)
        assert np.array_equal(fused, gbg), f"n={n}: {_why(fused, gbg)}"
        real = sum(1 for t in tags if t[0] != "noop")
        assert _launches(pg, noop=False) == real
        if n == 21:
            assert _launches(pf, noop=False) == real, pf  # one launch per gate that does something
        else:
            assert _launches(pf, noop=False) < real and pf.get("k_tile_passes", {}).get("launches", 0) >= 4, pf


# ---- 4. full size, against the oracle on closed sub-cubes -------------------------------------------------------------------

def test_fuzzed_batch_at_30_qubits_matches_the_oracle_on_closed_sub_cubes(O):
    n = 30
    ops, _ = fuzz_default_batch(n, np.random.default_rng(30), 96)
    with q.HipState(n, np.complex128) as st:
        st.init_basis(0)
        st.apply_ops(W.product_state_ops(n, seed=n)[0])
        st.set_option("profile", 1)
        st.profile_reset()
        agg = W.check_circuit(st, n, ops, O, gate_by_gate=False, seed=3, bases_per_step=2)
        prof = st.profile()
    assert agg["gates"] == len(ops) and agg["skipped"] == 0, agg
    assert agg["max_abs_delta"] == 0.0, agg  # the register fold only: only a -0 may differ
    assert prof.get("k_tile_passes", {}).get("launches", 0) >= 2, prof  # the default path really fused
