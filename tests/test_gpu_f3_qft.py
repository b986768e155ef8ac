"""The quantum Fourier transform of a register on the device (include/qip_hipx.h: qipx_state_apply_qft; HipState.apply_qft,
rustqip_amd.fourier): k_qft_tile (rustqip_amd/csrc/qip_qft_kernels.h) on every n up to 13, every placement of the register
relative to the wave row at n = 14, every pass boundary at the smallest n that shows it, both precisions and all four flag
combinations.  Every case is held per fibre to |got - exact|_2 <= 8 m u |old|_2 against tests/qft_ref.py (a long-double FFT; the
bar is derived there) and the worst ratio of each test is printed.  A block owns exactly one tile, so no case walks several."""
import ctypes as C

from gpu_common import *  # noqa: F401,F403

import qft_ref as R
from rustqip_amd import _ffi, classical, fourier

pytestmark = pytest.mark.gpu

_IDS = ("c128", "c64")


def _run(st, n, x, qubits, exact, dtype, flags=R.FLAGS):
    """the worst ratio to the bar's unit m u |fibre| over the flag combinations, each applied to a fresh upload of x"""
    worst = 0.0
    for inverse, reversed in flags:
        st.upload(x)
        st.apply_qft(qubits, inverse=inverse, reversed=reversed)
        got = st.download()
        ratio = R.worst_ratio(n, got, exact[(inverse, reversed)], x, qubits, dtype)
        assert ratio <= R.BAR, (n, qubits, inverse, reversed, np.dtype(dtype).name, ratio)
        worst = max(worst, ratio)
    return worst


def _sweep(cases, dtype, seed):
    worst, count, states = 0.0, 0, {}
    try:
        for n, qubits in cases:
            if n not in states:
                states[n] = q.HipState(n, dtype)
            x = R.make_state(n, seed + 31 * n + len(qubits), dtype)
            worst = max(worst, _run(states[n], n, x, qubits, R.qft_exact_all(n, x, qubits), dtype))
            count += len(R.FLAGS)
    finally:
        for st in states.values():
            st.close()
    return worst, count


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_small_n_every_placement_of_short_registers(dtype):
    cases = R.small_cases()
    assert {n for n, _ in cases} == set(range(1, 14)) and all(1 <= len(qs) <= 4 for _, qs in cases)
    assert len(cases) >= 300  # (n, register) pairs; each runs all four flag combinations
    worst, count = _sweep(cases, dtype, 100)
    assert count == 4 * len(cases)
    print(f"small n, {np.dtype(dtype).name}: {count} cases, worst |error| = {worst:.3f} m u |fibre|")


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_placement_matrix_at_n_14(dtype):
    worst, count = _sweep(R.placement_cases(), dtype, 200)
    print(f"placements at n = 14, {np.dtype(dtype).name}: {count} cases, worst |error| = {worst:.3f} m u |fibre|")


@pytest.mark.parametrize("case", range(len(R.boundary_cases())))
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_pass_boundaries(dtype, case):
    n, qubits, natural, reversed = R.boundary_cases()[case]
    x = R.make_state(n, 300 + case, dtype)
    with q.HipState(n, dtype) as st:
        assert st.qft_passes(qubits) == natural and st.qft_passes(qubits, inverse=True) == natural
        assert st.qft_passes(qubits, reversed=True) == reversed and st.qft_passes(qubits, inverse=True, reversed=True) == reversed
        worst = _run(st, n, x, qubits, R.qft_exact_all(n, x, qubits), dtype)
    print(f"n = {n}, m = {len(qubits)}, {natural} / {reversed} passes, {np.dtype(dtype).name}: worst |error| = {worst:.3f} m u |fibre|")


@pytest.mark.parametrize("n,qubits", R.ZERO_FIBRE_CASES)
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_zero_fibres_stay_zero(dtype, n, qubits):
    idx = R.fibre_index(n, qubits)
    fibre = idx.shape[0] // 3
    x = np.zeros(2 ** n, dtype=dtype)
    x[idx[fibre]] = R.make_state(len(qubits), 41, dtype)
    exact = R.qft_exact_all(n, x, qubits)
    others = np.delete(idx, fibre, axis=0).ravel()
    with q.HipState(n, dtype) as st:
        for inverse, reversed in R.FLAGS:
            st.upload(x)
            st.apply_qft(qubits, inverse=inverse, reversed=reversed)
            got = st.download()
            assert np.all(got[others] == 0), (inverse, reversed)  # (zeros of either sign)
            ratio = R.worst_ratio(n, got, exact[(inverse, reversed)], x, qubits, dtype)
            assert 0 < ratio <= R.BAR, ratio
            print(f"one fibre of n = {n}, {np.dtype(dtype).name}, inverse={inverse} reversed={reversed}: {ratio:.3f} m u |fibre|")


@pytest.mark.parametrize("n,qubits", R.ROUND_TRIP_CASES)
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_inverse_and_reversal(dtype, n, qubits):
    m, positions = len(qubits), [n - 1 - qb for qb in qubits]
    x = R.make_state(n, 51, dtype)
    exact = R.qft_exact_all(n, x, qubits)
    with q.HipState(n, dtype) as st:
        for reversed in (False, True):  # flags 0 then INVERSE; REVERSED then REVERSED | INVERSE
            st.upload(x)
            st.apply_qft(qubits, reversed=reversed)
            st.apply_qft(qubits, inverse=True, reversed=reversed)
            back = st.download()
            ratio = R.worst_ratio(n, back, x.astype(R.wide_type(dtype)), x, qubits, dtype)
            print(f"round trip n = {n}, m = {m}, reversed={reversed}, {np.dtype(dtype).name}: {ratio:.3f} m u |fibre|")
            assert ratio <= R.ROUND_TRIP_BAR, (reversed, ratio)
        # the reversed output, its register's bits reversed by permute_bits, is the natural output
        pi = list(range(n))
        for i, p in enumerate(positions):
            pi[p] = positions[m - 1 - i]
        st.upload(x)
        st.apply_qft(qubits, reversed=True)
        st.permute_bits(pi)
        ratio = R.worst_ratio(n, st.download(), exact[(False, False)], x, qubits, dtype)
        assert ratio <= R.BAR, ratio


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_the_call_and_the_lowered_circuit_each_meet_their_bar(dtype):
    """n = 12, nine qubits, scrambled: apply_qft to 8 m u per fibre, apply_ops(fourier.qft_ops(..)) to the gate path's bar of
    tests/gpu_common.py (1e-12 / 1e-5 per amplitude of a normalised state)"""
    n, qubits = 12, R.TIE_REGISTER
    x = rand_state(n, 61, dtype)
    exact = R.qft_exact_all(n, x, qubits)
    tol = TOL64 if dtype == np.complex128 else TOL32
    with q.HipState(n, dtype) as st:
        worst = _run(st, n, x, qubits, exact, dtype)
        for inverse, reversed in R.FLAGS:
            st.upload(x)
            st.apply_ops(fourier.qft_ops(qubits, inverse=inverse, reversed=reversed))
            err = float(np.max(np.abs(st.download() - exact[(inverse, reversed)])))
            assert err <= tol, (inverse, reversed, err)
    print(f"tie at n = 12, {np.dtype(dtype).name}: apply_qft worst |error| = {worst:.3f} m u |fibre|")


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_order_finding_of_7_modulo_15(dtype):
    n, counting, work = R.ORDER_FINDING
    tol = 1e-12 if dtype == np.complex128 else 1e-5
    want = np.zeros(256)
    want[[0, 64, 128, 192]] = 0.25
    with q.HipState(n, dtype) as st:
        st.init_basis(0)
        fourier.order_finding(st, counting, work, 7, 15)
        probs = st.measure_probs(counting)
        assert np.max(np.abs(probs - want)) <= tol, np.max(np.abs(probs - want))
        # the same through the readout: Hadamards and the table, then the inverse transform and samples in one call
        st.init_basis(0)
        st.apply_ops([q.make_matrix_op([qb], circuits.H) for qb in counting])
        classical.exp_mod_into(st, counting, work, 7, 15)
        shots = fourier.phase_estimation_readout(st, counting, 2000, seed=5)
        assert set(int(v) for v in shots) == {0, 64, 128, 192}
        # ... and with the phases left in reversed order by a reversed forward transform of the readout's result
        fourier.qft(st, counting, reversed=True)
        shots = fourier.phase_estimation_readout(st, counting, 500, seed=6, reversed=True)
        assert set(int(v) for v in shots) <= {0, 64, 128, 192}


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_an_empty_register_does_nothing(dtype):
    n = R.EMPTY_CASE[0]
    x = R.make_state(n, 71, dtype)
    with q.HipState(n, dtype) as st:
        st.upload(x)
        for inverse, reversed in R.FLAGS:
            st.apply_qft([], inverse=inverse, reversed=reversed)
            assert st.qft_passes([], inverse=inverse, reversed=reversed) == 0
        assert np.array_equal(st.download().view(np.uint8), x.view(np.uint8))


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_the_same_call_gives_the_same_bits(dtype):
    n, qubits = 13, R.qubits_at(13, [6, 0, 3, 7, 8, 9, 10, 11, 12, 5])
    x = R.make_state(n, 81, dtype)
    with q.HipState(n, dtype) as st, q.HipState(n, dtype) as other:
        for inverse, reversed in R.FLAGS:
            runs = []
            for handle in (st, st, other):
                handle.upload(x)
                handle.apply_qft(qubits, inverse=inverse, reversed=reversed)
                runs.append(handle.download())
            assert np.array_equal(runs[0].view(np.uint8), runs[1].view(np.uint8))
            assert np.array_equal(runs[0].view(np.uint8), runs[2].view(np.uint8))
            assert not np.array_equal(runs[0], x)


def _raw(st, qubits, count, flags):
    arr = None if qubits is None else (C.c_uint64 * max(1, len(qubits)))(*qubits)
    return _ffi.lib.qipx_state_apply_qft(st._h if st is not None else None, arr, count, flags), _ffi.last_error()


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_refusals_leave_the_state_untouched(dtype):
    n = 10
    x = R.make_state(n, 91, dtype)
    with q.HipState(n, dtype) as st:
        st.upload(x)
        for qubits, count, flags, message in (
                (None, 2, 0, "null qubit array"),
                ([1, 10], 2, 0, "qubit 10 out of range"),
                ([1, 2 ** 40], 2, 1, "out of range"),
                ([3, 4, 3], 3, 2, "qubit 3 repeated"),
                ([3, 4], 2, 4, "unknown flag bits"),
                ([3, 4], 2, 0xFFFFFFFC, "unknown flag bits"),
        ):
            rc, err = _raw(st, qubits, count, flags)
            assert rc == _ffi.QIP_ERR_INVALID and message in err and err.startswith("apply_qft:"), (message, rc, err)
            assert np.array_equal(st.download().view(np.uint8), x.view(np.uint8)), message
        rc, err = _raw(None, [1], 1, 0)
        assert rc == _ffi.QIP_ERR_INVALID and "null state handle" in err
        with pytest.raises(q.CircuitError, match="repeated"):
            st.apply_qft([5, 5])
        assert np.array_equal(st.download().view(np.uint8), x.view(np.uint8))
