"""The exact measurement reference of tests/measure_ref.py against the oracle, where the oracle is itself exact enough: every
Complex<f64> case the GPU measurement tests run at n <= 22 (the oracle's sequential f64 sum is within 1.7e-14 of the exact sum
there), and Complex<f32> at k = n, where every outcome is a single product.  No GPU."""
import numpy as np
import pytest

import measure_ref as R

_STATES = {}


def _state(n, dtype=np.complex128):
    key = (n, np.dtype(dtype))
    if key not in _STATES:
        _STATES[key] = R.make_state(n, R.seed_of(n, dtype), dtype)
    return _STATES[key]


def _f64_probs_cases():
    for n in R.SMALL_NS:
        for idx in R.small_index_sets(n):
            yield n, idx
    for n, pos, _, _ in R.GRID_SMALL_CASES:
        yield n, R.qubits(n, pos)
    for n, dtype, pos, _ in R.GRID_STEP_CASES:
        if dtype == np.complex128:
            yield n, R.qubits(n, pos)


def test_probs_ref_vs_oracle_f64(O):
    count = 0
    for n, idx in _f64_probs_cases():
        x = _state(n)
        got, want = R.probs_ref(n, idx, x), O.measure_probs(n, idx, x)
        assert got.shape == want.shape and got.dtype == np.float64
        assert np.max(np.abs(got - want)) <= 1e-13, (n, idx)
        count += 1
    assert count > 150


def test_prob_ref_and_norm_ref_vs_oracle_f64(O):
    for n, pos, outcomes in R.prob_cases():
        x, idx = _state(n), R.qubits(n, pos)
        for m in outcomes:
            assert abs(R.prob_ref(n, m, idx, x) - O.measure_prob(n, m, idx, x)) <= 1e-13, (n, idx, m)
    for n in sorted({n for n, _ in _f64_probs_cases()}):
        x = _state(n)
        assert abs(R.norm_ref(x) - O.prob_magnitude(x)) <= 1e-12, n
        y = R.make_state(n, 7, norm=2.5)
        assert abs(R.norm_ref(y) - O.prob_magnitude(y)) <= 1e-12, n


def test_probs_ref_f32_equals_oracle_at_k_equal_n(O):
    """k = n: an outcome is one product re*re + im*im formed in f32 — nothing is summed, so the two must be EQUAL"""
    for n in (1, 2, 3, 5, 8, 9, 13):
        x = _state(n, np.complex64)
        for pos in (list(range(n)), list(range(n))[::-1], [int(v) for v in np.random.default_rng(n).permutation(n)]):
            idx = R.qubits(n, pos)
            got, want = R.probs_ref(n, idx, x), O.measure_probs(n, idx, x)
            assert want.dtype == np.float32 and np.array_equal(got, want.astype(np.float64)), (n, idx)
            for m in (0, (1 << n) - 1, (1 << n) // 3):
                assert R.prob_ref(n, m, idx, x) == float(O.measure_prob(n, m, idx, x))


def test_probs_ref_piecewise_and_windows():
    """pieces of any power-of-two size give the same sums (to the last longdouble rounding), and a window adds only its own
    amplitudes"""
    n = 12
    for dtype in R.DTYPES:
        x = _state(n, dtype)
        p = R.products(x)
        for idx in R.small_index_sets(n)[::3] + [R.qubits(n, [8, 0, 3, 5, 6, 11])]:
            whole = R.probs_partial(n, idx, p)
            for low in (0, 3, 9):
                acc = np.zeros_like(whole)
                for o in range(0 if low else 3 << 9, 1 << n if low else 4 << 9, 1 << low):  # (single amplitudes: one stretch)
                    acc += R.probs_partial(n, idx, p[o:o + (1 << low)], o)
                if not low:
                    acc += R.probs_partial(n, idx, p[:1 << 9], 0) + R.probs_partial(n, idx, p[1 << 9:1 << 10], 1 << 9)
                    acc += R.probs_partial(n, idx, p[1 << 10:3 << 9], 1 << 10) + R.probs_partial(n, idx, p[1 << 11:], 1 << 11)
                assert np.max(np.abs(acc - whole)) <= 1e-18, (idx, low)
            half = R.probs_ref(n, idx, x, 1 << (n - 1), 1 << (n - 1)) + R.probs_ref(n, idx, x, 0, 1 << (n - 1))
            assert np.max(np.abs(half - R.probs_ref(n, idx, x))) <= 1e-16
        brute = np.zeros(8)
        idx = R.qubits(n, [0, 9, 4])
        for i in range(1 << n):
            brute[R.outcome_of(n, idx, i)] += float(p[i])
        assert np.max(np.abs(brute - R.probs_ref(n, idx, x))) <= 1e-14


def test_grid_cases_declare_their_route():
    """the (ki, kg, kl, b0, gx) written beside every k >= 5 case is what the restated routing gives"""
    for n, pos, f64, f32 in R.GRID_SMALL_CASES:
        assert (R.grid_route(n, pos, False), R.grid_route(n, pos, True)) == (f64, f32), (n, pos)
    for n, dtype, pos, route in R.GRID_STEP_CASES:
        assert R.grid_route(n, pos, dtype == np.complex64) == route, (n, pos)
    kinds = {(dtype == np.complex64, r[0], r[3] >= 0) for _, dtype, _, r in R.GRID_STEP_CASES}
    assert kinds == {(False, 1, False), (False, 2, False), (False, 3, False)} | {(True, ki, b) for ki in (1, 2, 3) for b in (False, True)}


def test_crossing_ref_and_f32_sample_seeds(O):
    x = np.array([0, 0.5, 0, 0.5j, 0.5, -0.5], dtype=np.complex128)
    assert R.crossing_ref(x, 0.0) == (0, 0.0)
    assert R.crossing_ref(x, 0.25)[0] == 1 and R.crossing_ref(x, 0.2500001)[0] == 3
    assert R.crossing_ref(x, 1.5) == (0, 0.5)
    # f64: the oracle's sequential scan crosses where the exact one does unless the sample is within its rounding of a boundary
    for n in R.SOFT_F64_NS:
        xs, idx = _state(n), R.soft_index_set(n)
        for r in R.soft_samples(n):
            at, dist = R.crossing_ref(xs, r)
            assert dist < 1e-13 or R.outcome_of(n, idx, at) == O.soft_measure(n, idx, xs, r)
    # f32: the seeds leave no sample within SOFT_MARGIN of a partial sum
    for n in R.SOFT_F32_NS:
        xs = _state(n, np.complex64)
        for r in R.soft_samples(R.SOFT_SAMPLE_SEED[n]):
            assert R.crossing_ref(xs, float(np.float32(r)))[1] >= R.SOFT_MARGIN, (n, r)
