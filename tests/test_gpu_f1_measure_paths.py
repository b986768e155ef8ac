"""SURVEY.md §8 row f1, every kernel path of measurement on a device state (rustqip_amd/csrc/qip_measure.hip and the measurement
block of qip_kernels.h) against the exact reference of tests/measure_ref.py: |amp|^2 formed in the state's precision, summed
in longdouble.  The device accumulates the same products in double, so ONE bar serves Complex<f64> and Complex<f32>:
1e-13 per outcome, 1e-12 on a sum.  The cases and what each is for: tests/measure_ref.py; the reference itself is held to the
oracle on the CPU by tests/test_measure_ref_cpu.py.

  k_measure_probs_small   test_measure_probs_few_qubits (tail only / one round / several rounds, f64 and packed f32),
                          test_large_state (a second round per block)
  k_measure_probs_grid    test_measure_probs_grid_small (k = n < 8, kl = 0, lane bits 6 / 7, b0 + kl = 8),
                          test_measure_probs_grid_step_bits (KI = 1, 2, 3 and their UN = 2 / 1 main loops),
                          test_measure_probs_many_outcomes_f32 (KI = 0 with UN = 4, packed)
  k_measure_probs         test_measure_prob_one_outcome, test_large_state
  k_collapse              test_measure_state_given_probability, test_measure_sampled_f64, test_measure_forced_f32
  k_chunk_norms           test_norm_sqr_of_unnormalised_states, test_large_state (its four-loads-in-flight loop)
  k_find_crossing         test_soft_measure_small_states_f64 / _f32
  the error returns       test_measurement_error_returns"""
from gpu_common import *  # noqa: F401,F403

import measure_ref as R

pytestmark = pytest.mark.gpu

_IDS = ("c128", "c64")
_STATES = {}


def _state(n, dtype):
    """the case state of (n, dtype) — the one tests/test_measure_ref_cpu.py checks the reference on; shared, never written to"""
    key = (n, np.dtype(dtype))
    if key not in _STATES:
        x = R.make_state(n, R.seed_of(n, dtype), dtype)
        x.setflags(write=False)
        _STATES[key] = x
    return _STATES[key]


def _check_probs(st, n, idx, x, norm):
    got, want = st.measure_probs(idx), R.probs_ref(n, idx, x)
    assert got.shape == want.shape
    assert np.max(np.abs(got - want)) <= 1e-13, (n, idx, float(np.max(np.abs(got - want))))
    assert abs(got.sum() - norm) <= 1e-12, (n, idx)


@pytest.mark.parametrize("n", R.SMALL_NS)
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_measure_probs_few_qubits(O, dtype, n):
    """k <= 4: k_measure_probs_small<T, K> and, for Complex<f32> with n >= 2, the packed <float, K, f32x4> with the `bit0` half
    of an element and the `mpos - 1` shift.  Sizes and index sets: measure_ref.SMALL_NS / small_index_sets."""
    x = _state(n, dtype)
    norm = R.norm_ref(x)
    with q.HipState(n, dtype) as st:
        st.upload(x)
        assert abs(st.norm_sqr() - norm) <= 1e-12  # (n < 10: k_chunk_norms on one short chunk)
        sets = R.small_index_sets(n)
        assert {len(s) for s in sets} == set(range(1, min(4, n) + 1))
        for idx in sets:
            _check_probs(st, n, idx, x, norm)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_measure_probs_grid_small(O, dtype):
    """k >= 5 at small sizes, KI = 0: (ki, kg, kl, b0, gx) of every case stands beside it in measure_ref.GRID_SMALL_CASES"""
    for n, pos, _, _ in R.GRID_SMALL_CASES:
        x = _state(n, dtype)
        with q.HipState(n, dtype) as st:
            st.upload(x)
            _check_probs(st, n, R.qubits(n, pos), x, R.norm_ref(x))


@pytest.mark.parametrize("n,dtype", [(20, np.complex128), (21, np.complex128), (22, np.complex128),
                                     (21, np.complex64), (22, np.complex64), (23, np.complex64)],
                         ids=("n20-c128", "n21-c128", "n22-c128", "n21-c64", "n22-c64", "n23-c64"))
def test_measure_probs_grid_step_bits(O, n, dtype):
    """at least 12 measured positions >= 8: the lowest 1, 2, 3 of them are walked per lane (KI), 2^11 outcomes stay on the grid.
    k_measure_probs_grid<double, KI>, <float, KI, f32x4> and <float, KI, f32x4, true>, KI = 1, 2, 3: the instantiations the
    product-state guard of the full-size tests launches.  Cases and their routes: measure_ref.GRID_STEP_CASES."""
    x = _state(n, dtype)
    norm = R.norm_ref(x)
    with q.HipState(n, dtype) as st:
        st.upload(x)
        mine = [pos for cn, cd, pos, _ in R.GRID_STEP_CASES if (cn, cd) == (n, dtype)]
        assert len(mine) >= 2
        for pos in mine:
            _check_probs(st, n, R.qubits(n, pos), x, norm)


def test_measure_probs_many_outcomes_f32(O):
    """the Complex<f32> index sets of test_measure_probs_many_outcomes (k = 5..16, KI = 0, bit 0 as the first / last / a middle
    outcome bit), which the oracle's f32 sums could only hold to 2e-6 * max(1, p * 2^k / 64): the same states at 1e-13"""
    xf = rand_state(12, 2, np.complex64)
    with q.HipState(12, np.complex64) as st:
        st.upload(xf)
        for idx in ([0, 11, 5, 6, 7, 1], list(range(12))):
            _check_probs(st, 12, idx, xf, R.norm_ref(xf))
    n = R.MANY_N
    xf = rand_state(n, 3, np.complex64)
    xf[::5] = 0
    norm = R.norm_ref(xf)
    with q.HipState(n, np.complex64) as st:
        st.upload(xf)
        for idx in R.many_outcome_sets_f32():
            _check_probs(st, n, idx, xf, norm)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_measure_prob_one_outcome(O, dtype):
    """k_measure_probs<T>: several blocks (n = 14, k = 1, 2), a single index (k = n = 13), a quarter of one block (n = 9, k = 3);
    qubit n-1 measured and not"""
    for n, pos, outcomes in R.prob_cases():
        x, idx = _state(n, dtype), R.qubits(n, pos)
        want = R.probs_ref(n, idx, x)
        with q.HipState(n, dtype) as st:
            st.upload(x)
            for m in outcomes:
                assert abs(st.measure_prob(m, idx) - want[m]) <= 1e-13, (n, idx, m)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_norm_sqr_of_unnormalised_states(O, dtype):
    """k_chunk_norms against the exact sum on states whose norm is not 1 (a norm that reads 1 whatever the state holds would
    pass every `norm_sqr() ~ 1` of the suite): one short chunk (n < 10), one, two and 64 chunks of 1024 amplitudes"""
    for n, norm in ((1, 2.5), (2, 0.37), (5, 2.5), (9, 0.37), (10, 2.5), (11, 0.37), (16, 2.5)):
        x = R.make_state(n, 50 + n, dtype, norm=norm)
        want = R.norm_ref(x)
        assert abs(want - norm) < 1e-5
        with q.HipState(n, dtype) as st:
            st.upload(x)
            assert abs(st.norm_sqr() - want) <= 1e-12 * want, (n, norm)


@pytest.mark.parametrize("n,dtype", R.BIG, ids=("n25-c128", "n26-c64"))
def test_large_state(O, n, dtype):
    """512 MiB: the round loop of k_measure_probs_small takes a second iteration per block, k_chunk_norms its unrolled loop,
    k_measure_probs several strides per block.  The state is made on the device — the seeded product state, then a non-unitary
    1-qubit matrix on qubit 0 and on qubit n-1, so the norm is not 1 — and reduced on the host in pieces of 2^22."""
    from oracle import window_parity as W

    sets = R.big_index_sets(n)
    prob_cases = R.big_prob_cases(n)
    with q.HipState(n, dtype) as st:
        st.init_basis(0)
        st.apply_ops(W.product_state_ops(n, 2500 + n)[0])
        for t in (0, n - 1):
            st.apply_op(q.make_matrix_op([t], GATES_1Q["dense"]))
        got_norm = st.norm_sqr()
        got_probs = [st.measure_probs(idx) for idx in sets]
        got_prob = [st.measure_prob(m, idx) for idx, m in prob_cases]
        norm = np.longdouble(0)
        want_probs = [np.zeros(1 << len(idx), dtype=np.longdouble) for idx in sets]
        want_prob = [np.zeros(1 << len(idx), dtype=np.longdouble) for idx, _ in prob_cases]
        for o in range(0, 1 << n, R.PIECE):
            p = R.products(st.download(o, R.PIECE))
            norm += R.norm_partial(p)
            for acc, idx in zip(want_probs + want_prob, sets + [idx for idx, _ in prob_cases]):
                acc += R.probs_partial(n, idx, p, o)
    norm = float(norm)
    assert abs(norm - 1) > 1e-3  # (far from 1 on the scale of the bars: a norm that always reads 1 fails)
    assert abs(got_norm - norm) <= 1e-12 * norm
    assert [len(idx) for idx in sets] == [1, 2, 3, 4]
    for idx, got, want in zip(sets, got_probs, want_probs):
        assert np.max(np.abs(got - want.astype(np.float64))) <= 1e-13, idx
        assert abs(got.sum() - norm) <= 1e-12 * norm, idx
    for (idx, m), got, want in zip(prob_cases, got_prob, want_prob):
        assert abs(got - float(want[m])) <= 1e-13, (idx, m)


def _collapse_cases(n):
    """(positions, outcome, probability handed in): k = 0 is a pure rescale; the rest zero the amplitudes that disagree"""
    if n == 1:
        return (([], 0, 0.37), ([], 0, 2.5), ([0], 1, 1.0), ([0], 0, 0.37))
    if n == 21:  # 8192 blocks' worth of amplitudes on a grid capped at 4096: the grid-stride loop's second trip
        return (([], 0, 0.37), ([0], 1, 1.0), ([20, 0, 9], 5, 2.5))
    return (([], 0, 0.37), ([], 0, 1.0), ([], 0, 2.5), ([0], 1, 2.5), ([n - 1], 0, 0.37), ([1, n - 1, 0], 6, 1.0), (list(range(n)), 5, 0.37))


@pytest.mark.parametrize("n", (1, 3, 10, 21))
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_measure_state_given_probability(O, dtype, n):
    """k_collapse through measure_state(indices, m, p): device and oracle both form 1 / sqrt(p) and two products per amplitude in
    the state's precision (the reference's `P::one() / p.sqrt()`), so the collapsed states are EQUAL"""
    x = _state(n, dtype)
    for pos, m, p in _collapse_cases(n):
        idx = R.qubits(n, pos)
        want = np.zeros_like(x)
        assert O.measure_state(n, idx, (m, p), x, want)
        with q.HipState(n, dtype) as st:
            st.upload(x)
            st.measure_state(idx, m, p)
            got = st.download()
        assert np.array_equal(got, want), (n, idx, m, p, float(np.max(np.abs(got - want))))
    with q.HipState(n, dtype) as st:  # probability zero: the state is left as it is (measurement_ops.rs:230)
        st.upload(x)
        st.measure_state([0], 1, 0.0)
        assert np.array_equal(st.download(), x)


def test_measure_sampled_f64(O):
    """measure with the outcome drawn on the device (`forced < 0`: soft_measure_t -> k_measure_probs -> k_collapse)"""
    n = 13
    x = _state(n, np.complex128)
    rs = [float(v) for v in np.random.default_rng(131).uniform(0, 1, 8)]
    for i, r in enumerate(rs):
        idx = ([1, 5, 10], [12, 0], [7])[i % 3]
        want = np.zeros_like(x)
        wm, wp = O.measure(n, idx, x, want, rand_u01=r)
        with q.HipState(n) as st:
            st.upload(x)
            m, p = st.measure(idx, rand_u01=r)
            assert m == wm and abs(p - wp) <= 1e-13 and abs(p - R.prob_ref(n, m, idx, x)) <= 1e-13, (idx, r)
            assert np.max(np.abs(st.download() - want)) <= 1e-12
            assert abs(st.norm_sqr() - 1) <= 1e-12


def test_measure_forced_f32(O):
    """Complex<f32> k_collapse, p_mult = 1.0f / sqrt((float)p): the collapsed state EQUALS the oracle's measure_state fed the
    probability the device returned"""
    n = 13
    x = _state(n, np.complex64)
    for idx, forced in (([1, 5, 10], 0), ([1, 5, 10], 6), ([12], 1), ([0, 12, 6], 5), (list(range(13)), 4097)):
        with q.HipState(n, np.complex64) as st:
            st.upload(x)
            m, p = st.measure(idx, measured=forced)
            got = st.download()
        assert m == forced and abs(p - R.prob_ref(n, m, idx, x)) <= 1e-13, (idx, forced)
        want = np.zeros_like(x)
        assert O.measure_state(n, idx, (m, p), x, want)
        assert np.array_equal(got, want), (idx, forced)


def test_soft_measure_small_states_f64(O):
    """one chunk shorter than a block's 256 lanes, up to four chunks of 1024 amplitudes: the device's outcome is the oracle's for every sample"""
    for n in R.SOFT_F64_NS:
        x, idx = _state(n, np.complex128), R.soft_index_set(n)
        rs = R.soft_samples(n) + list(R.SOFT_EDGES)
        with q.HipState(n) as st:
            st.upload(x)
            got = [st.soft_measure(idx, r) for r in rs]
        want = [O.soft_measure(n, idx, x, r) for r in rs]
        assert got == want, (n, [(r, a, b) for r, a, b in zip(rs, got, want) if a != b][:5])


def test_soft_measure_small_states_f32(O):
    """Complex<f32>: the oracle's own f32 scan drifts, so the expected index is the exact crossing (crossing_ref) of the sample
    as rounded to f32; a sample within SOFT_MARGIN of a partial sum has no defined outcome and is left out — at most 1 % of a
    case's samples may be, and the seeds are chosen so that none is"""
    for n in R.SOFT_F32_NS:
        x, idx = _state(n, np.complex64), R.soft_index_set(n)
        rs = R.soft_samples(R.SOFT_SAMPLE_SEED[n]) + [1.5]
        ref = [R.crossing_ref(x, float(np.float32(r))) for r in rs]
        keep = [i for i, (_, dist) in enumerate(ref) if dist >= R.SOFT_MARGIN]
        assert len(rs) - len(keep) <= len(rs) // 100
        with q.HipState(n, np.complex64) as st:
            st.upload(x)
            got = [st.soft_measure(idx, rs[i]) for i in keep]
        want = [R.outcome_of(n, idx, ref[i][0]) for i in keep]
        assert got == want, (n, [(rs[i], a, b) for i, a, b in zip(keep, got, want) if a != b][:5])


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_measurement_error_returns(O, dtype):
    """every refusal of the measurement entry points is QIP_ERR_INVALID (CircuitError) and leaves the state usable and unchanged"""
    n = 5
    x = _state(n, dtype)
    with q.HipState(n, dtype) as st:
        st.upload(x)

        def refused(call, *args, **kw):
            with pytest.raises(q.CircuitError):
                call(*args, **kw)
            assert np.array_equal(st.download(), x)

        bad_lists = ([1, 3, 1], [0, n], [], list(range(n + 1)))  # repeated, index = n, k = 0, k = n + 1
        for bad in bad_lists:
            refused(st.measure_probs, bad)
            refused(st.measure_prob, 0, bad)
            refused(st.soft_measure, bad, 0.5)
            refused(st.measure, bad, measured=0)
            refused(st.measure, bad, rand_u01=0.5)
            if bad:  # (k = 0 is measure_state's pure rescale)
                refused(st.measure_state, bad, 0, 0.5)
        refused(st.measure_prob, 4, [0, 3])            # an outcome of more than k bits
        refused(st.measure, [0, 3], measured=4)
        refused(st.measure_state, [0, 3], 4, 0.5)
        refused(st.measure_state, [], 1, 0.5)
        refused(st.measure_state, [2], 1, -1.0)        # a negative probability
        refused(st.measure_state, [2], 1, float("nan"))
        # and it still measures
        assert np.max(np.abs(st.measure_probs([0, 3]) - R.probs_ref(n, [0, 3], x))) <= 1e-13
