"""The extended calls (include/qip_hipx.h and the measurement calls) on handles that wrap caller memory and caller streams.

Handle forms (tests/wrapped_common.py): one-handle families run on `owned`, W1 and W2; two-handle families run the pairs
W1 + W1 (two torch streams, as tools/bench_adjoint.py), W1 + owned and W1 + W2 beside an owned + owned twin.  Every family runs
at n = 15 and at the smallest n it accepts with index bit 0 (qubit n - 1) among its qubits, in Complex<f64> and Complex<f32>.

Every family is held
  * to the reference and the bar of its own tests/*_ref.py module, applied to the owned twin's results (the docstrings name them);
  * bit for bit — the state(s) and every returned value — to the owned twin that ran the same calls: no route of these calls
    depends on who owns the buffers or the stream, so none is exempt;
  * to intact guard zones and the buffer contract (device_ptr() names the buffer download() reads) after the calls.
In the two-handle families one handle has work queued on ITS stream, with no synchronisation, when the other handle's call reads
it: the twin records the intermediate vectors for the references, the wrapped pair runs straight through.

test_relabelled_* start each family from a handle that apply_ops left relabelled (tile = 1, tile_relabel = 3, n = 15: the recipe
of the existing test_relabelled_state tests): the call settles it first, which is a k_permute_bits launch in the profile and,
on W1, a result in the caller's other tensor."""
from gpu_common import *  # noqa: F401,F403

import circuit_gradient_ref as CG
import diagonal_ref as DG
import expect_pauli_ref as E
import function_ref as F
import krylov_ref as K
import measure_ref as M
import noise_ref as NR  # noqa: F401
import pauli_pair_ref as PP
import pauli_rotation_ref as PR
import reduced_density_ref as D
import sample_many_ref as SM
import transition_ref as T
from test_gpu_f3_function import _hold_phase
from test_gpu_f3_noise import _run_chain, chain
from wrapped_common import Form, assert_buffer_contract, assert_twins, bits, close_forms, make_forms

pytestmark = pytest.mark.gpu

DTYPES = (np.complex128, np.complex64)
_IDS = ("c128", "c64")
BIG = 15


def _state(n, dtype, salt=0):
    return M.make_state(n, M.seed_of(n, dtype) + 1000 * salt, dtype)


def _same(a, b):
    """bit equality of returned values: arrays by their bytes, tuples and lists item by item, numbers by =="""
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))
    return a == b or (a != a and b != b)


def _one_handle(n, dtype, x, call, what):
    """call(st) on owned, W1 and W2 holding x: (the owned twin's returned value, its final vector) after the twin checks"""
    forms = make_forms(n, dtype, x)
    try:
        values = [call(f.st) for f in forms]
        final = assert_twins(forms, what)
        for f, v in zip(forms[1:], values[1:]):
            assert _same(values[0], v), f"{what}: {f.name} returned other values than the owned twin: {v!r} != {values[0]!r}"
        return values[0], final
    finally:
        close_forms(forms)


# ---- one handle --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, BIG))
@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_measurement_calls(O, dtype, n):
    """owned, W1, W2 at n = 1 and 15: norm_sqr, measure_probs (k = 1 .. 4, bit 0 and the top bit among them), measure_prob,
    soft_measure, soft_measure_many, sample, download_indices, then measure_state and a forced measure.  References of
    tests/measure_ref.py: probabilities within 1e-13, the norm within 1e-12 |psi|^2, an outcome is the exact crossing's
    (sample_many_ref.crossing_many) unless the sample lies within the margin of a partial sum (1e-9 / SOFT_MARGIN); the collapsed
    states EQUAL the oracle's measure_state, as tests/test_gpu_f1_measure_paths.py holds them."""
    x = _state(n, dtype)
    sets = [[n - 1]] if n == 1 else [[n - 1], [0, n - 1], [n - 1, 7, 0], [3, n - 1, 0, 9]]
    rs = SM.margin_samples(dtype, n, 64)
    picks = np.array([0, (1 << n) - 1] + ([5, 64, 4097] if n == BIG else []), dtype=np.uint64)
    forced = 1 if n == 1 else 2  # (outcome bit i is qubit sets[-1][i]: the qubit measure_state has just collapsed onto 1)

    def call(st):
        out = [st.norm_sqr()]
        for idx in sets:
            out += [st.measure_probs(idx), st.measure_prob(1, idx), st.soft_measure(idx, float(rs[0]))]
        out += [st.soft_measure_many(sets[-1], rs), st.sample(sets[-1], 32, seed=5), st.download_indices(picks)]
        st.measure_state(sets[0], 1, 0.37)
        out.append(st.download())
        out.append(st.measure(sets[-1], measured=forced))
        return out

    values, final = _one_handle(n, dtype, x, call, f"measure n={n} {np.dtype(dtype).name}")
    norm = M.norm_ref(x)
    assert abs(values[0] - norm) <= 1e-12 * norm
    at, dist = SM.crossing_many(x, rs)
    margin = 1e-9 if np.dtype(dtype) == np.complex128 else M.SOFT_MARGIN
    keep = np.flatnonzero(dist >= margin)
    assert len(keep) >= len(rs) - max(1, len(rs) // 16)
    pos = 1
    for idx in sets:
        probs, prob, soft = values[pos:pos + 3]
        pos += 3
        want = M.probs_ref(n, idx, x)
        assert np.max(np.abs(probs - want)) <= 1e-13 and abs(prob - want[1]) <= 1e-13, idx
        if 0 in keep:
            assert soft == M.outcome_of(n, idx, at[0]), idx
    many, sampled, picked, collapsed, (m, p) = values[pos:pos + 5]
    assert [int(many[i]) for i in keep] == [M.outcome_of(n, sets[-1], at[i]) for i in keep]
    rs2 = np.random.Generator(np.random.PCG64(5)).random(32)  # (sample's own draws; a Complex<f32> state rounds them to f32)
    rs2 = rs2.astype(np.float32).astype(np.float64) if np.dtype(dtype) == np.complex64 else rs2
    at2, dist2 = SM.crossing_many(x, rs2)
    keep2 = np.flatnonzero(dist2 >= margin)
    assert len(sampled) == 32 and [int(sampled[i]) for i in keep2] == [M.outcome_of(n, sets[-1], at2[i]) for i in keep2]
    assert np.array_equal(bits(picked), bits(x[picks.astype(np.int64)]))
    want = np.zeros_like(x)
    assert O.measure_state(n, sets[0], (1, 0.37), x, want)
    assert np.array_equal(collapsed, want)
    assert m == forced and abs(p - M.prob_ref(n, forced, sets[-1], collapsed)) <= 1e-13
    want2 = np.zeros_like(x)
    assert O.measure_state(n, sets[-1], (m, p), collapsed, want2)
    assert np.array_equal(final, want2)


@pytest.mark.parametrize("n", (1, BIG))
@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_pauli_expectations_and_rotations(dtype, n):
    """owned, W1, W2 at n = 1 (every string) and 15 (expect_pauli_ref.mask_cases: x = 0, bit 0 alone, the top bit, n_Y = 1 .. 5):
    expect_pauli within 1e-12 |psi|^2 of expect_ref_many; apply_pauli_rotations of all the terms in one call within
    pauli_rotation_ref's sequence bar 12 R u |psi|_2 of rotate_many_ref."""
    x = _state(n, dtype)
    terms = ([E.term_of_string(s) for s in E.all_strings(n)] if n == 1 else [E.term_of_masks(n, cx, cz) for _, cx, cz in E.mask_cases(n)])
    angles = np.random.default_rng(n).uniform(-3, 3, len(terms))

    def call(st):
        e = st.expect_pauli(terms)
        st.apply_pauli_rotations(terms, angles)
        return e

    e, final = _one_handle(n, dtype, x, call, f"pauli n={n} {np.dtype(dtype).name}")
    assert np.max(np.abs(e - E.expect_ref_many(n, terms, x))) <= 1e-12 * E.norm_sqr_ref(x)
    ok, worst = PR.within_sequence_bar(len(terms), final, PR.rotate_many_ref(n, terms, angles, x), x)
    print(f"n={n}: rotations |got - ref|_2 = {worst:.3f} R u |psi|_2, bar {PR.BAR}")
    assert ok


@pytest.mark.parametrize("n", (1, BIG))
@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_diagonal_sums(dtype, n):
    """owned, W1, W2 at n = 1 and 15: expect_diagonal and two apply_diagonal calls with different tables (40 and 7 random Z
    strings; at n = 15 they reach across the tile boundary at bit 12 and hold bit 0).  diagonal_ref: the moments within
    moment_bars, each phase pass within phase_bar of phase_ref on the vector it started from."""
    x = _state(n, dtype)
    tables = [DG.random_case(n, 40, 11 + n), DG.random_case(n, 7, 12 + n)]
    gammas = (0.7, -1.3)
    mids = []

    def call(st):
        zs, cs = tables[0]
        m = st.expect_diagonal([DG.z_term(n, z) for z in zs], cs)
        for (zs, cs), g in zip(tables, gammas):
            st.apply_diagonal([DG.z_term(n, z) for z in zs], cs, g)
            if len(mids) < 2:
                mids.append(st.download())  # (the owned twin runs first: its intermediate vectors)
        return m

    m, final = _one_handle(n, dtype, x, call, f"diagonal n={n} {np.dtype(dtype).name}")
    zs, cs = tables[0]
    bar1, bar2 = DG.moment_bars(n, len(zs), float(np.sum(np.abs(cs))), amps=x)
    ref1, ref2 = DG.moments_ref(n, zs, cs, x)
    assert abs(m[0] - ref1) <= bar1 and abs(m[1] - ref2) <= bar2
    assert np.array_equal(mids[1], final)
    start = x
    for (zs, cs), g, got in zip(tables, gammas, mids):
        ok, worst = DG.within_phase_bar(n, len(zs), float(np.sum(np.abs(g * cs))), got, DG.phase_ref(n, zs, cs, g, start), start)
        print(f"n={n} gamma={g}: worst / bar = {worst:.3f}")
        assert ok
        start = got


@pytest.mark.parametrize("n", (1, BIG))
@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_classical_functions(dtype, n):
    """owned, W1, W2 at n = 1 and 15: apply_function as XOR, as ADD, as XOR over seven out positions outside the row (two passes,
    n = 15), and as ADD with phases.  function_ref.apply_function_ref: without phases the result carries the input's bytes; with
    phases |got_j - ref_j| <= 8 u |psi_j| (test_gpu_f3_function._hold_phase)."""
    x = _state(n, dtype)
    rng = np.random.default_rng(20 + n)
    if n == 1:
        moves = [([], [0], "xor"), ([], [0], "add")]
        phased = ([0], [], "xor")
    else:
        wide = ([0, n - 1, n - 6], [n - 1 - p for p in list(range(6, 13))[::-1] + [3]], "xor")
        assert q.function_passes(n, wide[0], wide[1], "xor") == 2
        moves = [([n - 1, 0, 9], [n - 2, 5, 1, 7], "xor"), ([3, n - 1], [0, 8, n - 3], "add"), wide]
        phased = ([4, n - 1], [n - 2, 2, 10], "add")
    tabs = [rng.integers(0, 2 ** len(o), size=2 ** len(i), dtype=np.uint64) for i, o, _ in moves]
    ptab = rng.integers(0, 2 ** len(phased[1]), size=2 ** len(phased[0]), dtype=np.uint64) if phased[1] else None
    ph = rng.uniform(-7, 7, size=2 ** len(phased[0]))
    mids = []

    def call(st):
        for (ins, outs, mode), v in zip(moves, tabs):
            st.apply_function(ins, outs, values=v, mode=mode)
        if not mids:
            mids.append(st.download())
        st.apply_function(phased[0], phased[1], values=ptab, phases=ph, mode=phased[2])

    _, final = _one_handle(n, dtype, x, call, f"function n={n} {np.dtype(dtype).name}")
    want = x
    for (ins, outs, mode), v in zip(moves, tabs):
        want = F.apply_function_ref(n, want, ins, outs, v, None, mode)
    assert np.array_equal(bits(mids[0]), bits(want))
    ref = F.apply_function_ref(n, want, phased[0], phased[1], ptab, ph, phased[2])
    moved = np.abs(F.apply_function_ref(n, want, phased[0], phased[1], ptab, None, phased[2]).astype(np.complex128))
    nz = moved > 0
    assert np.all(final[~nz] == 0)
    _hold_phase(final[nz], ref[nz], moved[nz], F.UNIT[dtype], f"n={n} phases")


@pytest.mark.parametrize("n", (1, BIG))
@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_reduced_density_and_apply_reduce(dtype, n):
    """owned, W1, W2 at n = 1 and 15: reduced_density_matrix (k = 1 .. 6 at n = 15, bit 0 among the qubits) within
    reduced_density_ref's bar 1e-12 sqrt(rho_aa rho_a'a') of density_ref; apply_reduce of a random matrix: the state within
    TOL64 / TOL32 |A| |psi| of noise_ref.apply_reduce, the returned density within the same density bar (Complex<f32>: of the
    downloaded result), as tests/test_gpu_f3_noise.py holds them."""
    x = _state(n, dtype)
    rng = np.random.default_rng(30 + n)
    sets = [[0]] if n == 1 else [[n - 1], [n - 1, 0], [5, n - 1, 0, 9, 2, 12]]
    aq, bq = ([0], [0]) if n == 1 else ([n - 1, 3], [n - 1, 8])
    a = rng.standard_normal((1 << len(aq), 1 << len(aq))) + 1j * rng.standard_normal((1 << len(aq), 1 << len(aq)))

    def call(st):
        return [st.reduced_density_matrix(idx) for idx in sets] + [st.apply_reduce(aq, a, bq)]

    values, final = _one_handle(n, dtype, x, call, f"density n={n} {np.dtype(dtype).name}")
    for idx, rho in zip(sets, values):
        assert D.worst_ratio(rho, D.density_ref(n, idx, x)) <= 1.0 and D.exact_structure(rho), idx
    ref_y, ref_rho = NR.apply_reduce(n, aq, a, bq, x)
    tol = TOL64 if np.dtype(dtype) == np.complex128 else TOL32
    assert np.max(np.abs(final.astype(np.complex128) - ref_y)) <= tol * np.linalg.norm(a, 2) * np.linalg.norm(x.astype(np.complex128))
    if np.dtype(dtype) == np.complex64:
        ref_rho = D.density_ref(n, bq, final)
    assert D.worst_ratio(values[-1], ref_rho) <= 1.0 and D.exact_structure(values[-1])


@pytest.mark.parametrize("n,length", ((2, 2), (BIG, 6), (BIG, "mixed")))
@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_noise_channels(dtype, n, length):
    """owned, W1, W2 at n = 2 (two channels on qubits 0 and 1) and 15 (test_gpu_f3_noise.chain: six channels whose steps all
    fuse, and 'mixed', one of whose steps covers four qubits and runs composed — asserted through channel_passes).  The owned
    twin is held by test_gpu_f3_noise._run_chain: the chosen branches are noise_ref.trajectory's, every weight within
    1e-12 N of the reference on the state the channel met, the final state within the per-channel state bar."""
    chans, us = chain(n, length)
    x = _state(n, dtype, salt=2)
    if n == BIG:
        passes = q.channel_passes(n, chans)
        assert passes == ((len(chans) + 2, len(chans) - 2) if length == "mixed" else (len(chans) + 1, len(chans) - 1))
    forms = make_forms(n, dtype, x)
    try:
        what = f"channels n={n} {length} {np.dtype(dtype).name}"
        chosen, ws, y = _run_chain(forms[0].st, n, dtype, chans, us, x, what)
        for f in forms[1:]:
            c2, w2 = f.st.apply_channels(chans, us)
            assert _same([np.asarray(chosen), list(ws)], [np.asarray(c2), list(w2)]), (what, f.name)
        assert np.array_equal(assert_twins(forms, what), y)
    finally:
        close_forms(forms)


# ---- two handles -----------------------------------------------------------------------------------------------------------------
ARRANGEMENTS = ("W1+W1", "W1+owned", "W1+W2")


def _pair(arrangement, n, dtype, xa, xb):
    second = {"W1+W1": "W1", "W1+owned": "owned", "W1+W2": "W2", "owned+owned": "owned"}[arrangement]
    first = "owned" if arrangement == "owned+owned" else "W1"
    return Form(first, n, dtype, xa, salt=0), Form(second, n, dtype, xb, salt=1)  # (every W1 has a stream of its own)


def _two_handles(n, dtype, xa, xb, call, what, arrangements=ARRANGEMENTS):
    """call(a, b, probe) on an owned pair — probe(st) downloads an intermediate vector for the references — and on every
    arrangement of wrapped handles, where probe does nothing: (values, records, final a, final b) of the twin after the checks"""
    records = []
    ta, tb = _pair("owned+owned", n, dtype, xa, xb)
    try:
        values = call(ta.st, tb.st, lambda st: records.append(st.download()))
        fa, fb = ta.st.download(), tb.st.download()
        for arrangement in arrangements:
            a, b = _pair(arrangement, n, dtype, xa, xb)
            try:
                got = call(a.st, b.st, lambda st: None)
                where = f"{what} {arrangement}"
                assert _same(values, got), f"{where}: returned {got!r}, the owned pair {values!r}"
                assert np.array_equal(a.st.download(), fa) and np.array_equal(b.st.download(), fb), where
                for f in (a, b):
                    assert_buffer_contract(f, where)
            finally:
                a.close()
                b.close()
        return values, records, fa, fb
    finally:
        ta.close()
        tb.close()


def _pauli_terms(n):
    if n == 1:
        return [E.term_of_string(s) for s in E.all_strings(1)]
    return [PP.term_of_masks(n, cx, cz) for cx, cz in ((0, 0x4001), (1, 0x11), (1, 0x7000), (1 << (n - 1), 0x7001), (0x4102, 0x4106), (0, 0))]


@pytest.mark.parametrize("n", (1, BIG))
@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_pauli_sum_and_matrix_elements(dtype, n):
    """W1 + W1, W1 + owned, W1 + W2 at n = 1 and 15: a rotation queued on a, b <- H a at once, a <- a + H' b, <b| P |a>.
    pauli_pair_ref: every element of a sum within (count + 8) u (sum |c_t| |src| + |dst_old|) of pauli_sum_ref, the matrix
    elements within 1e-12 |bra| |ket| of matrix_elements_ref."""
    xa, xb = _state(n, dtype), _state(n, dtype, salt=1)
    terms = _pauli_terms(n)
    cs = np.random.default_rng(40 + n).standard_normal(len(terms)) + 1j * np.random.default_rng(41 + n).standard_normal(len(terms))
    few = min(3, len(terms))

    def call(a, b, probe):
        a.apply_pauli_rotations(terms[:1], [0.4])  # queued on a's stream
        probe(a)
        b.apply_pauli_sum(a, terms, cs)
        probe(b)
        a.apply_pauli_sum(b, terms[:few], cs[:few], accumulate=True)
        return b.pauli_matrix_elements(a, terms)

    me, (a1, b1), a2, b2 = _two_handles(n, dtype, xa, xb, call, f"pauli pair n={n} {np.dtype(dtype).name}")
    assert np.array_equal(b1, b2)
    ok, worst = PP.within_bar(b1, PP.pauli_sum_ref(n, terms, cs, a1), PP.sum_bar(n, terms, cs, a1))
    assert ok, worst
    ok, worst = PP.within_bar(a2, PP.pauli_sum_ref(n, terms[:few], cs[:few], b1, a1), PP.sum_bar(n, terms[:few], cs[:few], b1, a1))
    assert ok, worst
    assert np.max(np.abs(me - PP.matrix_elements_ref(n, terms, b1, a2))) <= PP.melem_bar(b1, a2)


@pytest.mark.parametrize("n", (1, BIG))
@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_transition_matrices(dtype, n):
    """W1 + W1, W1 + owned, W1 + W2 at n = 1 and 15: an H gate queued on the ket, then bra.transition_matrix(ket) on k = 1, 2, 3
    qubits with bit 0 and the top bit among them.  transition_ref: every entry within 1e-12 sqrt(rho_ket[a][a] rho_bra[a'][a'])."""
    xa, xb = _state(n, dtype), _state(n, dtype, salt=1)
    sets = [[0]] if n == 1 else [[n - 1], [0, n - 1], [n - 1, 6, 0]]
    h = q.make_matrix_op([n - 1], circuits.H)

    def call(a, b, probe):
        b.apply_op(h)  # queued on the ket's stream
        probe(b)
        return [a.transition_matrix(b, idx) for idx in sets]

    ms, (b1,), _, _ = _two_handles(n, dtype, xa, xb, call, f"transition n={n} {np.dtype(dtype).name}")
    for idx, m in zip(sets, ms):
        bar = T.bars(T.row_weights(n, idx, b1), T.row_weights(n, idx, xa))
        assert T.worst_ratio(m, T.transition_ref(n, idx, xa, b1), bar) <= 1.0, idx


@pytest.mark.parametrize("n", (1, BIG))
@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_vector_arithmetic(dtype, n):
    """W1 + W1, W1 + owned, W1 + W2 at n = 1 and 15: an H gate queued on b, then a <- c0 a + c1 b with its norm, <b|a> and <a|a>,
    b.copy_from(a), max_abs_diff of equal states, a gate on b, max_abs_diff again.  krylov_ref: the combination has the bytes of
    lincomb_spec, its norm within 1e-12 of norm_exact, the inner products within 1e-12 |bra| |ket| of inner_ref; max_abs_diff
    counts the amplitudes that differ exactly and gives their largest distance within 4 ulp (a subtraction and a hypot in
    double)."""
    xa, xb = _state(n, dtype), _state(n, dtype, salt=1)
    h = q.make_matrix_op([n - 1], circuits.H)
    cs = np.array([0.6 - 0.3j, -1.1 + 0.2j])

    def call(a, b, probe):
        b.apply_op(h)  # queued on b's stream
        probe(b)
        norm = a.linear_combination([a, b], cs, want_norm=True)
        probe(a)
        ip = a.inner_products([b, a])
        b.copy_from(a)
        same = a.max_abs_diff(b)
        b.apply_op(h)
        return norm, ip, same, a.max_abs_diff(b)

    (norm, ip, same, apart), (b1, a1), fa, fb = _two_handles(n, dtype, xa, xb, call, f"vector n={n} {np.dtype(dtype).name}")
    want = K.lincomb_spec([xa, b1], cs, dtype)
    assert np.array_equal(bits(a1), bits(want)) and np.array_equal(bits(fa), bits(want))
    assert abs(norm - K.norm_exact(want)) <= K.NORM_BAR * K.norm_exact(want)
    for got, bra in zip(ip, (b1, a1)):
        assert abs(got - K.inner_ref(bra, a1)) <= K.inner_bar(bra, a1)
    assert same == (0.0, 0)
    d = np.abs(fa.astype(np.complex128) - fb.astype(np.complex128))
    assert apart[1] == int(np.count_nonzero(fa != fb)) and abs(apart[0] - float(d.max())) <= 4 * 2.0 ** -53 * float(d.max())


@pytest.mark.parametrize("n", (4, BIG))
@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_gradients_with_a_wrapped_work_handle(dtype, n):
    """W1 + W1, W1 + owned, W1 + W2 at n = 4 (the smallest size of circuit_gradient_ref) and 15: adjoint_gradient
    (pauli_pair_ref.gradient_case: 12 rotations, a 10-term observable) and circuit_gradient (circuit_gradient_ref's `layers`
    circuit), the second handle the work state.  pauli_pair_ref.gradient_bars and circuit_gradient_ref.bars hold the energy, the
    gradient and the restored state against adjoint_gradient_ref and the clongdouble circuit_gradient_ref."""
    rot, angles, obs, oc = PP.gradient_case(n)
    circuit, params, terms, coeffs, psi0 = CG.case("layers", n, dtype)
    xb = _state(n, dtype, salt=1)

    def call(a, b, probe):
        first = a.adjoint_gradient(rot, angles, obs, oc, b)
        probe(a)
        a.upload(psi0)
        return first, a.circuit_gradient(circuit, params, terms, coeffs, b)

    x = _state(n, dtype)
    ((e1, g1), (e2, g2)), (back1,), back2, _ = _two_handles(n, dtype, x, xb, call, f"gradients n={n} {np.dtype(dtype).name}")
    e_ref, g_ref = PP.adjoint_gradient_ref(n, rot, angles, obs, oc, x)
    bar_e, bar_g = PP.gradient_bars(len(rot), oc, x)
    assert abs(e1 - e_ref) <= bar_e and np.max(np.abs(g1 - g_ref)) <= bar_g
    assert np.linalg.norm(back1.astype(np.complex128) - x.astype(np.complex128)) <= PP.restore_bar(len(rot), x)
    e_ref, g_ref = CG.circuit_gradient_ref(n, circuit, params, terms, coeffs, psi0)
    bar_e, bar_g, bar_r = CG.bars(circuit, params, coeffs, psi0)
    assert abs(e2 - e_ref) <= bar_e and np.all(np.abs(g2 - g_ref) <= bar_g)
    assert np.linalg.norm(back2.astype(np.complex128) - psi0.astype(np.complex128)) <= bar_r


@pytest.mark.parametrize("n", (2, BIG))
@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_krylov_basis_on_wrapped_basis_handles(dtype, n):
    """The start state W1 with three W1 basis handles (four torch streams), with three owned and with three W2 basis handles, at
    n = 2 (the smallest whose Krylov space holds the three vectors) and 15: krylov_basis of the Ising chain, m = 2, reorthogonalised.  krylov_ref: alphas and betas within
    B = krylov_bar(m, T, S, dtype) of the numpy restatement (lanczos); basis[0] within B / S of the restatement's (the bar of the
    existing orthonormality check); the start state is unchanged; everything bit-equal to the all-owned twin."""
    m = 2
    terms, coeffs = K.ising_chain(n)
    bar = K.bar(m, terms, coeffs, dtype)
    x = K.start_state(n, dtype)
    ar = K.Arith(n, terms, coeffs, dtype)
    want_a, want_b, want_basis, _ = K.lanczos(ar, ar.load(x), m, True, bar)
    filler = _state(n, dtype, salt=3)
    runs = {}
    for kind in ("owned", "W1", "W2"):
        psi = Form("owned" if kind == "owned" else "W1", n, dtype, x)
        basis = [Form(kind, n, dtype, filler, salt=2 + i) for i in range(m + 1)]
        try:
            a, b = psi.st.krylov_basis(terms, coeffs, [f.st for f in basis], reorthogonalize=True)
            runs[kind] = (a, b, [f.st.download() for f in basis])
            assert np.array_equal(bits(psi.st.download()), bits(x)), kind
            for f in [psi] + basis:
                assert_buffer_contract(f, f"krylov {kind} n={n}")
        finally:
            for f in [psi] + basis:
                f.close()
    a, b, vectors = runs["owned"]
    worst = float(max(np.max(np.abs(a - want_a)), np.max(np.abs(b - want_b))))
    print(f"n={n}: worst |alpha, beta - restated| = {worst:.3e}, B = {bar:.3e}")
    assert a.shape == b.shape == (m,) and worst <= bar
    unit = want_basis[0].astype(np.complex128)  # (the norm is a device reduction in another order: basis[0] within B / S, not its bytes)
    assert np.linalg.norm(vectors[0].astype(np.complex128) - unit) <= bar / K.weight(coeffs)
    for kind in ("W1", "W2"):
        assert _same(list(runs["owned"]), list(runs[kind])), kind


# ---- from a relabelled handle ------------------------------------------------------------------------------------------------------
def _relabelled(n, dtype, xs, names):
    """forms holding xs[i] with tile = 1, tile_relabel = 3 and profile = 1, each left relabelled by apply_ops (the recipe of the
    existing test_relabelled_state tests), the profile reset"""
    ops = circuits.c2_random_circuit(n, 80, seed=41)
    forms = [Form(name, n, dtype, x, salt=i) for i, (name, x) in enumerate(zip(names, xs))]
    for f in forms:
        f.set_options(tile=1, tile_relabel=3, profile=1)
        f.st.apply_ops(ops)
        f.st.profile_reset()
    return forms


def _swept(f):
    return f.launches().get("k_permute_bits", 0)


_ONE = {
    "measure": lambda st, n: [st.measure_probs([n - 1, 0]), st.soft_measure([n - 1], 0.4), st.norm_sqr(), st.measure([0, n - 1], measured=2)],
    "pauli": lambda st, n: [st.expect_pauli(_pauli_terms(n)), st.apply_pauli_rotations(_pauli_terms(n)[:3], [0.3, 0.5, -0.7])],
    "diagonal": lambda st, n: [st.expect_diagonal([{0: "Z", n - 1: "Z"}, {3: "Z"}], [0.5, -1.5]),
                               st.apply_diagonal([{0: "Z", n - 1: "Z"}, {3: "Z"}], [0.5, -1.5], 0.8)],
    "function": lambda st, n: [st.apply_function([n - 1, 0], [n - 2, 5, 7], values=np.arange(4, dtype=np.uint64) * 3 % 8, mode="add")],
    "density": lambda st, n: [st.reduced_density_matrix([n - 1, 0, 6]), st.apply_reduce([n - 1], [[0.6, 0.8j], [0.8j, 0.6]], [0, n - 1])],
    "channels": lambda st, n: list(st.apply_channels(*chain(n, 2))),
}


@pytest.mark.parametrize("family", sorted(_ONE))
@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_relabelled_one_handle(dtype, family):
    """owned and W1 at n = 15, left relabelled: each one-handle family settles the state first — one k_permute_bits launch in
    each profile — and then gives, bit for bit, what it gives on a settled owned twin (which the tests above hold to the
    references); on W1 the buffer contract holds after the settling sweep landed in the caller's other tensor."""
    n = BIG
    x = _state(n, dtype)
    forms = _relabelled(n, dtype, [x, x, x], ("owned", "owned", "W1"))
    settled = forms[0]
    try:
        start = settled.st.download()  # settles the twin: a restored layout moves amplitudes exactly
        assert _swept(settled) == 1, "the batch left no layout to restore"
        values = [_ONE[family](f.st, n) for f in forms]
        assert _swept(forms[1]) >= 1 and _swept(forms[2]) >= 1, "the call did not settle the relabelled state"
        assert _same(values[0], values[1]) and _same(values[0], values[2]), family
        final = settled.st.download()
        assert np.array_equal(forms[1].st.download(), final) and np.array_equal(forms[2].st.download(), final)
        assert start.shape == final.shape
        assert_buffer_contract(forms[2], f"relabelled {family}")
    finally:
        close_forms(forms)


_TWO = {
    "pauli_pair": lambda a, b, n: [b.apply_pauli_sum(a, _pauli_terms(n), np.arange(1, 7) * (0.3 - 0.1j)), b.pauli_matrix_elements(a, _pauli_terms(n))],
    "transition": lambda a, b, n: [a.transition_matrix(b, [n - 1, 0])],
    "vector": lambda a, b, n: [a.inner_products([b, a]), b.linear_combination([a, b], [0.5, 0.25j], want_norm=True), a.max_abs_diff(b)],
    "copy": lambda a, b, n: [b.copy_from(a), a.max_abs_diff(b)],
    "gradient": lambda a, b, n: [a.adjoint_gradient(*PP.gradient_case(n)[:2], *PP.gradient_case(n)[2:], b)],
}


@pytest.mark.parametrize("family", sorted(_TWO))
@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_relabelled_two_handles(dtype, family):
    """An owned pair and a W1 + W1 pair at n = 15, all four left relabelled: each two-handle family settles both of its handles
    first (a k_permute_bits launch in both profiles) and gives, bit for bit, what the owned pair gives; buffer contract on both
    W1 handles."""
    n = BIG
    xa, xb = _state(n, dtype), _state(n, dtype, salt=1)
    forms = _relabelled(n, dtype, [xa, xb, xa, xb], ("owned", "owned", "W1", "W1"))
    try:
        want = _TWO[family](forms[0].st, forms[1].st, n)
        got = _TWO[family](forms[2].st, forms[3].st, n)
        for i, f in enumerate(forms):  # (copy_from overwrites its destination: that one has nothing to restore)
            assert _swept(f) >= 1 or (family == "copy" and i % 2 == 1), (family, i, f.name, "no settling sweep")
        assert _same(want, got), family
        for twin, f in ((forms[0], forms[2]), (forms[1], forms[3])):
            assert np.array_equal(f.st.download(), twin.st.download()), family
            assert_buffer_contract(f, f"relabelled {family}")
    finally:
        close_forms(forms)


def test_relabelled_krylov_basis():
    """A relabelled W1 start state with three W1 basis handles beside an all-owned twin, n = 15, Complex<f64>: krylov_basis
    settles the start state (a k_permute_bits launch) and returns the twin's alphas, betas and basis vectors bit for bit."""
    n, dtype = BIG, np.complex128
    terms, coeffs = K.ising_chain(n)
    x = _state(n, dtype)
    runs = []
    for kind in ("owned", "W1"):
        psi, = _relabelled(n, dtype, [x], (kind,))
        basis = [Form(kind, n, dtype, x, salt=2 + i) for i in range(3)]
        try:
            a, b = psi.st.krylov_basis(terms, coeffs, [f.st for f in basis])
            assert _swept(psi) >= 1
            runs.append([a, b] + [f.st.download() for f in basis])
            for f in [psi] + basis:
                assert_buffer_contract(f, f"relabelled krylov {kind}")
        finally:
            for f in [psi] + basis:
                f.close()
    assert _same(runs[0], runs[1])
