"""The two-state Pauli calls on device states (include/qip_hipx.h): dst (+)= (sum_t c_t P_t) src (k_pauli_sum), <bra| P |ket>
(k_pauli_melem) and HipState.adjoint_gradient built from them and the rotations.

The references and the bars are those of tests/pauli_pair_ref.py, with u = 2^-53 (Complex<f64>) or 2^-24 (Complex<f32>):

    Pauli sum, element by element:   |got_j - ref_j| <= (count + 8) u (sum_t |c_t| |src[j ^ x_t]| + |dst_old[j]|)
    matrix element:                  |got - ref| <= 1e-12 ||phi||_2 ||psi||_2
    adjoint gradient:                |grad_k - ref_k| <= 2 S ||psi_0||^2 ((48 T + count + 8) u + 1e-12)
                                     |E - ref|        <=   S ||psi_0||^2 ((24 T + count + 8) u + 1e-12)

Both kernels walk k_expect_pauli's geometry, so the sizes are those of the expect and rotate tests: n = 1, 2, 3 below one wave,
n = 9 the row loop of one block, n = 13 one whole span per block or two blocks, n = 22 hundreds of blocks.  Every test prints its
worst figure before it asserts."""
import ctypes as C
import subprocess

from gpu_common import *  # noqa: F401,F403

import expect_pauli_ref as E
import pauli_pair_ref as P
import pauli_rotation_ref as R
from rustqip_amd import _ffi
from test_gpu_f1_expect_pauli import MANY_BLOCK_MASKS

pytestmark = pytest.mark.gpu

_IDS = ("c128", "c64")
_STATES = {}
GROUP_DEFAULT = 16  # the default of option "sum_group"


def _state(n, dtype, norm=1.0, salt=0):
    """the case state of (n, dtype, norm, salt): shared, never written to; another salt is another seed"""
    key = (n, np.dtype(dtype), norm, salt)
    if key not in _STATES:
        x = P.make_state(n, P.seed_of(n, dtype) + 1000 * salt, dtype, norm=norm)
        x.setflags(write=False)
        _STATES[key] = x
    return _STATES[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _summed(dst, src, x, terms, coeffs, old=None):
    """the download of dst after dst (+)= H src; src holds x already"""
    if old is not None:
        dst.upload(old)
    dst.apply_pauli_sum(src, terms, coeffs, accumulate=old is not None)
    return dst.download()


def _hold_sum(n, terms, coeffs, got, x, old, what):
    bar = P.sum_bar(n, terms, coeffs, x, old)
    ok, worst = P.within_bar(got, P.pauli_sum_ref(n, terms, coeffs, x, old), bar)
    print(f"{what}: worst |got - ref| = {worst * (len(terms) + P.SUM_SLACK):.2f} u scale, bar {len(terms) + P.SUM_SLACK:.0f}")
    assert ok, what


def _hold_elements(n, terms, got, bra, ket, what):
    ref, bar = P.matrix_elements_ref(n, terms, bra, ket), P.melem_bar(bra, ket)
    worst = float(np.max(np.abs(got - ref))) if len(terms) else 0.0
    print(f"{what}: worst |got - ref| = {worst:.3e}, bar {bar:.3e}")
    assert got.dtype == np.complex128 and got.shape == (len(terms),)
    assert worst <= bar, what


def _coeffs(count, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(count) + 1j * rng.standard_normal(count)


# ---- 1: below one wave ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", P.DTYPES, ids=_IDS)
def test_tiny_vectors(dtype):
    """every Pauli string on n = 1, 2 and 3: one sum each (alternately storing and accumulating), all matrix elements in one call"""
    for n in (1, 2, 3):
        x, y = _state(n, dtype, 0.8), _state(n, dtype, 0.6, salt=1)
        strings = P.all_strings(n)
        cs = _coeffs(len(strings), 31 + n)
        with q.HipState(n, dtype) as src, q.HipState(n, dtype) as dst:
            src.upload(x)
            for i, (s, c) in enumerate(zip(strings, cs)):
                old = y if i % 2 else None
                got = _summed(dst, src, x, [s], [c], old)  # (the string form of a term)
                term = [P.term_of_string(s)]
                ok, w = P.within_bar(got, P.pauli_sum_ref(n, term, [c], x, old), P.sum_bar(n, term, [c], x, old))
                assert ok, (n, s, w)
            assert np.array_equal(_bits(src.download()), _bits(x))
            dst.upload(y)
            got = dst.pauli_matrix_elements(src, strings)
        _hold_elements(n, [P.term_of_string(s) for s in strings], got, y, x, f"n={n} all strings")


# ---- 2: the Pauli sum, one block and several blocks ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (9, 13))
@pytest.mark.parametrize("dtype", P.DTYPES, ids=_IDS)
def test_sum_of_one_term(dtype, n):
    """every case of mask_cases(n) alone, with a complex coefficient: x = 0, x = bit 0 alone (inside a packed Complex<f32> element:
    the unpacked pair pass), the top bit, all bits, n_Y = 1 .. 5 with bit 0 set and clear; storing and accumulating in turn"""
    x, y = _state(n, dtype), _state(n, dtype, 0.5, salt=1)
    cases = P.mask_cases(n)
    cs = _coeffs(len(cases), 50 + n)
    with q.HipState(n, dtype) as src, q.HipState(n, dtype) as dst:
        src.upload(x)
        for i, ((name, cx, cz), c) in enumerate(zip(cases, cs)):
            term, old = [P.term_of_masks(n, cx, cz)], (y if i % 2 else None)
            got = _summed(dst, src, x, term, [c], old)
            _hold_sum(n, term, [c], got, x, old, f"n={n} {name} accumulate={old is not None}")
        assert np.array_equal(_bits(src.download()), _bits(x))


@pytest.mark.parametrize("accumulate", (False, True), ids=("store", "accumulate"))
@pytest.mark.parametrize("n", (9, 13))
@pytest.mark.parametrize("dtype", P.DTYPES, ids=_IDS)
def test_sum_of_a_batch(dtype, n, accumulate):
    """67 terms over three x masks (bit 0 set: 41 terms, more than one pass under any group; bit 0 clear; zero with the empty
    term) under the default group and under 1, 4 and 32 (every kernel capacity), each held to the bar (no bit promise across
    groupings); the same call twice leaves the same bits"""
    x, old = _state(n, dtype), (_state(n, dtype, 0.5, salt=1) if accumulate else None)
    terms, cs = P.batch_case(n)
    assert q.pauli_sum_passes(n, terms) == P.batch_passes(GROUP_DEFAULT)
    with q.HipState(n, dtype) as src, q.HipState(n, dtype) as dst:
        src.upload(x)
        got = _summed(dst, src, x, terms, cs, old)
        _hold_sum(n, terms, cs, got, x, old, f"n={n} batch default group")
        if not accumulate:
            dst.upload(_state(n, dtype, 0.5, salt=2))  # (whatever the destination held is gone)
        again = _summed(dst, src, x, terms, cs, old)
        assert np.array_equal(_bits(again), _bits(got))
        for group in (1, 4, 32):
            dst.set_option("sum_group", group)
            _hold_sum(n, terms, cs, _summed(dst, src, x, terms, cs, old), x, old, f"n={n} batch group {group}")
        # no terms: zero, or the destination as it is
        dst.upload(x)
        dst.apply_pauli_sum(src, [], [], accumulate=accumulate)
        assert np.array_equal(_bits(dst.download()), _bits(x if accumulate else np.zeros_like(x)))


@pytest.mark.parametrize("dtype", P.DTYPES, ids=_IDS)
def test_many_blocks(dtype):
    """n = 22, the family "mixed" of the expect tests' MANY_BLOCK_MASKS (a pair mask with n_Y = 2 and 5, a Z string, the empty
    term): hundreds of blocks, whole spans per lane and row; the sum accumulating, the matrix elements as one call"""
    n = 22
    x, y = _state(n, dtype), _state(n, dtype, 0.5, salt=1)
    terms = [P.term_of_masks(n, cx, cz) for cx, cz in MANY_BLOCK_MASKS["mixed"]]
    cs = _coeffs(len(terms), 22)
    with q.HipState(n, dtype) as src, q.HipState(n, dtype) as dst:
        src.upload(x)
        got = _summed(dst, src, x, terms, cs, y)
        dst.upload(y)
        elements = dst.pauli_matrix_elements(src, terms)
    _hold_sum(n, terms, cs, got, x, y, f"n={n} mixed")
    _hold_elements(n, terms, elements, y, x, f"n={n} mixed")


@pytest.mark.parametrize("n", (9, 13))
@pytest.mark.parametrize("dtype", P.DTYPES, ids=_IDS)
def test_sum_against_a_rotation(dtype, n):
    """exp(-i theta P) psi = cos theta psi - i sin theta P psi as one two-term sum (the I term and P) against
    apply_pauli_rotations on a twin: apart by at most the sum of the two element bars"""
    theta = 0.7
    x = _state(n, dtype)
    with q.HipState(n, dtype) as src, q.HipState(n, dtype) as dst, q.HipState(n, dtype) as twin:
        src.upload(x)
        for name, cx, cz in P.mask_cases(n)[::2]:
            term = P.term_of_masks(n, cx, cz)
            terms, cs = [{}, term], [math.cos(theta), -1j * math.sin(theta)]
            got = _summed(dst, src, x, terms, cs)
            twin.upload(x)
            twin.apply_pauli_rotations([term], [theta])
            want = twin.download()
            bar = P.sum_bar(n, terms, cs, x) + R.element_bar(n, term, x)
            ok, worst = P.within_bar(got, want.astype(np.complex128), bar)
            print(f"n={n} {name}: worst |sum - rotation| = {worst:.3f} of the two bars")
            assert ok, name


# ---- 3: matrix elements ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (9, 13))
@pytest.mark.parametrize("dtype", P.DTYPES, ids=_IDS)
def test_matrix_elements(dtype, n):
    """every case of mask_cases(n) between two states of different seeds; a batch is its single-term calls bit for bit under
    expect_group 1, 4 and 16; <a|b> = conj(<b|a>); both states bit-unchanged"""
    phi, psi = _state(n, dtype, 0.7, salt=1), _state(n, dtype)
    terms = [P.term_of_masks(n, cx, cz) for _, cx, cz in P.mask_cases(n)] + [{}]
    with q.HipState(n, dtype) as bra, q.HipState(n, dtype) as ket:
        bra.upload(phi)
        ket.upload(psi)
        got = bra.pauli_matrix_elements(ket, terms)
        _hold_elements(n, terms, got, phi, psi, f"n={n} mask cases")
        singles = np.array([bra.pauli_matrix_elements(ket, [t])[0] for t in terms])
        assert np.array_equal(_bits(singles), _bits(got))
        for group in (1, 4, 16, 32):  # (32: the call takes min(expect_group, 16))
            ket.set_option("expect_group", group)
            assert np.array_equal(_bits(bra.pauli_matrix_elements(ket, terms)), _bits(got)), group
        ab, ba = bra.inner(ket), ket.inner(bra)
        print(f"n={n}: |<a|b> - conj(<b|a>)| = {abs(ab - ba.conjugate()):.3e}, bar {P.melem_bar(phi, psi):.3e}")
        assert abs(ab - ba.conjugate()) <= P.melem_bar(phi, psi) and ab == got[-1]
        assert bra.pauli_matrix_elements(ket, []).shape == (0,)
        assert np.array_equal(_bits(bra.download()), _bits(phi)) and np.array_equal(_bits(ket.download()), _bits(psi))


@pytest.mark.parametrize("n", (9, 13))
@pytest.mark.parametrize("dtype", P.DTYPES, ids=_IDS)
def test_matrix_elements_of_a_batch(dtype, n):
    """the 67 terms of the batch case (runs of 41, 20 and 6 terms of one mask: several passes under every group) against the
    reference and against the single-term calls, bit for bit"""
    phi, psi = _state(n, dtype, 0.7, salt=1), _state(n, dtype)
    terms, _ = P.batch_case(n)
    with q.HipState(n, dtype) as bra, q.HipState(n, dtype) as ket:
        bra.upload(phi)
        ket.upload(psi)
        got = bra.pauli_matrix_elements(ket, terms)
        singles = np.array([bra.pauli_matrix_elements(ket, [t])[0] for t in terms])
        for group in (1, 4):
            ket.set_option("expect_group", group)
            assert np.array_equal(_bits(bra.pauli_matrix_elements(ket, terms)), _bits(got)), group
    _hold_elements(n, terms, got, phi, psi, f"n={n} batch")
    assert np.array_equal(_bits(singles), _bits(got))


@pytest.mark.parametrize("n", (9, 13))
@pytest.mark.parametrize("dtype", P.DTYPES, ids=_IDS)
def test_one_state_as_bra_and_ket(dtype, n):
    """bra is ket, the Hermitian case: the real part agrees with expect_pauli at 2e-12 norm^2 (either call's bar), the imaginary
    part is below the bar"""
    psi = _state(n, dtype, 0.5)
    terms = [P.term_of_masks(n, cx, cz) for _, cx, cz in P.mask_cases(n)] + [{}]
    with q.HipState(n, dtype) as st:
        st.upload(psi)
        got, want = st.pauli_matrix_elements(st, terms), st.expect_pauli(terms)
        assert np.array_equal(_bits(st.download()), _bits(psi))
    norm2 = E.norm_sqr_ref(psi)
    print(f"n={n}: worst real part {np.max(np.abs(got.real - want)):.3e} (bar {2e-12 * norm2:.3e}), imaginary {np.max(np.abs(got.imag)):.3e}")
    assert np.all(np.abs(got.real - want) <= 2e-12 * norm2)
    assert np.all(np.abs(got.imag) <= P.MELEM_BAR * norm2)
    _hold_elements(n, terms, got, psi, psi, f"n={n} bra is ket")


@pytest.mark.parametrize("n", (9, 13))
@pytest.mark.parametrize("dtype", P.DTYPES, ids=_IDS)
def test_sum_then_inner_is_the_expectation(dtype, n):
    """work <- H psi, then <psi|work> against psi.expectation(terms, c), real c: apart by at most the sum's bar through
    Cauchy-Schwarz ((count + 8) u S norm^2) plus the bars of the two calls (1e-12 S norm^2 each)"""
    psi = _state(n, dtype, 0.5)
    terms, cs = P.batch_case(n)
    cs = cs.real.copy()
    S, norm2 = float(np.sum(np.abs(cs))), E.norm_sqr_ref(psi)
    with q.HipState(n, dtype) as st, q.HipState(n, dtype) as work:
        st.upload(psi)
        work.apply_pauli_sum(st, terms, cs)
        got, want = st.inner(work), st.expectation(terms, cs)
    bar = ((len(terms) + P.SUM_SLACK) * P.unit_roundoff(dtype) + 2 * P.MELEM_BAR) * S * norm2
    print(f"n={n}: |<psi|H psi> - expectation| = {abs(got - want):.3e}, bar {bar:.3e}")
    assert abs(got - want) <= bar


# ---- 4: the adjoint gradient -------------------------------------------------------------------------------------------------------
def _energy(st, x, rot, angles, obs, cs):
    st.upload(x)
    st.apply_pauli_rotations(rot, angles)
    return st.expectation(obs, cs)


@pytest.mark.parametrize("n", (10, 13))
@pytest.mark.parametrize("dtype", P.DTYPES, ids=_IDS)
def test_adjoint_gradient(dtype, n):
    """T = 12 strings (two consecutive ones of one x mask, a Z-only string), an observable of 10 terms with the identity, against
    adjoint_gradient_ref; the state is back within 12 * 2T u ||psi_0||; one angle also against parameter shift through the
    existing calls, E(theta_k + pi/4) - E(theta_k - pi/4), exact for these rotations, at twice the energy bar"""
    x = _state(n, dtype, 0.9)
    rot, angles, obs, cs = P.gradient_case(n)
    T = len(rot)
    want_e, want_g = P.adjoint_gradient_ref(n, rot, angles, obs, cs, x)
    bar_e, bar_g = P.gradient_bars(T, cs, x)
    with q.HipState(n, dtype) as st, q.HipState(n, dtype) as work:
        st.upload(x)
        energy, grad = st.adjoint_gradient(rot, angles, obs, cs, work)
        back = st.download()
        norm_work = work.norm_sqr()
        k = 5
        shift = np.zeros(T)
        shift[k] = math.pi / 4
        ps = _energy(st, x, rot, angles + shift, obs, cs) - _energy(st, x, rot, angles - shift, obs, cs)
    print(f"n={n}: |E - ref| = {abs(energy - want_e):.3e} (bar {bar_e:.3e}), worst |grad - ref| = {np.max(np.abs(grad - want_g)):.3e} "
          f"(bar {bar_g:.3e}), |grad[{k}] - parameter shift| = {abs(grad[k] - ps):.3e} (bar {2 * bar_e:.3e})")
    away = float(np.linalg.norm(back.astype(np.complex128) - x.astype(np.complex128)))
    print(f"n={n}: the state is {away:.3e} from psi_0, bar {P.restore_bar(T, x):.3e}")
    assert isinstance(energy, float) and grad.dtype == np.float64 and grad.shape == (T,)
    assert abs(energy - want_e) <= bar_e
    assert np.all(np.abs(grad - want_g) <= bar_g)
    assert np.max(np.abs(want_g)) > 100 * bar_g  # (the gradient is not small against its bar)
    assert away <= P.restore_bar(T, x)
    S = float(np.sum(np.abs(cs)))
    assert 0 < norm_work <= (S * S) * E.norm_sqr_ref(x) * 1.001 and math.isfinite(norm_work)  # `work` holds a valid state: H psi_T rotated back
    assert abs(grad[k] - ps) <= 2 * bar_e


@pytest.mark.parametrize("dtype", P.DTYPES, ids=_IDS)
def test_adjoint_gradient_refusals(dtype):
    n = 6
    x = _state(n, dtype)
    rot, obs = ["XIIZII", "IYIIXI"], ["ZZIIII", "IIIIII"]
    with q.HipState(n, dtype) as st, q.HipState(n, dtype) as work, q.HipState(n + 1, dtype) as wider, \
            q.HipState(n, np.complex64 if dtype == np.complex128 else np.complex128) as other:
        st.upload(x)
        work.upload(x)
        for args in ((rot, [0.1], obs, [1.0, 2.0], work), (rot, [0.1, 0.2], obs, [1.0], work), (rot, [0.1, 0.2], obs, [1.0, 2.0], wider),
                     (rot, [0.1, 0.2], obs, [1.0, 2.0], other), (rot, [0.1, 0.2], obs, [1.0, 2.0], st), (rot, [0.1, float("nan")], obs, [1.0, 2.0], work),
                     (rot, [0.1, 0.2], obs, [1.0, float("inf")], work), (["XX"], [0.1], obs, [1.0, 2.0], work), (rot, [0.1, 0.2], [{n: "Z"}, {}], [1.0, 2.0], work)):
            with pytest.raises((q.CircuitError, q.QipHipError)):
                st.adjoint_gradient(*args)
            assert np.array_equal(_bits(st.download()), _bits(x)) and np.array_equal(_bits(work.download()), _bits(x))
        energy, grad = st.adjoint_gradient([], [], obs, [1.0, 2.0], work)  # no angles: the energy alone
        assert grad.shape == (0,) and abs(energy - st.expectation(obs, [1.0, 2.0])) <= 1e-6


# ---- 5: relabelled handles ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", P.DTYPES, ids=_IDS)
def test_relabelled_states(dtype):
    """tile = 1 with tile_relabel = 3 at n = 15 (the setting of the rotate tests' test_relabelled_state): apply_ops leaves both
    handles relabelled and either call restores the caller's order of both first — seen as a permutation sweep in each profile;
    the results are those of settled twins, bit for bit"""
    n = 15
    ops = circuits.c2_random_circuit(n, 80, seed=41)
    xa, xb = _state(n, dtype), _state(n, dtype, 0.5, salt=1)
    terms = [P.term_of_masks(n, cx, cz) for cx, cz in ((0, 0x4001), (1, 0x11), (1, 0x7000), (1 << (n - 1), 0x7001), (0x4102, 0x4106), (0, 0))]
    cs = _coeffs(len(terms), 15)
    with q.HipState(n, dtype) as a, q.HipState(n, dtype) as b, q.HipState(n, dtype) as ta, q.HipState(n, dtype) as tb:
        def relabel():
            for st, x in ((a, xa), (b, xb)):
                st.upload(x)
                st.apply_ops(ops)
                st.profile_reset()

        def swept(st):
            return st.profile().get("k_permute_bits", {}).get("launches", 0)

        for st in (a, b):
            st.set_option("tile", 1)
            st.set_option("tile_relabel", 3)
            st.set_option("profile", 1)
        relabel()
        ta.copy_from(a)  # (settles: copies in the caller's order)
        tb.copy_from(b)
        relabel()
        got = a.pauli_matrix_elements(b, terms)
        assert swept(a) >= 1 and swept(b) >= 1, "a batch left no layout to restore"
        assert np.array_equal(_bits(got), _bits(ta.pauli_matrix_elements(tb, terms)))
        relabel()
        b.apply_pauli_sum(a, terms, cs, accumulate=True)
        assert swept(a) >= 1 and swept(b) >= 1, "a batch left no layout to restore"
        tb.apply_pauli_sum(ta, terms, cs, accumulate=True)
        assert b.max_abs_diff(tb) == (0.0, 0) and a.max_abs_diff(ta) == (0.0, 0)


# ---- 6: ordering ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", P.DTYPES, ids=_IDS)
def test_ordered_after_the_source_and_complete_on_return(dtype):
    """apply_ops queued on the source with no synchronise, the sum, and at once another apply_ops on the source: the destination
    holds what a run with explicit synchronises leaves, bit for bit"""
    n = 12
    layer = circuits.h_layer(n)
    terms = ["ZIIIIIIIIIIZ", "XIIIIIIIIIIX", "IYIIIIZIIIXI", "IIIIIIIIIIII", "IIXIIIIIYIIZ"]
    cs = _coeffs(len(terms), 12)
    with q.HipState(n, dtype) as src, q.HipState(n, dtype) as dst:
        src.init_basis(5)
        src.apply_ops(layer)
        dst.apply_pauli_sum(src, terms, cs)  # no synchronise before ...
        src.apply_ops(layer)                 # ... and none after
        got = dst.download()
        after = src.download()
        src.init_basis(5)
        src.apply_ops(layer)
        src.sync()
        y = src.download()
        dst.apply_pauli_sum(src, terms, cs)
        dst.sync()
        src.sync()
        src.apply_ops(layer)
        src.sync()
        want = dst.download()
        assert np.array_equal(_bits(after), _bits(src.download()))
    assert np.array_equal(_bits(got), _bits(want))
    _hold_sum(n, [P.term_of_string(s) for s in terms], cs, got, y, None, "after one layer")


# ---- 7: refusals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", P.DTYPES, ids=_IDS)
def test_refusals(dtype):
    n = 5
    x, y = _state(n, dtype), _state(n, dtype, 0.5, salt=1)
    add, elem = _ffi.lib.qipx_state_apply_pauli_sum, _ffi.lib.qipx_state_pauli_matrix_elements
    u64, u8, dbl = lambda v: (C.c_uint64 * len(v))(*v), lambda v: (C.c_uint8 * len(v))(*v), lambda v: (C.c_double * len(v))(*v)
    good = (u64([0, 2, 3]), u64([0, 3, 1]), u8([1, 3, 2]))
    cs = dbl([0.4, -1.2, 0.3, 0.8])
    values = dbl([7.0] * 4)
    other_dtype = np.complex64 if dtype == np.complex128 else np.complex128
    with q.HipState(n, dtype) as src, q.HipState(n, dtype) as dst, q.HipState(n + 1, dtype) as wider, q.HipState(n, other_dtype) as other:
        src.upload(x)
        dst.upload(y)
        wider.init_basis(3)
        other.init_basis(3)

        def refused(rc, code=_ffi.QIP_ERR_INVALID):
            message = _ffi.last_error()
            assert rc == code and message
            assert np.array_equal(_bits(dst.download()), _bits(y)) and np.array_equal(_bits(src.download()), _bits(x))
            assert list(values) == [7.0] * 4
            return message

        for accumulate in (0, 1):
            refused(add(dst._h, dst._h, *good, cs, 2, accumulate))      # dst is src
            refused(add(dst._h, None, *good, cs, 2, accumulate))        # no source
            refused(add(None, src._h, *good, cs, 2, accumulate))        # no destination
            refused(add(dst._h, wider._h, *good, cs, 2, accumulate))    # differing n
            refused(add(wider._h, src._h, *good, cs, 2, accumulate))
            refused(add(dst._h, other._h, *good, cs, 2, accumulate))    # differing dtype
            for null in range(4):
                args = list(good) + [cs]
                args[null] = None
                refused(add(dst._h, src._h, *args, 2, accumulate))
            for bad in (float("nan"), float("inf"), -float("inf")):
                for at in (2, 3):  # the real and the imaginary part of the last term's coefficient
                    c = [0.4, -1.2, 0.3, 0.8]
                    c[at] = bad
                    assert "term 1" in refused(add(dst._h, src._h, *good, dbl(c), 2, accumulate))
            refused(add(dst._h, src._h, good[0], u64([3, 3, 1]), good[2], cs, 2, accumulate))            # repeated inside a term
            refused(add(dst._h, src._h, good[0], good[1], u8([1, 4, 2]), cs, 2, accumulate))             # code 4
            refused(add(dst._h, src._h, good[0], u64([0, n, 1]), good[2], cs, 2, accumulate))            # qubit = n
            refused(add(dst._h, src._h, u64([0, 2, 1]), good[1], good[2], cs, 2, accumulate))            # decreasing
            refused(add(dst._h, src._h, u64([1, 2, 3]), good[1], good[2], cs, 2, accumulate))            # term_start[0] != 0
        refused(elem(dst._h, None, *good, 2, values))
        refused(elem(None, src._h, *good, 2, values))
        refused(elem(dst._h, wider._h, *good, 2, values))
        refused(elem(dst._h, other._h, *good, 2, values))
        for null in range(4):
            args = list(good) + [values]
            args[null] = None
            refused(elem(dst._h, src._h, args[0], args[1], args[2], 2, args[3]))
        refused(elem(dst._h, src._h, good[0], u64([3, 3, 1]), good[2], 2, values))
        refused(elem(dst._h, src._h, good[0], good[1], u8([1, 4, 2]), 2, values))
        refused(elem(dst._h, src._h, good[0], u64([0, n, 1]), good[2], 2, values))
        refused(elem(dst._h, src._h, u64([0, 2, 1]), good[1], good[2], 2, values))
        refused(elem(dst._h, src._h, u64([1, 2, 3]), good[1], good[2], 2, values))
        for call in (lambda: dst.apply_pauli_sum(wider, ["ZIIII"], [1.0]), lambda: dst.apply_pauli_sum(other, ["ZIIII"], [1.0]),
                     lambda: dst.apply_pauli_sum(dst, ["ZIIII"], [1.0]), lambda: dst.apply_pauli_sum(src, ["ZIIII", "XIIII"], [1.0]),
                     lambda: dst.apply_pauli_sum(src, ["XX"], [1.0]), lambda: dst.apply_pauli_sum(src, [{n: "X"}], [1.0]),
                     lambda: dst.apply_pauli_sum(src, [{0: "W"}], [1.0]), lambda: dst.pauli_matrix_elements(wider, ["ZIIII"]),
                     lambda: dst.pauli_matrix_elements(other, ["ZIIII"]), lambda: dst.inner(wider)):
            with pytest.raises(q.CircuitError):
                call()
        for value in (0, -1, 33):
            with pytest.raises(q.CircuitError):
                dst.set_option("sum_group", value)
        refused(_ffi.QIP_ERR_INVALID)  # (nothing above touched a state)
        assert elem(dst._h, src._h, None, None, None, 0, None) == _ffi.QIP_OK  # no terms: nothing to do, null arrays allowed
        assert add(dst._h, src._h, None, None, None, None, 0, 1) == _ffi.QIP_OK  # accumulating nothing
        assert np.array_equal(_bits(dst.download()), _bits(y))
        # and both still work
        terms = [{0: "X", 3: "Z"}, {1: "Y"}]
        assert elem(dst._h, src._h, *good, 2, values) == _ffi.QIP_OK
        got_values = np.array(list(values)).view(np.complex128)
        assert add(dst._h, src._h, *good, cs, 2, 1) == _ffi.QIP_OK
        got = dst.download()
        assert add(dst._h, src._h, None, None, None, None, 0, 0) == _ffi.QIP_OK  # storing nothing: zero
        assert not np.any(dst.download())
    _hold_elements(n, terms, got_values, y, x, "after the refusals")
    _hold_sum(n, terms, [0.4 - 1.2j, 0.3 + 0.8j], got, x, y, "after the refusals")


# ---- 8: the C++ mirror -----------------------------------------------------------------------------------------------------------
def test_cpp_mirror(tmp_path):
    n = 10
    a, b = _state(n, np.complex128), _state(n, np.complex128, 0.5, salt=1)
    rng = np.random.default_rng(13)
    strings = ["".join(rng.choice(list("IXYZ"), n)) for _ in range(10)] + ["I" * n, "Z" * n, "Y" * n]
    cs = _coeffs(len(strings), 14)
    exe = str(tmp_path / "test_pair_mirror")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "rustqip_amd", "host"), os.path.join(ROOT, "tests", "cpp", "test_pair_mirror.cpp"),
                    "-o", exe, "-L" + os.path.join(ROOT, "rustqip_amd", "lib"), "-lqip_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "rustqip_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib",
                    "-Wl,-rpath-link,/opt/rocm/lib"], check=True, capture_output=True)
    a.tofile(tmp_path / "a.bin")
    b.tofile(tmp_path / "b.bin")
    args = [v for s, c in zip(strings, cs) for v in (s, float(c.real).hex(), float(c.imag).hex())]
    res = subprocess.run([exe, str(n), str(tmp_path / "a.bin"), str(tmp_path / "b.bin"), str(tmp_path / "out.bin")] + args,
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    with q.HipState(n) as sa, q.HipState(n) as sb:
        sa.upload(a)
        sb.upload(b)
        elements, inner = sa.pauli_matrix_elements(sb, strings), sa.inner(sb)
        sb.apply_pauli_sum(sa, strings, cs, accumulate=True)
        want = np.concatenate([sb.download(), elements, [inner]])
    got = np.fromfile(tmp_path / "out.bin", dtype=np.complex128)
    assert np.array_equal(_bits(got), _bits(want))
