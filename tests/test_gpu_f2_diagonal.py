"""Diagonal Pauli sums of any size in one pass on a device state (include/qip_hipx.h: qipx_state_apply_diagonal,
qipx_state_expect_diagonal; HipState.apply_diagonal / expect_diagonal / qaoa_layers): k_diag_phase and k_diag_moments
(rustqip_amd/csrc/qip_diag_kernels.h) — the short tile of n < 12, one full tile, several tiles per block, plain and packed
Complex<f32> elements, the term table's upload between unsynchronised calls.

The reference and the bars are those of tests/diagonal_ref.py, with u = 2^-53 (Complex<f64>) or 2^-24 (Complex<f32>), T terms,
L = 12, A = sum |gamma c_t|, A1 = sum |c_t| and c(n) the chain length the header states:

    phase, element by element:   |got_j - ref_j| <= [12 u + (T + L + 8) 2^-53 A] |psi_j|
    moments:                     |m1 - ref| <= (T + L + c(n) + 6) 2^-53 A1 |psi|^2,   |m2 - ref| <= (2 (T + L) + c(n) + 10) 2^-53 A1^2 |psi|^2

Every test prints its worst figure before it asserts."""
import ctypes as C
import subprocess

from gpu_common import *  # noqa: F401,F403

import diagonal_ref as D
import pauli_rotation_ref as P
from rustqip_amd import _ffi

pytestmark = pytest.mark.gpu

_IDS = ("c128", "c64")
_STATES = {}


def _state(n, dtype, norm=1.0):
    """the case state of (n, dtype, norm): shared, never written to (no amplitude is -0)"""
    key = (n, np.dtype(dtype), norm)
    if key not in _STATES:
        x = P.make_state(n, P.seed_of(n, dtype), dtype, norm=norm)
        x.setflags(write=False)
        _STATES[key] = x
    return _STATES[key]


def _terms(n, zs):
    return [D.z_term(n, z) for z in zs]


def _phased(st, x, terms, coeffs, gamma):
    st.upload(x)
    st.apply_diagonal(terms, coeffs, gamma)
    return st.download()


def _hold_phase(n, zs, cs, gamma, got, x, what):
    weight = abs(gamma) * float(np.sum(np.abs(cs)))
    ok, worst = D.within_phase_bar(n, len(zs), weight, got, D.phase_ref(n, zs, cs, gamma, x), x)
    print(f"{what} gamma={gamma}: worst |got - ref| = {worst:.4f} of the bar (T = {len(zs)}, A = {weight:.3g})")
    assert ok, what
    return worst


def _hold_moments(n, zs, cs, got, x, what):
    r1, r2 = D.moments_ref(n, zs, cs, x)
    b1, b2 = D.moment_bars(n, len(zs), float(np.sum(np.abs(cs))), x)
    print(f"{what}: |m1 - ref| = {abs(got[0] - r1):.3e} (bar {b1:.3e}), |m2 - ref| = {abs(got[1] - r2):.3e} (bar {b2:.3e})")
    assert abs(got[0] - r1) <= b1 and abs(got[1] - r2) <= b2, what


def _hold_case(st, n, zs, cs, x, what, gammas=(0.7, -1.9)):
    terms = _terms(n, zs)
    for gamma in gammas:
        _hold_phase(n, zs, cs, gamma, _phased(st, x, terms, cs, gamma), x, what)
    st.upload(x)
    _hold_moments(n, zs, cs, st.expect_diagonal(terms, cs), x, what)
    assert np.array_equal(st.download().view(np.uint8), x.view(np.uint8)), what  # expect leaves the state as it is


# ---- 1: every n across the tile boundary --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(1, 16))
@pytest.mark.parametrize("dtype", D.DTYPES, ids=_IDS)
def test_every_n(dtype, n):
    """n = 1 .. 15: the short tile, exactly one tile, two, four, eight.  T = 1 (each single Z, ZZ across the boundary and across
    the halves of a packed element, the all-Z string), the empty term alone, and 40 random terms; gamma = 0 changes no bit"""
    x = _state(n, dtype, 0.8)
    with q.HipState(n, dtype) as st:
        for name, zs, cs in D.single_cases(n):
            _hold_case(st, n, zs, cs, x, f"n={n} {name}")
        zs, cs = D.random_case(n, 40, 500 + n)
        _hold_case(st, n, zs, cs, x, f"n={n} random40")
        assert np.array_equal(_phased(st, x, _terms(n, zs), cs, 0.0).view(np.uint8), x.view(np.uint8))


# ---- 2: many terms ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", D.DTYPES, ids=_IDS)
def test_many_terms(dtype):
    """n = 14, T = 5000: more distinct low masks than a block has lanes, repeated masks, one group of 600 terms that share a low
    mask; a list confined to the bits above the tile boundary (every term lands in a[0]) and one confined to the bits below"""
    n = 14
    x = _state(n, dtype)
    zs, cs = D.random_case(n, 5000, 77)
    rng = np.random.default_rng(78)
    for i in rng.choice(5000, 600, replace=False):
        zs[int(i)] = (zs[int(i)] & ~0xFFF) | 0x5A5
    assert len({z & 0xFFF for z in zs}) > 256 and len(set(zs)) < len(zs)
    assert sum(1 for z in zs if (z & 0xFFF) == 0x5A5) >= 600
    with q.HipState(n, dtype) as st:
        _hold_case(st, n, zs, cs, x, "n=14 T=5000", gammas=(0.7,))
        hz, hc = D.random_case(n, 200, 79, high=D.TILE_BITS)
        assert all(z & 0xFFF == 0 for z in hz)
        _hold_case(st, n, hz, hc, x, "n=14 high bits only", gammas=(-1.9,))
        lz, lc = D.random_case(n, 300, 80, low=D.TILE_BITS)
        _hold_case(st, n, lz, lc, x, "n=14 low bits only", gammas=(0.7,))


# ---- 3: large angles ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", D.DTYPES, ids=_IDS)
def test_large_angles(dtype):
    """coefficients of magnitude ~100, T = 300: |gamma D| up to ~10^4, carried by the bar's A term alone (the sine and cosine are
    double-precision evaluations of a double-precision angle for Complex<f32> too: a single-precision sine would miss the bar)"""
    n = 13
    x = _state(n, dtype)
    zs, cs = D.random_case(n, 300, 81, scale=100.0)
    big = float(np.max(np.abs(D.energies_ref(n, zs, cs))))
    print(f"largest |D| = {big:.1f}")
    assert big > 2000
    with q.HipState(n, dtype) as st:
        _hold_case(st, n, zs, cs, x, "n=13 large angles", gammas=(1.9,))


# ---- 4: many blocks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", D.DTYPES, ids=_IDS)
def test_many_blocks(dtype):
    """n = 22: 1024 tiles, one per block, the full-tile streaming path"""
    n = 22
    x = _state(n, dtype)
    zs, cs = D.random_case(n, 40, 82)
    with q.HipState(n, dtype) as st:
        _hold_case(st, n, zs, cs, x, "n=22", gammas=(0.7,))


# ---- 4b: several tiles per block ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,n", ((np.complex128, 25), (np.complex64, 26)), ids=_IDS)
def test_several_tiles_per_block(dtype, n):
    """n = 25 and 26: 2^13 and 2^14 tiles on 4096 blocks, two and four tiles per block — the table rebuilt for the block's next
    tile, the lane sums of the moments carried across tiles.  Held on the device to the existing calls on the same terms (the
    largest size of any case: nothing but four doubles crosses to the host).  The state is H on every qubit of |5> followed by
    a first diagonal phase: every amplitude has modulus 2^(-n/2) (to n roundings), its phase differs from tile to tile.
        apply_diagonal vs apply_pauli_rotations, max_abs_diff:  [12 u + (T + L + 8) 2^-53 A] |psi_j|  +  T * 24 u |psi_j|
            (the rotation tests' element bar 12 u (|psi_j| + |psi_jx|) with x = 0, once per term; moduli are kept)
        expect_diagonal vs expect_pauli: the moment bars + expect_pauli's documented 1e-12 |psi|^2 per term"""
    geometry_tiles = (1 << (n - D.TILE_BITS)) // 4096
    assert geometry_tiles >= 2
    u = D.unit_roundoff(dtype)
    zs, cs = D.random_case(n, 9, 91 + n)
    zs[0] = (1 << (n - 1)) | (1 << D.TILE_BITS) | 1  # the top bit (differs between blocks), the first bit above the tile (between
    zs[1] = 1 << D.TILE_BITS                         # the tiles of one block), bit 0
    terms = _terms(n, zs)
    a1 = float(np.sum(np.abs(cs)))
    gamma = 0.7
    modulus = 2.0 ** (-n / 2) * (1 + 1e-5)  # (n roundings of the H layer: below 26 * 2^-24)
    with q.HipState(n, dtype) as st, q.HipState(n, dtype) as twin:
        st.init_basis(5)
        st.apply_ops(circuits.h_layer(n))
        st.apply_diagonal(terms[::-1], cs, 0.4)
        twin.copy_from(st)
        norm = st.norm_sqr()
        m1, m2 = st.expect_diagonal(terms, cs)
        singles = st.expect_pauli(terms)
        pairs = st.expect_pauli([D.z_term(n, a ^ b) for a in zs for b in zs])
        st.apply_diagonal(terms, cs, gamma)
        twin.apply_pauli_rotations(terms, gamma * cs)
        worst, differ = st.max_abs_diff(twin)
        norm_after = st.norm_sqr()
    bar = (D.BAR * u + (len(zs) + D.TILE_BITS + 8) * 2.0 ** -53 * abs(gamma) * a1 + len(zs) * 24 * u) * modulus
    print(f"n={n}, {geometry_tiles} tiles per block: max |apply_diagonal - rotations| = {worst:.3e} ({differ} amplitudes differ), bar {bar:.3e}")
    assert worst <= bar
    b1, b2 = D.moment_bars(n, len(zs), a1, norm=norm)
    d1 = abs(m1 - float(np.dot(cs, singles)))
    d2 = abs(m2 - float(np.dot(np.outer(cs, cs).ravel(), pairs)))
    print(f"m1 vs expect_pauli: {d1:.3e} (bar {b1 + 1e-12 * a1 * norm:.3e}); m2 vs pairwise products: {d2:.3e} (bar {b2 + 1e-12 * a1 * a1 * norm:.3e})")
    assert d1 <= b1 + 1e-12 * a1 * norm and d2 <= b2 + 1e-12 * a1 * a1 * norm
    assert abs(m1) > 1e3 * (b1 + 1e-12 * a1 * norm) or abs(m2) > 1e3 * (b2 + 1e-12 * a1 * a1 * norm)  # (the comparison is not of zeros)
    assert abs(norm_after - norm) <= 2 * D.BAR * u * norm


# ---- 5: against the existing calls --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", D.DTYPES, ids=_IDS)
def test_against_the_existing_calls(dtype):
    n, gamma = 13, 0.7
    x = _state(n, dtype, 0.5)
    u = D.unit_roundoff(dtype)
    zs, cs = D.random_case(n, 12, 83)
    terms = _terms(n, zs)
    a1 = float(np.sum(np.abs(cs)))
    norm = float(np.sum(np.abs(x.astype(np.complex128)) ** 2))
    with q.HipState(n, dtype) as st:
        got = _phased(st, x, terms, cs, gamma)
        norm_after = st.norm_sqr()
        st.upload(x)
        norm_before = st.norm_sqr()
        m1, m2 = st.expect_diagonal(terms, cs)
        singles = st.expect_pauli(terms)
        pairs = st.expect_pauli([D.z_term(n, a ^ b) for a in zs for b in zs])
        st.apply_pauli_rotations(terms, gamma * cs)
        want = st.download()
    err = np.abs(got.astype(np.complex128) - want.astype(np.complex128))
    bar = D.phase_bar(n, len(zs), abs(gamma) * a1, x) + P.sequence_bar(len(zs), x)
    print(f"apply_diagonal vs apply_pauli_rotations: worst {float(np.max(err / bar)):.4f} of the two bars")
    assert np.all(err <= bar)
    b1, b2 = D.moment_bars(n, len(zs), a1, x)
    d1 = abs(m1 - float(np.dot(cs, singles)))
    d2 = abs(m2 - float(np.dot(np.outer(cs, cs).ravel(), pairs)))
    print(f"m1 vs expect_pauli: {d1:.3e} (bar {b1 + 1e-12 * a1 * norm:.3e}); m2 vs pairwise products: {d2:.3e} (bar {b2 + 1e-12 * a1 * a1 * norm:.3e})")
    assert d1 <= b1 + 1e-12 * a1 * norm  # (expect_pauli's documented 1e-12 norm^2 per term)
    assert d2 <= b2 + 1e-12 * a1 * a1 * norm
    print(f"norm_sqr: {abs(norm_after - norm_before):.3e}, bar {2 * D.BAR * u * norm_before:.3e}")
    assert abs(norm_after - norm_before) <= 2 * D.BAR * u * norm_before


# ---- 6: a relabelled state ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", D.DTYPES, ids=_IDS)
def test_relabelled_state(dtype):
    """tile = 1 with tile_relabel = 3 at n = 15 (the rotation tests' recipe): the batch leaves the qubits relabelled and both calls
    restore the caller's order first"""
    n = 15
    ops = circuits.c2_random_circuit(n, 80, seed=41)
    x = _state(n, dtype)
    zs, cs = D.random_case(n, 30, 84)
    terms = _terms(n, zs)
    with q.HipState(n, dtype) as st, q.HipState(n, dtype) as twin:
        st.set_option("tile", 1)
        st.set_option("tile_relabel", 3)
        st.set_option("profile", 1)
        st.upload(x)
        st.apply_ops(ops)
        twin.copy_from(st)  # (settles: a copy in the caller's order)
        y = twin.download()
        st.upload(x)
        st.apply_ops(ops)
        st.profile_reset()
        st.apply_diagonal(terms, cs, 0.7)
        assert st.profile().get("k_permute_bits", {}).get("launches", 0) >= 1, "the batch left no layout to restore"
        got = st.download()
        twin.apply_diagonal(terms, cs, 0.7)
        assert st.max_abs_diff(twin) == (0.0, 0)
        st.upload(x)
        st.apply_ops(ops)
        moments = st.expect_diagonal(terms, cs)
        twin.upload(y)
        assert moments == twin.expect_diagonal(terms, cs)
    _hold_phase(n, zs, cs, 0.7, got, y, "n=15 relabelled")
    _hold_moments(n, zs, cs, moments, y, "n=15 relabelled")


# ---- 7: stream order ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", D.DTYPES, ids=_IDS)
def test_queued_between_batches_without_a_synchronise(dtype):
    """apply_ops, apply_diagonal(A), apply_diagonal(B), apply_ops with nothing in between: the second call rewrites the term table
    (and its pinned host copy) while the first may still be queued.  A and B differ in length, and B outgrows A's buffer."""
    n = 13
    layer = circuits.h_layer(n)
    za, ca = D.random_case(n, 7, 85)
    zb, cb = D.random_case(n, 6000, 86)
    ta, tb = _terms(n, za), _terms(n, zb)
    with q.HipState(n, dtype) as st, q.HipState(n, dtype) as twin:
        st.init_basis(5)
        st.apply_ops(layer)
        st.apply_diagonal(ta, ca, 0.7)  # no synchronise in between
        st.apply_diagonal(tb, cb, -0.3)
        st.apply_diagonal(ta, ca, 0.2)
        st.apply_ops(layer)
        got = st.download()
        twin.init_basis(5)
        twin.apply_ops(layer)
        twin.download()  # (a download waits for the stream)
        twin.apply_diagonal(ta, ca, 0.7)
        y = twin.download()
        twin.apply_diagonal(tb, cb, -0.3)
        mid = twin.download()
        twin.apply_diagonal(ta, ca, 0.2)
        twin.download()
        twin.apply_ops(layer)
        want = twin.download()
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    _hold_phase(n, zb, cb, -0.3, mid, y, "B after A")


# ---- 8: determinism -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", D.DTYPES, ids=_IDS)
def test_same_call_same_bits(dtype):
    n = 14
    x = _state(n, dtype)
    zs, cs = D.random_case(n, 900, 87)
    terms = _terms(n, zs)
    with q.HipState(n, dtype) as st:
        a = _phased(st, x, terms, cs, 0.7)
        b = _phased(st, x, terms, cs, 0.7)
        st.upload(x)
        ma, mb = st.expect_diagonal(terms, cs), st.expect_diagonal(terms, cs)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert np.array([ma]).tobytes() == np.array([mb]).tobytes()


# ---- 9: both element packings of Complex<f32> ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (9, 13))
def test_packed_and_plain_f32_elements(n):
    """option "packed_f32" = 1 (the default) and 0.  The option, and with it the plain 8-byte Complex<f32> walk of both kernels,
    exists in a tuning build only (the product build compiles neither): there the two packings leave the same bits — the
    energy does not depend on the packing — and each meets the element bar; the product build checks the default alone"""
    x = _state(n, np.complex64)
    zs, cs = D.random_case(n, 40, 88 + n)
    terms = _terms(n, zs)
    results = {}
    for options in variants({}, {"packed_f32": 0}):
        with q.HipState(n, np.complex64) as st:
            for key, value in options.items():
                st.set_option(key, value)
            got = _phased(st, x, terms, cs, 0.7)
            st.upload(x)
            results[tuple(options)] = (got, st.expect_diagonal(terms, cs))
        _hold_phase(n, zs, cs, 0.7, got, x, f"n={n} {options or 'default'}")
        _hold_moments(n, zs, cs, results[tuple(options)][1], x, f"n={n} {options or 'default'}")
    first = results[()]
    for got, _ in results.values():
        assert np.array_equal(got.view(np.uint8), first[0].view(np.uint8)), \
            "the packing changed the bits"  # (the product build has the packed walk alone: one result, nothing to compare)
    assert len(results) == (2 if tuning() else 1), "packed_f32 = 0 runs in a tuning build and only there"


# ---- 10: refusals -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", D.DTYPES, ids=_IDS)
def test_refusals(dtype):
    n = 5
    x = _state(n, dtype)
    u64, u8, dbl = lambda v: (C.c_uint64 * len(v))(*v), lambda v: (C.c_uint8 * len(v))(*v), lambda v: (C.c_double * len(v))(*v)
    good = (u64([0, 2, 3]), u64([0, 3, 1]), u8([3, 3, 3]), dbl([0.4, -1.2]))  # Z0 Z3, Z1
    out = (C.c_double * 2)()
    apply = lambda *a: _ffi.lib.qipx_state_apply_diagonal(st._h, *a, 0.7)  # noqa: E731
    expect = lambda *a: _ffi.lib.qipx_state_expect_diagonal(st._h, *a, out)  # noqa: E731
    with q.HipState(n, dtype) as st:
        st.upload(x)

        def refused(rc, code=_ffi.QIP_ERR_INVALID):
            assert rc == code and _ffi.last_error()
            message = _ffi.last_error()
            assert np.array_equal(st.download().view(np.uint8), x.view(np.uint8))
            return message

        for call in (apply, expect):
            for null in range(4):
                args = list(good)
                args[null] = None
                refused(call(*args, 2))
            for bad in (float("nan"), float("inf"), -float("inf")):
                assert "term 1" in refused(call(good[0], good[1], good[2], dbl([0.4, bad]), 2))
            for code in (1, 2):  # an X and a Y factor in the last term
                message = refused(call(good[0], good[1], u8([3, 3, code]), good[3], 2))
                assert "term 1 is not diagonal" in message
            refused(call(good[0], u64([3, 3, 1]), good[2], good[3], 2))  # repeated inside a term
            refused(call(good[0], good[1], u8([3, 4, 3]), good[3], 2))   # code 4
            refused(call(good[0], u64([0, n, 1]), good[2], good[3], 2))  # qubit = n
            refused(call(u64([0, 2, 1]), good[1], good[2], good[3], 2))  # decreasing
            refused(call(u64([1, 2, 3]), good[1], good[2], good[3], 2))  # term_start[0] != 0
            refused(call(good[0], good[1], good[2], good[3], D.MAX_TERMS + 1), _ffi.QIP_ERR_UNSUPPORTED)  # (refused before any array is read)
        refused(_ffi.lib.qipx_state_expect_diagonal(st._h, *good, 2, None))  # null moments
        for bad in (float("nan"), float("inf")):
            refused(_ffi.lib.qipx_state_apply_diagonal(st._h, *good, 2, bad))  # gamma
        assert "term 0" in refused(_ffi.lib.qipx_state_apply_diagonal(st._h, good[0], good[1], good[2], dbl([1e200, 1.0]), 2, 1e200))
        for bad in ([{n: "Z"}], ["ZZ"], [{0: "W"}]):
            with pytest.raises(q.CircuitError):
                st.apply_diagonal(bad, [0.1])
        with pytest.raises(q.CircuitError):
            st.expect_diagonal(["ZIIII", "IZIII"], [1.0])
        with pytest.raises(q.CircuitError, match="term 0 is not diagonal"):
            st.apply_diagonal(["XIIII"], [1.0])
        # no terms: nothing to do, null arrays allowed
        assert _ffi.lib.qipx_state_apply_diagonal(st._h, None, None, None, None, 0, 0.7) == _ffi.QIP_OK
        out[0] = out[1] = 5.0
        assert _ffi.lib.qipx_state_expect_diagonal(st._h, None, None, None, None, 0, out) == _ffi.QIP_OK
        assert (out[0], out[1]) == (0.0, 0.0) and st.expect_diagonal([], []) == (0.0, 0.0)
        st.apply_diagonal([], [])
        assert np.array_equal(st.download().view(np.uint8), x.view(np.uint8))
        # and both still work
        assert expect(*good, 2) == _ffi.QIP_OK
        moments = (out[0], out[1])
        assert apply(*good, 2) == _ffi.QIP_OK
        got = st.download()
    zs = [D.z_of(n, {0: "Z", 3: "Z"}), D.z_of(n, {1: "Z"})]
    _hold_phase(n, zs, [0.4, -1.2], 0.7, got, x, "after the refusals")
    _hold_moments(n, zs, [0.4, -1.2], moments, x, "after the refusals")


# ---- 11: the mirrors ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", D.DTYPES, ids=_IDS)
def test_qaoa_layers(dtype):
    """ring + fields at n = 10, three layers: the explicit call sequence bit for bit, and the rotations path within the bars"""
    n = 10
    x = _state(n, dtype)
    terms = [{a: "Z", (a + 1) % n: "Z"} for a in range(n)] + [{a: "Z"} for a in range(n)]
    rng = np.random.default_rng(89)
    cs = rng.standard_normal(len(terms))
    gammas, betas = [0.7, -0.4, 1.1], [0.3, 0.9, -0.6]
    mixer = lambda b: [q.make_matrix_op([a], [np.cos(b), -1j * np.sin(b), -1j * np.sin(b), np.cos(b)]) for a in range(n)]  # noqa: E731
    with q.HipState(n, dtype) as st:
        st.upload(x)
        st.qaoa_layers(terms, cs, gammas, betas)
        got = st.download()
        st.upload(x)
        for g, b in zip(gammas, betas):
            st.apply_diagonal(terms, cs, g)
            st.apply_ops(mixer(b))
        explicit = st.download()
        st.upload(x)
        for g, b in zip(gammas, betas):
            st.apply_pauli_rotations(terms, g * cs)
            st.apply_ops(mixer(b))
        rotations = st.download()
        with pytest.raises(q.CircuitError):
            st.qaoa_layers(terms, cs, gammas, betas[:-1])
    assert np.array_equal(got.view(np.uint8), explicit.view(np.uint8))
    # every step is unitary: the 2-norm of the difference stays within the sum of the steps' bars (a mixer layer is n dense ops)
    u = D.unit_roundoff(dtype)
    norm = float(np.linalg.norm(x.astype(np.complex128)))
    tol = TOL64 if dtype == np.complex128 else TOL32
    bar = sum((D.BAR * u + (len(terms) + D.TILE_BITS + 8) * 2.0 ** -53 * abs(g) * float(np.sum(np.abs(cs)))) * norm
              + P.sequence_bar(len(terms), x) + 2 * n * tol * norm for g in gammas)
    d = float(np.linalg.norm(got.astype(np.complex128) - rotations.astype(np.complex128)))
    print(f"qaoa_layers vs rotations + RX: |difference|_2 = {d:.3e}, bar {bar:.3e}")
    assert d <= bar


def test_cpp_mirror(tmp_path):
    n = 10
    x = _state(n, np.complex128)
    rng = np.random.default_rng(90)
    strings = ["".join(rng.choice(list("IZ"), n)) for _ in range(14)] + ["I" * n, "Z" * n]
    coeffs = rng.standard_normal(len(strings))
    gamma = 0.7
    exe = str(tmp_path / "test_diag_mirror")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "rustqip_amd", "host"), os.path.join(ROOT, "tests", "cpp", "test_diag_mirror.cpp"),
                    "-o", exe, "-L" + os.path.join(ROOT, "rustqip_amd", "lib"), "-lqip_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "rustqip_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib",
                    "-Wl,-rpath-link,/opt/rocm/lib"], check=True, capture_output=True)
    x.tofile(tmp_path / "state.bin")
    args = [a for s, c in zip(strings, coeffs) for a in (s, float(c).hex())]
    res = subprocess.run([exe, str(n), str(tmp_path / "state.bin"), str(tmp_path / "out.bin"), float(gamma).hex()] + args,
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    with q.HipState(n) as st:
        st.upload(x)
        m1, m2 = st.expect_diagonal(strings, coeffs)
        st.apply_diagonal(strings, coeffs, gamma)
        want = st.download()
    got = np.fromfile(tmp_path / "out.bin", dtype=np.complex128)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    assert [float(v) for v in res.stdout.split()] == [m1, m2], res.stdout  # (17 significant digits: the doubles themselves)
