"""Vector arithmetic of device states (include/qip_hipx.h): dst <- sum_i c_i src_i (k_lincomb), <bra_i|ket> (k_inner_many), and
the solvers HipState builds on them with apply_pauli_sum: krylov_basis, ground_state, krylov_evolve.

The references and the bars are those of tests/krylov_ref.py:

    combination      the bytes of download() equal lincomb_spec (the arithmetic the header fixes, in numpy)
    its norm         |got - ref| <= 1e-12 ref, ref the exact sum of the stored squares
    inner product    |got - ref| <= 1e-12 |bra| |ket| (pauli_pair_ref.melem_bar), ref by math.fsum
    solvers          B = K m (T + 8) u S with the measured K of krylov_ref.py

Both kernels are grid-stride passes over 16-byte elements in a grid of max(elements / 1024, 1) blocks, at most 4096: n = 1, 2, 3 are
below one wave (n = 1 in Complex<f32> is one element), n = 9 one block, n = 13 several blocks, n = 22 more than one turn of the
loop per lane.  Every test prints its worst figure before it asserts."""
import ctypes as C
import math
import subprocess

from gpu_common import *  # noqa: F401,F403

import krylov_ref as R
import pauli_pair_ref as P
from rustqip_amd import _ffi

pytestmark = pytest.mark.gpu

_IDS = ("c128", "c64")
_STATES = {}
SIZES = (1, 2, 3, 9, 13, 22)


def _state(n, dtype, salt=0, norm=0.7):
    """the case state of (n, dtype, salt): shared, never written to"""
    key = (n, np.dtype(dtype), salt, norm)
    if key not in _STATES:
        x = R.make_state(n, R.seed_of(n, dtype) + 1000 * salt, dtype, norm=norm)
        x.setflags(write=False)
        _STATES[key] = x
    return _STATES[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _coeffs(count, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(count) + 1j * rng.standard_normal(count)


def _hold_norm(got, stored, what):
    ref = R.norm_exact(stored)
    print(f"{what}: norm {got!r}, exact {ref!r}, apart {abs(got - ref) / ref if ref else abs(got - ref):.3e} (bar {R.NORM_BAR:.0e})")
    assert abs(got - ref) <= R.NORM_BAR * ref, what


class _Pool:
    """`count` device states holding the case states of salts 0 .. count - 1, and a destination"""

    def __init__(self, n, dtype, count):
        self.n, self.dtype = n, dtype
        self.host = [_state(n, dtype, salt) for salt in range(count)]
        self.dev = [q.HipState(n, dtype) for _ in range(count)]
        self.dst = q.HipState(n, dtype)
        for st, x in zip(self.dev, self.host):
            st.upload(x)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for st in self.dev + [self.dst]:
            st.close()

    def unchanged(self, skip=()):
        return all(np.array_equal(_bits(st.download()), _bits(x)) for i, (st, x) in enumerate(zip(self.dev, self.host)) if i not in skip)


# ---- 1: the combination ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_combination_at_every_size(dtype, n):
    """three sources with complex coefficients (the Lanczos update's shape) and the norm, twice: the specified bits, the same bits
    and the same norm again, the sources as they were"""
    cs = _coeffs(3, 100 + n)
    with _Pool(n, dtype, 3) as p:
        want = R.lincomb_spec(p.host, cs, dtype)
        norm = p.dst.linear_combination(p.dev, cs, want_norm=True)
        got = p.dst.download()
        assert got.dtype == np.dtype(dtype) and np.array_equal(_bits(got), _bits(want)), f"n={n}: {int(np.sum(got != want))} amplitudes differ"
        _hold_norm(norm, want, f"n={n}")
        p.dst.init_basis(0)
        again = p.dst.linear_combination(p.dev, cs, want_norm=True)
        assert again == norm and np.array_equal(_bits(p.dst.download()), _bits(want))
        assert p.dst.linear_combination(p.dev, cs) is None and np.array_equal(_bits(p.dst.download()), _bits(want))
        assert p.unchanged()


@pytest.mark.parametrize("n", (13, 20))
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_combination_of_every_count(dtype, n):
    """1, 2, 3, 4, 5, 8 and 16 sources (every kernel capacity, and counts inside one), 6, 7 and 9 too; the norm on every other"""
    with _Pool(n, dtype, 16) as p:
        for i, count in enumerate((1, 2, 3, 4, 5, 6, 7, 8, 9, 16)):
            cs = _coeffs(count, 200 + count)
            want = R.lincomb_spec(p.host[:count], cs, dtype)
            norm = p.dst.linear_combination(p.dev[:count], cs, want_norm=bool(i % 2))
            got = p.dst.download()
            assert np.array_equal(_bits(got), _bits(want)), f"n={n} count={count}: {int(np.sum(got != want))} amplitudes differ"
            if i % 2:
                _hold_norm(norm, want, f"n={n} count={count}")
        assert p.unchanged()


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_destination_among_the_sources(dtype):
    """dst as the first, a middle and the last of five sources, a source listed twice, dst listed twice, and dst alone (scaling
    in place): every source is read at j before j is stored"""
    n = 13
    with _Pool(n, dtype, 5) as p:
        for at in (0, 2, 4):
            cs = _coeffs(5, 300 + at)
            want = R.lincomb_spec(p.host, cs, dtype)
            own = p.dev[at]
            norm = own.linear_combination(p.dev, cs, want_norm=True)
            assert np.array_equal(_bits(own.download()), _bits(want)), at
            _hold_norm(norm, want, f"dst = source {at}")
            assert p.unchanged(skip=(at,))
            own.upload(p.host[at])
        cs = _coeffs(4, 310)
        twice = [0, 3, 0, 1]
        p.dst.linear_combination([p.dev[i] for i in twice], cs)
        assert np.array_equal(_bits(p.dst.download()), _bits(R.lincomb_spec([p.host[i] for i in twice], cs, dtype)))
        p.dev[1].linear_combination([p.dev[1], p.dev[2], p.dev[1]], cs[:3])
        assert np.array_equal(_bits(p.dev[1].download()), _bits(R.lincomb_spec([p.host[1], p.host[2], p.host[1]], cs[:3], dtype)))
        p.dev[1].upload(p.host[1])
        p.dev[3].linear_combination([p.dev[3]], [cs[0]])
        assert np.array_equal(_bits(p.dev[3].download()), _bits(R.lincomb_spec([p.host[3]], [cs[0]], dtype)))
        assert p.unchanged(skip=(3,))


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_coefficients_get_no_special_case(dtype):
    """complex, purely real, purely imaginary, zero and minus zero, 1, and coefficients that round to a denormal of the state's
    precision (1e-42 in f32) or to zero (1e-50 in f32): the specified bits in every company"""
    n = 9
    tiny = 1e-42 if dtype == np.complex64 else 1e-310
    cases = [
        [0.3 - 1.2j, 2.0, -0.75j], [1.0, 0.0, -0.0], [0.0, 0.0, 0.0], [1.0, 1.0, -1.0], [tiny, 1j * tiny, 1.0],
        [1e-50, 0.5, tiny * (1 + 1j)], [complex(-0.0, 0.0), complex(0.0, -0.0), 1e150 if dtype == np.complex128 else 1e30],
    ]
    with _Pool(n, dtype, 3) as p:
        for cs in cases:
            want = R.lincomb_spec(p.host, cs, dtype)
            norm = p.dst.linear_combination(p.dev, cs, want_norm=True)
            got = p.dst.download()
            assert np.array_equal(_bits(got), _bits(want)), (cs, int(np.sum(_bits(got) != _bits(want))))
            _hold_norm(norm, want, f"coefficients {cs}")
        assert p.unchanged()


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_no_sources_is_zero(dtype):
    for n in (1, 9):
        with q.HipState(n, dtype) as dst:
            dst.upload(_state(n, dtype))
            assert dst.linear_combination([], [], want_norm=True) == 0.0
            assert not np.any(_bits(dst.download()))
            dst.upload(_state(n, dtype))
            assert dst.linear_combination([], []) is None and not np.any(_bits(dst.download()))


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_scale_axpy_normalize(dtype):
    n = 9
    x, y = _state(n, dtype), _state(n, dtype, 1)
    with q.HipState(n, dtype) as a, q.HipState(n, dtype) as b:
        a.upload(x)
        b.upload(y)
        a.scale(0.5 - 2j)
        want = R.lincomb_spec([x], [0.5 - 2j], dtype)
        assert np.array_equal(_bits(a.download()), _bits(want))
        a.axpy(-0.25j, b)
        want = R.lincomb_spec([want, y], [1.0, -0.25j], dtype)
        assert np.array_equal(_bits(a.download()), _bits(want))
        old = a.normalize()
        assert abs(old - math.sqrt(R.norm_exact(want))) <= 1e-12 * old
        assert np.array_equal(_bits(a.download()), _bits(R.lincomb_spec([want], [1.0 / old], dtype)))
        assert abs(a.inner_products([a])[0].real - 1.0) <= 8 * R.unit_roundoff(dtype)
        assert np.array_equal(_bits(b.download()), _bits(y))
        a.linear_combination([], [])
        with pytest.raises(q.CircuitError):
            a.normalize()


# ---- 2: inner products --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_inner_products_at_every_size(dtype, n):
    """four bras, the ket among them: each value within the bar, the batch bit-equal to its single calls, <ket|ket> with an
    imaginary part of exactly +0 (the header promises it), nothing changed"""
    with _Pool(n, dtype, 4) as p:
        ket, x = p.dev[3], p.host[3]
        got = ket.inner_products(p.dev)
        assert got.dtype == np.complex128 and got.shape == (4,)
        for i in range(4):
            ref, bar = R.inner_ref(p.host[i], x), R.inner_bar(p.host[i], x)
            print(f"n={n} bra {i}: |got - ref| = {abs(got[i] - ref):.3e}, bar {bar:.3e}")
            assert abs(got[i] - ref) <= bar, i
            single = ket.inner_products([p.dev[i]])
            assert np.array_equal(_bits(single), _bits(got[i:i + 1])), i
        assert got[3].imag == 0.0 and not np.signbit(got[3].imag)
        assert np.array_equal(_bits(ket.inner_products(p.dev)), _bits(got))
        assert p.unchanged()


@pytest.mark.parametrize("n", (13, 20))
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_inner_products_of_every_count(dtype, n):
    """1, 2, 4, 8 and 16 bras (every kernel capacity), 3, 5 and 9 too: one accumulation order whatever the count"""
    with _Pool(n, dtype, 16) as p:
        ket, x = p.dst, _state(n, dtype, 16)
        ket.upload(x)
        full = ket.inner_products(p.dev)
        for i in range(16):
            assert abs(full[i] - R.inner_ref(p.host[i], x)) <= R.inner_bar(p.host[i], x), i
        for count in (1, 2, 3, 4, 5, 8, 9):
            assert np.array_equal(_bits(ket.inner_products(p.dev[:count])), _bits(full[:count])), count
        assert np.array_equal(_bits(ket.inner_products(p.dev[::-1])), _bits(full[::-1]))
        assert ket.inner_products([]).shape == (0,)
        assert p.unchanged() and np.array_equal(_bits(ket.download()), _bits(x))


# ---- 3: refusals ------------------------------------------------------------------------------------------------------------------
def _raw_lincomb(dst, handles, coeffs, count, norm=None):
    arr = (C.c_void_p * max(len(handles), 1))(*handles) if handles is not None else None
    cs = (C.c_double * max(len(coeffs), 1))(*coeffs) if coeffs is not None else None
    return _ffi.lib.qipx_state_linear_combination(dst, arr, cs, count, norm)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_refusals_leave_the_destination_untouched(dtype):
    n = 9
    x = _state(n, dtype)
    other_dtype = np.complex64 if dtype == np.complex128 else np.complex128
    with _Pool(n, dtype, 2) as p, q.HipState(n + 1, dtype) as bigger, q.HipState(n, other_dtype) as other:
        p.dst.upload(x)
        h = [s._h.value for s in p.dev]
        norm = C.c_double(7.0)
        inv, uns = _ffi.QIP_ERR_INVALID, _ffi.QIP_ERR_UNSUPPORTED
        assert _raw_lincomb(p.dst._h, [h[0]] * 17, [1.0, 0.0] * 17, 17, C.byref(norm)) == uns and "17" in _ffi.last_error()
        assert _raw_lincomb(p.dst._h, [h[0], None], [1.0, 0.0] * 2, 2, C.byref(norm)) == inv and "null state handle" in _ffi.last_error()
        assert _raw_lincomb(p.dst._h, None, [1.0, 0.0], 1) == inv
        assert _raw_lincomb(p.dst._h, [h[0]], None, 1) == inv
        assert _raw_lincomb(p.dst._h, [h[0], bigger._h.value], [1.0, 0.0] * 2, 2) == inv and "size or precision" in _ffi.last_error()
        assert _raw_lincomb(p.dst._h, [other._h.value], [1.0, 0.0], 1) == inv and "size or precision" in _ffi.last_error()
        for bad, at in ((float("nan"), 1), (float("inf"), 2), (-float("inf"), 3)):
            cs = [1.0, 0.0, 0.5, 0.25]
            cs[at] = bad
            assert _raw_lincomb(p.dst._h, h, cs, 2, C.byref(norm)) == inv
            assert f"source {at // 2}" in _ffi.last_error() and "not finite" in _ffi.last_error()
        assert norm.value == 7.0
        out = (C.c_double * 40)()
        bras = lambda hs: (C.c_void_p * max(len(hs), 1))(*hs)  # noqa: E731
        assert _ffi.lib.qipx_state_inner_products(bras([h[0]] * 17), 17, p.dst._h, out) == uns
        assert _ffi.lib.qipx_state_inner_products(bras([h[0], None]), 2, p.dst._h, out) == inv
        assert _ffi.lib.qipx_state_inner_products(None, 1, p.dst._h, out) == inv
        assert _ffi.lib.qipx_state_inner_products(bras(h), 2, p.dst._h, None) == inv
        assert _ffi.lib.qipx_state_inner_products(bras([bigger._h.value]), 1, p.dst._h, out) == inv
        assert _ffi.lib.qipx_state_inner_products(bras([other._h.value]), 1, p.dst._h, out) == inv
        assert _ffi.lib.qipx_state_inner_products(None, 0, p.dst._h, None) == _ffi.QIP_OK
        assert list(out) == [0.0] * 40
        # the Python layer: its own checks raise CircuitError, the library's refusals QipHipError
        with pytest.raises(q.CircuitError):
            p.dst.linear_combination(p.dev, [1.0])
        with pytest.raises(q.CircuitError):
            p.dst.linear_combination([p.dev[0], bigger], [1.0, 1.0])
        with pytest.raises(q.CircuitError):
            p.dst.inner_products([other])
        with pytest.raises(q.CircuitError):
            p.dst.inner_products([x])
        with pytest.raises(q.QipHipError):
            p.dst.linear_combination([p.dev[0]] * 17, [1.0] * 17)
        with pytest.raises(q.CircuitError, match="source 1"):  # (QIP_ERR_INVALID)
            p.dst.linear_combination(p.dev, [1.0, float("nan")])
        assert np.array_equal(_bits(p.dst.download()), _bits(x)) and p.unchanged()


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_solver_arguments_are_checked_before_anything_is_queued(dtype):
    n = 6
    terms, coeffs = R.ising_chain(n)
    x, y = _state(n, dtype), _state(n, dtype, 1)
    with q.HipState(n, dtype) as psi, q.HipState(n, dtype) as b0, q.HipState(n, dtype) as b1, q.HipState(n + 1, dtype) as bigger:
        psi.upload(x)
        for b in (b0, b1):
            b.upload(y)
        bad = [
            (terms, coeffs * (1 + 0j), [b0, b1]), (terms, coeffs[:-1], [b0, b1]), (terms, np.where(np.arange(len(coeffs)) == 2, np.nan, coeffs), [b0, b1]),
            (terms, coeffs, [b0]), (terms, coeffs, [b0, b1] * 9), (terms, coeffs, [b0, psi]), (terms, coeffs, [b0, b0]), (terms, coeffs, [b0, bigger]),
            (terms, coeffs, [b0, x]), (terms[:-1] + [{n: "X"}], coeffs, [b0, b1]), (terms[:-1] + [{0: "Q"}], coeffs, [b0, b1]),
        ]
        for t, c, basis in bad:
            for call in (lambda: psi.krylov_basis(t, c, basis), lambda: psi.ground_state(t, c, basis), lambda: psi.krylov_evolve(t, c, 0.1, basis)):
                with pytest.raises((q.CircuitError, q.QipHipError)):
                    call()
        with pytest.raises(q.CircuitError):
            psi.ground_state(terms, coeffs, [b0, b1], restarts=0)
        with pytest.raises(q.CircuitError):
            psi.krylov_evolve(terms, coeffs, 0.1, [b0, b1], substeps=0)
        assert np.array_equal(_bits(psi.download()), _bits(x))
        assert all(np.array_equal(_bits(b.download()), _bits(y)) for b in (b0, b1))
        psi.linear_combination([], [])
        with pytest.raises(q.CircuitError):
            psi.krylov_basis(terms, coeffs, [b0, b1])  # (a zero state has no direction)


# ---- 4: the solvers -----------------------------------------------------------------------------------------------------------------
class _Basis:
    def __init__(self, n, dtype, m):
        self.states = [q.HipState(n, dtype) for _ in range(m + 1)]

    def __enter__(self):
        return self.states

    def __exit__(self, *exc):
        for st in self.states:
            st.close()


@pytest.mark.parametrize("name,n,m,reorth", R.BASIS_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_krylov_basis_against_the_restatement(dtype, name, n, m, reorth):
    """alphas and betas within B of the numpy restatement in the state's precision; the state unchanged; the basis orthonormal
    to B / S when reorthogonalised; basis[0] the normalised state bit for bit"""
    _, _, terms, coeffs = R.spectrum(name, n)
    bar = R.bar(m, terms, coeffs, dtype)
    x = R.start_state(n, dtype)
    ar = R.Arith(n, terms, coeffs, dtype)
    want_a, want_b, want_basis, _ = R.lanczos(ar, ar.load(x), m, reorth, bar)
    with q.HipState(n, dtype) as psi, _Basis(n, dtype, m) as basis:
        psi.upload(x)
        a, b = psi.krylov_basis(terms, coeffs, basis, reorthogonalize=reorth)
        assert a.shape == b.shape == (m,) and a.dtype == b.dtype == np.float64
        worst = float(max(np.max(np.abs(a - want_a)), np.max(np.abs(b - want_b))))
        print(f"{name} n={n} m={m} reorth={reorth}: worst |alpha, beta - restated| = {worst:.3e}, B = {bar:.3e}")
        assert worst <= bar
        assert np.array_equal(_bits(psi.download()), _bits(x))
        assert np.array_equal(_bits(basis[0].download()), _bits(want_basis[0]))
        if reorth:
            defect = R.basis_defect(lambda bra, ket: complex(ket.inner_products([bra])[0]), basis)
            print(f"  orthonormality of the first and the last vector: {defect:.3e}, B / S = {bar / R.weight(coeffs):.3e}")
            assert defect <= bar / R.weight(coeffs)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_krylov_basis_breaks_down_in_an_invariant_subspace(dtype):
    """n = 3 with room for 15 steps: the XXZ chain conserves the magnetisation, the steps end after at most 8, the last beta is at
    most B and the Ritz values are eigenvalues within B"""
    name, n, m = R.BREAKDOWN_CASE
    lam, _, terms, coeffs = R.spectrum(name, n)
    bar = R.bar(m, terms, coeffs, dtype)
    with q.HipState(n, dtype) as psi, _Basis(n, dtype, m) as basis:
        psi.upload(R.start_state(n, dtype))
        a, b = psi.krylov_basis(terms, coeffs, basis)
        assert len(a) == len(b) <= 8 and b[-1] <= bar
        worst = max(R.nearest(lam, th) for th in R.ritz_values(a, b))
        print(f"{len(a)} steps, last beta {b[-1]:.3e}, worst |ritz - eigenvalue| = {worst:.3e}, B = {bar:.3e}")
        assert worst <= bar


@pytest.mark.parametrize("name,n,m,restarts", R.GROUND_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_ground_state(dtype, name, n, m, restarts):
    lam, _, terms, coeffs = R.spectrum(name, n)
    bar = R.bar(m, terms, coeffs, dtype)
    with q.HipState(n, dtype) as psi, _Basis(n, dtype, m) as basis:
        psi.upload(R.start_state(n, dtype))
        first, first_residual = psi.ground_state(terms, coeffs, basis)  # one round
        print(f"{name}: one round: energy {first!r}, residual {first_residual:.3e}")
        assert R.nearest(lam, first) <= first_residual + bar
        energy, residual = psi.ground_state(terms, coeffs, basis, restarts=restarts)
        print(f"{name}: energy {energy!r}, lowest eigenvalue {lam[0]!r}, residual {residual:.3e}, B = {bar:.3e}")
        assert R.nearest(lam, energy) <= residual + bar
        assert residual <= bar, "the restatement converges on this input (tests/test_krylov_cpu.py)"
        assert abs(energy - lam[0]) <= bar
        assert abs(math.sqrt(psi.inner_products([psi])[0].real) - 1.0) <= bar
        assert abs(psi.expectation(terms, coeffs) - lam[0]) <= bar


@pytest.mark.parametrize("name,n,m,t,substeps", R.EVOLVE_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_krylov_evolve_against_the_exact_propagator(dtype, name, n, m, t, substeps):
    _, _, terms, coeffs = R.spectrum(name, n)
    bar = R.bar(m, terms, coeffs, dtype)
    x = R.start_state(n, dtype)
    norm = math.sqrt(R.norm_exact(x))
    _, want_estimate = R.krylov_evolve(R.Arith(n, terms, coeffs, dtype), x, t, m, substeps, bar)
    exact = R.propagate_exact(name, n, t, x)
    with q.HipState(n, dtype) as psi, _Basis(n, dtype, m) as basis:
        psi.upload(x)
        estimate = psi.krylov_evolve(terms, coeffs, t, basis, substeps=substeps)
        got = psi.download()
    err = float(np.linalg.norm(got.astype(np.complex128) - exact))
    drift = abs(math.sqrt(R.norm_exact(got)) - norm)
    print(f"{name} t={t}: |got - exact| = {err:.3e} (bar {bar * norm:.3e}), norm drift {drift:.3e} (bar {bar:.3e}), "
          f"estimate {estimate:.6e}, restated {want_estimate:.6e}")
    assert drift <= bar
    assert abs(estimate - want_estimate) <= 1e-6 * want_estimate
    assert err <= bar * norm


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_relabelled_states(dtype):
    """tile = 1 with tile_relabel = 3 at n = 15 (the setting of the Pauli-pair tests): apply_ops leaves the handles relabelled and
    either call restores the caller's order of all of them first; the results are those of settled twins, bit for bit"""
    n = 15
    ops = circuits.c2_random_circuit(n, 80, seed=41)
    xa, xb = _state(n, dtype), _state(n, dtype, 1)
    cs = _coeffs(2, 15)
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
        got = a.inner_products([b, a])
        assert swept(a) >= 1 and swept(b) >= 1, "a batch left no layout to restore"
        assert np.array_equal(_bits(got), _bits(ta.inner_products([tb, ta])))
        relabel()
        norm = b.linear_combination([a, b], cs, want_norm=True)
        assert swept(a) >= 1 and swept(b) >= 1, "a batch left no layout to restore"
        assert norm == tb.linear_combination([ta, tb], cs, want_norm=True)
        assert b.max_abs_diff(tb) == (0.0, 0) and a.max_abs_diff(ta) == (0.0, 0)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_ordered_after_the_sources_and_complete_on_return(dtype):
    """apply_ops queued on a source with no synchronise, the combination, and at once another apply_ops on the source: the
    destination holds what a run with explicit synchronises leaves, bit for bit"""
    n = 12
    layer = circuits.h_layer(n)
    cs = _coeffs(2, 12)
    with q.HipState(n, dtype) as src, q.HipState(n, dtype) as dst, q.HipState(n, dtype) as twin:
        def run(sync):
            src.init_basis(5)
            dst.init_basis(9)
            src.apply_ops(layer)
            if sync:
                src.sync()
            dst.linear_combination([src, dst], cs)
            src.apply_ops(layer)  # the combination has read the source already
            if sync:
                src.sync()
            return dst.download()

        want = run(True)
        twin.upload(want)
        got = run(False)
        assert np.array_equal(_bits(got), _bits(want))


# ---- 5: the C++ mirror ----------------------------------------------------------------------------------------------------------------
def test_cpp_mirror(tmp_path):
    n = 10
    states = [_state(n, np.complex128, salt) for salt in range(3)]
    cs = _coeffs(3, 14)
    exe = str(tmp_path / "test_krylov_mirror")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "rustqip_amd", "host"), os.path.join(ROOT, "tests", "cpp", "test_krylov_mirror.cpp"),
                    "-o", exe, "-L" + os.path.join(ROOT, "rustqip_amd", "lib"), "-lqip_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "rustqip_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib",
                    "-Wl,-rpath-link,/opt/rocm/lib"], check=True, capture_output=True)
    paths = []
    for name, x in zip("abc", states):
        paths.append(str(tmp_path / f"{name}.bin"))
        x.tofile(paths[-1])
    args = [v for c in cs for v in (float(c.real).hex(), float(c.imag).hex())]
    res = subprocess.run([exe, str(n)] + paths + [str(tmp_path / "out.bin")] + args, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    with _Pool(n, np.complex128, 3) as p:
        norm = p.dst.linear_combination(p.dev, cs, want_norm=True)
        combined = p.dst.download()
        inner = p.dev[2].inner_products(p.dev)
        p.dev[1].linear_combination([p.dev[1], p.dev[0]], [cs[1], cs[0]])
        want = np.concatenate([combined, [norm], inner, p.dev[1].download()])
    got = np.fromfile(tmp_path / "out.bin", dtype=np.complex128)
    assert np.array_equal(_bits(got), _bits(want))
