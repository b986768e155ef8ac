"""Vector arithmetic and Krylov solvers of device states (include/qip_hipx.h), the parts that need no GPU: the references of
tests/krylov_ref.py against dense matrices, eigh and the exact propagator; the condition under which the GPU tests run (the numpy
restatement of the solvers, in the state's own precision, meets every bar with K / 8); K itself; the host-side tridiagonal code of
rustqip_amd.state; null handles of the two C calls (there is no CPU fall-back)."""
import ctypes as C
import math

import numpy as np
import pytest

import krylov_ref as R
import pauli_pair_ref as P
import rustqip_amd as q
from rustqip_amd import _ffi, state as S

_IDS = ("c128", "c64")
_CHECKS = {}


def _checks(dtype):
    """the solver checks of one precision: computed once, shared by the tests below"""
    if np.dtype(dtype) not in _CHECKS:
        _CHECKS[np.dtype(dtype)] = R.solver_checks(dtype)
    return _CHECKS[np.dtype(dtype)]


# ---- the references -------------------------------------------------------------------------------------------------------------
def test_dense_matrix_against_kronecker_products():
    n = 3
    pauli = {"I": np.eye(2), "X": np.array([[0, 1], [1, 0]]), "Y": np.array([[0, -1j], [1j, 0]]), "Z": np.diag([1, -1])}
    for name, make in R.HAMILTONIANS.items():
        terms, coeffs = make(n)
        want = np.zeros((8, 8), dtype=np.complex128)
        for term, c in zip(terms, coeffs):
            m = np.eye(1)
            for qb in range(n):  # qubit 0 is the top index bit: the leftmost factor
                m = np.kron(m, pauli[term.get(qb, "I")])
            want = want + c * m
        got = R.dense_matrix(n, terms, coeffs)
        assert np.array_equal(got, want), name
        assert np.array_equal(got, got.conj().T)
        psi = P.make_state(n, 5, np.complex128)
        assert np.max(np.abs(got @ psi - P.pauli_sum_ref(n, terms, coeffs, psi))) <= 1e-14


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_lincomb_spec_is_a_rounded_combination(dtype):
    """the specified arithmetic against the combination in complex128: per element within (count + 3) u sum_i |c_i| |s_i[j]|
    (rounding of c_i, three roundings per complex product, count - 1 additions)"""
    n, u = 7, R.unit_roundoff(dtype)
    rng = np.random.default_rng(12)
    for count in (1, 2, 3, 5, 16):
        srcs = [P.make_state(n, 40 + i, dtype, norm=0.7) for i in range(count)]
        cs = rng.standard_normal(count) + 1j * rng.standard_normal(count)
        got = R.lincomb_spec(srcs, cs, dtype)
        assert got.dtype == np.dtype(dtype)
        want = sum(c * s.astype(np.complex128) for c, s in zip(cs, srcs))
        scale = sum(abs(c) * np.abs(s.astype(np.complex128)) for c, s in zip(cs, srcs))
        assert np.all(np.abs(got.astype(np.complex128) - want) <= (count + 3) * u * scale), count
    x = P.make_state(n, 3, dtype)
    assert np.array_equal(R.lincomb_spec([x], [1.0], dtype), x)  # (1 x - 0 y and 1 y + 0 x are exact)
    assert abs(R.norm_exact(x) - float(np.linalg.norm(x.astype(np.complex128))) ** 2) <= 1e-14
    assert abs(R.inner_ref(x, x).real - R.norm_exact(x)) <= 1e-15 and R.inner_ref(x, x).imag == 0.0


# ---- the restated solvers: K and the condition of the GPU tests ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_restatement_meets_every_bar_with_an_eighth_of_k(dtype):
    """alphas / betas against the extended-precision run, Ritz values and energies against eigh, the evolved state against the
    exact propagator: every error at most (K / 8) m (T + 8) u S"""
    for what, err, unit in _checks(dtype):
        print(f"{np.dtype(dtype).name} {what}: error {err:.3e} = {err / unit:.4f} units, allowed {R.K / 8:.4f}")
    for what, err, unit in _checks(dtype):
        assert err <= R.K / 8 * unit, what


def test_k_is_eight_times_the_worst_ratio_rounded_up_to_a_power_of_two():
    worst = max(err / unit for dtype in R.DTYPES for _, err, unit in _checks(dtype))
    print(f"worst ratio {worst:.4f}, K = {R.K}")
    assert R.K == 2.0 ** math.ceil(math.log2(8 * worst))
    assert S.KRYLOV_K == R.K
    terms, coeffs = R.ising_chain(6)
    for dtype in R.DTYPES:
        assert q.krylov_bar(15, len(terms), float(np.sum(np.abs(coeffs))), dtype) == R.bar(15, terms, coeffs, dtype)


def test_breakdown_case_stops_early():
    name, n, m = R.BREAKDOWN_CASE
    lam, _, terms, coeffs = R.spectrum(name, n)
    for dtype in R.DTYPES:
        ar = R.Arith(n, terms, coeffs, dtype)
        a, b, _, _ = R.lanczos(ar, ar.load(R.start_state(n, dtype)), m, True, R.bar(m, terms, coeffs, dtype))
        assert len(a) == len(b) <= 8 and b[-1] <= R.bar(m, terms, coeffs, dtype)


# ---- the host-side tridiagonal code ---------------------------------------------------------------------------------------------
def test_tridiagonal_eigh_and_propagator_column():
    rng = np.random.default_rng(8)
    for k in (1, 2, 7, 15):
        a, b = rng.standard_normal(k), np.abs(rng.standard_normal(k)) + 0.1  # (betas as krylov_basis returns them: k of them)
        t = R.tridiagonal(a, b)
        assert t.shape == (k, k) and np.array_equal(t, t.T)
        theta, y = q.tridiagonal_eigh(a, b)
        assert np.all(np.diff(theta) >= 0)
        assert np.max(np.abs(t @ y - y * theta)) <= 1e-13 * max(1.0, float(np.max(np.abs(t))) * k)
        assert np.array_equal(q.tridiagonal_eigh(a, b[:k - 1])[0], theta)  # (the closing beta is not part of the matrix)
        tau = 0.37
        col = q.tridiagonal_propagator_column(a, b, tau)
        # exp(-i T tau) e_0 by the Taylor series in complex128 (|T tau| < 4: 60 terms are plenty)
        want, term = np.zeros(k, dtype=np.complex128), np.eye(k, dtype=np.complex128)[:, 0]
        for order in range(60):
            want = want + term
            term = (-1j * tau) * (t @ term) / (order + 1)
        assert col.dtype == np.complex128 and np.max(np.abs(col - want)) <= 1e-13
        assert abs(np.linalg.norm(col) - 1.0) <= 1e-14
        assert np.max(np.abs(q.tridiagonal_propagator_column(a, b, 0.0) - np.eye(k)[:, 0])) <= 1e-14
        assert np.max(np.abs(col - (y * np.exp(-1j * theta * tau)) @ y[0, :])) <= 1e-13  # (the eigendecomposition's column)
        # the restatement's column entry by entry RELATIVELY: the last entry, (|T| tau)^(k-1) / (k-1)! small, makes the estimate
        restated = R.propagator_column(a, b, tau)
        assert np.all(np.abs(col - restated) <= 1e-12 * np.abs(restated)), k
        for many in (3.0, -11.0):  # (several steps of the series)
            wide = q.tridiagonal_propagator_column(a, b, many)
            assert np.all(np.abs(wide - R.propagator_column(a, b, many)) <= 1e-11 * np.abs(R.propagator_column(a, b, many)) + 1e-300)
            assert np.max(np.abs(wide - (y * np.exp(-1j * theta * many)) @ y[0, :])) <= 1e-12
    with pytest.raises(ValueError):
        q.tridiagonal_eigh([], [])
    with pytest.raises(ValueError):
        q.tridiagonal_eigh([1.0, 2.0, 3.0], [0.5])


# ---- the C calls without a device -------------------------------------------------------------------------------------------------
def test_null_handles_are_refused():
    """no CPU fall-back: without a device there is no handle, and a null handle is refused whatever else is passed"""
    cs = (C.c_double * 4)(1.0, 0.0, 0.5, 0.0)
    out = (C.c_double * 4)()
    norm = C.c_double(7.0)
    handles = (C.c_void_p * 2)(None, None)
    for count in (0, 1, 2, 17):
        assert _ffi.lib.qipx_state_linear_combination(None, handles, cs, count, C.byref(norm)) == _ffi.QIP_ERR_INVALID
        assert "null state handle" in _ffi.last_error()
        assert _ffi.lib.qipx_state_linear_combination(None, None, None, count, None) == _ffi.QIP_ERR_INVALID
        assert _ffi.lib.qipx_state_inner_products(handles, count, None, out) == _ffi.QIP_ERR_INVALID
        assert "null state handle" in _ffi.last_error()
        assert _ffi.lib.qipx_state_inner_products(None, count, None, None) == _ffi.QIP_ERR_INVALID
    assert norm.value == 7.0 and list(out) == [0.0] * 4
