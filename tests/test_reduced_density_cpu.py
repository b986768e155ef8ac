"""Reduced density matrices (include/qip_hipx.h), the parts that need no GPU: the tests' reference against the literal double loop
of the definition, von_neumann_entropy on matrices known by hand, and a null handle (there is no CPU fall-back)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import reduced_density_ref as D
import rustqip_amd as q
from rustqip_amd import _ffi, von_neumann_entropy


# ---- the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", D.DTYPES, ids=("c128", "c64"))
def test_reference_is_the_definition(dtype):
    """n <= 5, every subset with k <= 3 in ascending qubit order and in two scrambled orders: the reshaped longdouble sums against
    the amplitude-by-amplitude loop in complex128, whose rounding is at most 2^(n-k) u of the bar's scale"""
    worst = 0.0
    for n in range(1, 6):
        x = D.make_state(n, D.seed_of(n, dtype), dtype, norm=0.9)
        for k in range(1, min(3, n) + 1):
            for subset in itertools.combinations(range(n), k):
                orders = [list(subset), D.scrambled(subset, n + k), D.scrambled(subset, 31 * n + k)[::-1]]
                for indices in orders:
                    ref, lit = D.density_ref(n, indices, x), D.density_literal(n, indices, x)
                    d = np.sqrt(np.diag(ref).real)
                    scale = np.outer(d, d)
                    err = np.abs(ref - lit)
                    assert np.all(err <= 64 * 2.0 ** -53 * scale), (n, indices)
                    worst = max(worst, float(np.max(err / np.where(scale > 0, scale, 1.0))))
                    assert np.all(np.abs(ref - ref.conj().T) <= 4 * 2.0 ** -53 * scale)  # (numpy may fuse the products' sums)
                    assert np.array_equal(D.permuted(D.density_ref(n, list(subset), x), [list(subset).index(v) for v in indices]), ref)
    print(f"{np.dtype(dtype).name}: worst |ref - literal| = {worst:.3e} of the scale")


def test_bar_and_structure_helpers():
    ref = np.array([[0.5, 0.25j], [0.0, 0.125]])
    ref[1, 0] = np.conj(ref[0, 1])  # (the literal -0.25j has a real part of -0.0)
    assert D.worst_ratio(ref, ref) == 0.0
    off = ref.copy()
    off[0, 1] += 0.5 * D.BAR * 0.25
    assert 0.49 < D.worst_ratio(off, ref) < 0.51
    assert D.exact_structure(ref) and not D.exact_structure(off)
    signed = ref.copy()
    signed[1, 1] = complex(0.125, -0.0)
    assert not D.exact_structure(signed)  # a diagonal imaginary part of -0.0 is not +0.0
    zero_row = np.array([[0.5, 0.0], [0.0, 0.0]], dtype=np.complex128)
    leak = zero_row.copy()
    leak[0, 1] = 1e-300
    assert D.worst_ratio(zero_row, zero_row) == 0.0 and D.worst_ratio(leak, zero_row) == np.inf


# ---- the entropy helper ------------------------------------------------------------------------------------------------------------
def _ket(n, *indices):
    v = np.zeros(1 << n, dtype=np.complex128)
    v[list(indices)] = 1.0 / np.sqrt(len(indices))
    return v


def test_von_neumann_entropy():
    bell = _ket(2, 0b00, 0b11)
    for qubit in (0, 1):
        assert abs(von_neumann_entropy(D.density_ref(2, [qubit], bell)) - 1.0) <= 1e-14
    assert abs(von_neumann_entropy(D.density_ref(2, [0, 1], bell))) <= 1e-14
    ghz = _ket(5, 0, 31)
    for indices in ([0], [4, 1], [2, 3, 0], [0, 1, 2, 3]):
        assert abs(von_neumann_entropy(D.density_ref(5, indices, ghz)) - 1.0) <= 1e-14, indices
    product = np.kron(np.kron([0.6, 0.8j], [1.0, 0.0]), np.array([1.0, 1.0]) / np.sqrt(2.0))
    for indices in ([0], [1], [2], [0, 2], [2, 1]):
        assert abs(von_neumann_entropy(D.density_ref(3, indices, product))) <= 1e-14, indices
    # base e, and a raw (unnormalised) matrix: the trace is divided out
    half = D.density_ref(2, [0], bell)
    assert abs(von_neumann_entropy(half, base=np.e) - np.log(2.0)) <= 1e-14
    assert abs(von_neumann_entropy(0.37 * half) - 1.0) <= 1e-14
    assert abs(von_neumann_entropy(np.diag([0.5, 0.25, 0.25, 0.0])) - 1.5) <= 1e-14
    assert von_neumann_entropy(np.diag([1.0, -1e-17])) == 0.0  # a rounding-negative eigenvalue is clipped
    assert q.von_neumann_entropy is von_neumann_entropy
    for bad in (np.zeros((2, 3)), np.zeros((2, 2)), np.ones(4)):
        with pytest.raises(ValueError):
            von_neumann_entropy(bad)


# ---- no host fall-back ---------------------------------------------------------------------------------------------------------------
def test_null_handle_is_refused():
    out = (C.c_double * 8)(*([7.0] * 8))
    idx = (C.c_uint64 * 1)(0)
    assert _ffi.lib.qipx_state_reduced_density(None, idx, 1, out) == _ffi.QIP_ERR_INVALID
    assert _ffi.last_error() and list(out) == [7.0] * 8
    assert _ffi.lib.qipx_state_reduced_density(None, None, 0, None) == _ffi.QIP_ERR_INVALID
