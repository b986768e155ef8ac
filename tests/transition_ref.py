"""An exact reference for the reduced transition matrix of a few qubits of two states and its bar — shared by
tests/test_circuit_gradient_cpu.py and tests/test_gpu_f2_transition.py.  A plain helper module: numpy only.

With the amplitudes of either state seen as a 2^k x 2^(n-k) matrix (tests/reduced_density_ref.py, psi_matrix: row a, bit i of a
the bit of qubit indices[i]; column b the other bits), M[a][a'] = sum_b ket[a,b] conj(bra[a',b]), raw.  The amplitudes are
widened to complex128, the products are formed in complex128 and summed over b in longdouble.

The bar is the reduced-density bar with Cauchy-Schwarz over two different rows: the absolute sum of an entry's products is at
most sqrt(rho_ket[a][a] rho_bra[a'][a']), rho_x[a][a] = sum_b |x[a,b]|^2, and |got - ref| <= 1e-12 times that."""
import numpy as np

from reduced_density_ref import (DTYPES, few_column_sets, make_state, ordered_subsets, position_sets, psi_matrix, qubits,  # noqa: F401
                                 scrambled, seed_of)

BAR = 1e-12


def transition_ref(n, indices, bra, ket):
    """complex128[2^k, 2^k]: M of the qubits `indices`"""
    x, y = psi_matrix(n, indices, ket), psi_matrix(n, indices, bra)
    m = x.shape[0]
    out = np.empty((m, m), dtype=np.complex128)
    for a in range(m):
        prod = x[a][None, :] * np.conj(y)  # complex128 products, row a of ket against every row a' of bra
        out[a] = (np.sum(prod.real, axis=1, dtype=np.longdouble).astype(np.float64)
                  + 1j * np.sum(prod.imag, axis=1, dtype=np.longdouble).astype(np.float64))
    return out


def row_weights(n, indices, x):
    """float64[2^k]: rho_x[a][a] = sum_b |x[a,b]|^2, in longdouble"""
    p = psi_matrix(n, indices, x)
    return np.sum(p.real ** 2 + p.imag ** 2, axis=1, dtype=np.longdouble).astype(np.float64)


def bars(ref_ket_diag, ref_bra_diag):
    """float64[2^k, 2^k]: the bar of every entry, rows by the ket's weights and columns by the bra's"""
    return BAR * np.sqrt(np.outer(np.maximum(ref_ket_diag, 0.0), np.maximum(ref_bra_diag, 0.0)))


def worst_ratio(got, ref, bar):
    """the largest |got - ref| / bar over the entries (an entry whose bar is zero has to be exactly zero: inf otherwise)"""
    err = np.abs(np.asarray(got) - ref)
    ratio = np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(np.max(ratio))


def permuted(m, perm):
    """M of the index list [indices[p] for p in perm] from M of `indices` (any matrix, Hermitian or not): bit i of a new row or
    column index is bit perm[i] of the old"""
    k = len(perm)
    old = np.zeros(1 << k, dtype=np.int64)
    for new in range(1 << k):
        for i, p in enumerate(perm):
            old[new] |= ((new >> i) & 1) << p
    return np.asarray(m)[np.ix_(old, old)]
