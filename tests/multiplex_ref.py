"""A reference for the multiplexed gate (include/qip_hipx.h: qipx_state_apply_multiplexed), by index arithmetic alone: for every
basis index j the select value x and the matrix index a are gathered bit by bit from j, the group's other members are j with its
target bits replaced, and y_a is summed in matrix-index order.  Nothing of the kernel's rows, walks or shuffles appears here.

    apply_multiplexed_spec    the header's arithmetic exactly, in the state's dtype: the table rounded once, four products and two
                              sums per term, each rounded (numpy never fuses), terms added for a' ascending; a row that is exactly
                              a unit row passes the amplitude's bits
    apply_multiplexed_exact   the same map in np.clongdouble for complex128 states and in complex128 for complex64 states, from the
                              table as given (unrounded)

and the builders the tests share: tables of unitary, real and wildly scaled matrices, the block-diagonal dense matrix of a table,
the Ry chain of a register preparation."""
import numpy as np

from function_ref import DTYPES, UNIT, gather, make_state, scatter  # noqa: F401  (the tests take them from here)

REAL = {np.dtype(np.complex128): np.float64, np.dtype(np.complex64): np.float32}
BAR = {1: 6.0, 2: 9.0}  # (1.5 M + 3) u


def _groups(n, select, targets):
    """x and a of every index, and the indices of every index's group in matrix-index order: part[a'][j]"""
    j = np.arange(2 ** n, dtype=np.uint64)
    x = gather(n, j, select)
    a = gather(n, j, targets)
    M = 2 ** len(targets)
    rest = j & ~scatter(n, np.full_like(j, M - 1), targets)
    part = [rest | scatter(n, np.full_like(j, a2), targets) for a2 in range(M)]
    return x.astype(np.int64), a.astype(np.int64), [p.astype(np.int64) for p in part]


def _table(matrices, m, k):
    t = np.asarray(matrices, dtype=np.complex128)
    assert t.shape == (2 ** m, 2 ** k, 2 ** k), t.shape
    return t


def unit_rows(table):
    """[x, a]: row a of matrix x is exactly the unit row e_a (zeros of either sign)"""
    M = table.shape[1]
    return np.all(table == np.eye(M, dtype=table.dtype)[None, :, :], axis=2)


def apply_multiplexed_spec(n, psi, select, targets, matrices):
    dtype = np.dtype(psi.dtype)
    real = REAL[dtype]
    with np.errstate(all="ignore"):
        table = _table(matrices, len(select), len(targets)).astype(dtype)  # rounded once
        x, a, part = _groups(n, select, targets)
        pr, pi = np.ascontiguousarray(psi.real, dtype=real), np.ascontiguousarray(psi.imag, dtype=real)
        yr = yi = None
        for a2, idx in enumerate(part):
            w = table[x, a, a2]
            wr, wi = np.ascontiguousarray(w.real), np.ascontiguousarray(w.imag)
            xr, xi = pr[idx], pi[idx]
            tr = wr * xr - wi * xi
            ti = wr * xi + wi * xr
            assert tr.dtype == real
            yr, yi = (tr, ti) if a2 == 0 else (yr + tr, yi + ti)
        keep = unit_rows(table)[x, a]
        out = np.empty_like(psi)
        out.real = np.where(keep, pr, yr)
        out.imag = np.where(keep, pi, yi)
    return out


def apply_multiplexed_exact(n, psi, select, targets, matrices):
    wide = np.clongdouble if np.dtype(psi.dtype) == np.complex128 else np.complex128
    table = _table(matrices, len(select), len(targets)).astype(wide)
    x, a, part = _groups(n, select, targets)
    v = psi.astype(wide)
    y = np.zeros(len(psi), dtype=wide)
    for a2, idx in enumerate(part):
        y = y + table[x, a, a2] * v[idx]
    return y


def norm_products(n, psi, select, targets, matrices):
    """|U_x[a]|_2 |v|_2 of every index, in double: what the error statement is relative to"""
    table = _table(matrices, len(select), len(targets))
    x, a, part = _groups(n, select, targets)
    v2 = sum(np.abs(psi.astype(np.complex128)[idx]) ** 2 for idx in part)
    return np.sqrt(np.sum(np.abs(table) ** 2, axis=2))[x, a] * np.sqrt(v2)


def group_norms(n, psi, targets):
    _, _, part = _groups(n, [], targets)
    return np.sqrt(sum(np.abs(psi.astype(np.complex128)[idx]) ** 2 for idx in part))


# ---- tables ----------------------------------------------------------------------------------------------------------------------
def unitary_table(rng, m, k):
    M = 2 ** k
    z = rng.standard_normal((2 ** m, M, M)) + 1j * rng.standard_normal((2 ** m, M, M))
    qm, r = np.linalg.qr(z)
    d = np.diagonal(r, axis1=1, axis2=2)
    return qm * (d / np.abs(d))[:, None, :]


def real_table(rng, m, k):
    M = 2 ** k
    return rng.standard_normal((2 ** m, M, M)).astype(np.complex128)


def scaled_table(rng, m, k, decades=6):
    """entries whose magnitudes spread over 2 * decades decades, entry by entry"""
    M = 2 ** k
    z = rng.standard_normal((2 ** m, M, M)) + 1j * rng.standard_normal((2 ** m, M, M))
    return z * 10.0 ** rng.uniform(-decades, decades, size=z.shape)


TABLES = {"unitary": unitary_table, "real": real_table, "scaled": scaled_table}


def with_identities(rng, table, share=0.5):
    """the table with about `share` of its matrices replaced by the exact identity; returns (table, mask of the replaced)"""
    t = np.array(table)
    mask = rng.random(len(t)) < share
    t[mask] = np.eye(t.shape[1])
    return t, mask


def block_diagonal(table):
    """the dense matrix of the map on select + target qubits with sub-index x * M + a, and the order of the op's qubits for it
    (a MatrixOp's first index is the most significant sub-index bit): index_order(select, targets)"""
    count, M = table.shape[0], table.shape[1]
    out = np.zeros((count * M, count * M), dtype=np.complex128)
    for x in range(count):
        out[x * M:(x + 1) * M, x * M:(x + 1) * M] = table[x]
    return out


def index_order(select, targets):
    return list(select)[::-1] + list(targets)[::-1]


# ---- register preparation ----------------------------------------------------------------------------------------------------------
def ry_chain(amplitudes):
    """the tables of the k multiplexed Ry passes that take |0..0> to |amplitudes| (pass i: qubit i selected by the qubits below it,
    2^i matrices) and the phases of the final phase table — written out here independently of rustqip_amd.multiplex"""
    a = np.asarray(amplitudes, dtype=np.complex128)
    k = len(a).bit_length() - 1
    w = a.real * a.real + a.imag * a.imag
    levels = {k: w}  # levels[b][x]: the weight of the branch whose low b bits read x
    for b in range(k - 1, -1, -1):
        w = w.reshape(2, -1).sum(axis=0)
        levels[b] = w
    tables = []
    for i in range(k):
        split = levels[i + 1].reshape(2, -1)
        half = (2.0 * np.arctan2(np.sqrt(split[1]), np.sqrt(split[0]))) / 2
        c, s = np.cos(half), np.sin(half)
        t = np.zeros((2 ** i, 2, 2), dtype=np.complex128)
        t[:, 0, 0], t[:, 0, 1], t[:, 1, 0], t[:, 1, 1] = c, -s, s, c
        tables.append(t)
    return tables, np.angle(a)


def random_amplitudes(rng, k, zero_branch=False):
    a = rng.standard_normal(2 ** k) + 1j * rng.standard_normal(2 ** k)
    if zero_branch and k >= 2:
        a[np.arange(2 ** k) % 4 == 1] = 0  # the branches whose low two bits read 01 have no weight
    return a / np.linalg.norm(a)
