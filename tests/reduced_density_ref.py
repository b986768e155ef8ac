"""An exact reference for the reduced density matrix of a few qubits of a state, its bar, and the index sets the tests run —
shared by tests/test_reduced_density_cpu.py and tests/test_gpu_f2_reduced_density.py.  A plain helper module: numpy only.

With the amplitudes seen as a 2^k x 2^(n-k) matrix Psi (row a: bit i of a is the bit of qubit indices[i]; column b: the other
bits), rho[a][a'] = sum_b Psi[a,b] conj(Psi[a',b]), raw (divided by no norm).  The amplitudes of the states of
tests/measure_ref.py are widened to complex128, the products are formed in complex128 and summed over b in longdouble.

The bar for every entry is that of the project's matrix elements (tests/pauli_pair_ref.py: 1e-12 ||phi|| ||psi||) applied to
rows a and a' of Psi: |got - ref| <= 1e-12 sqrt(ref[a][a] ref[a'][a']); by Cauchy-Schwarz the absolute sum of an entry's
products is at most that square root.

Qubit q is amplitude-index bit n - 1 - q (`position`), as in tests/measure_ref.py."""
import itertools

import numpy as np

from measure_ref import DTYPES, make_state, qubits, seed_of  # noqa: F401  (the states and conventions of the measurement tests)

BAR = 1e-12


def psi_matrix(n, indices, x):
    """complex128[2^k, 2^(n-k)]: the amplitudes as rows a and columns b"""
    indices = [int(q) for q in indices]
    k = len(indices)
    assert len(set(indices)) == k and all(0 <= q < n for q in indices)
    cube = np.asarray(x).astype(np.complex128).reshape((2,) * n)  # axis q is qubit q (index bit n - 1 - q)
    rest = [q for q in range(n) if q not in indices]
    return cube.transpose(indices[::-1] + rest).reshape(1 << k, -1)  # (bit k-1 of a is the most significant: qubit indices[k-1])


def density_ref(n, indices, x):
    """complex128[2^k, 2^k]: rho of the qubits `indices`"""
    psi = psi_matrix(n, indices, x)
    m = psi.shape[0]
    out = np.empty((m, m), dtype=np.complex128)
    for a in range(m):
        prod = psi[a][None, :] * np.conj(psi)  # complex128 products, row a against every row a'
        out[a] = (np.sum(prod.real, axis=1, dtype=np.longdouble).astype(np.float64)
                  + 1j * np.sum(prod.imag, axis=1, dtype=np.longdouble).astype(np.float64))
    return out


def density_literal(n, indices, x):
    """the double loop of the definition, amplitude index by amplitude index (small n only)"""
    k = len(indices)
    pos = [n - 1 - int(q) for q in indices]
    x = np.asarray(x).astype(np.complex128)
    rest = [b for b in range(n) if b not in pos]
    out = np.zeros((1 << k, 1 << k), dtype=np.complex128)

    def index(a, b):
        j = 0
        for i, p in enumerate(pos):
            j |= ((a >> i) & 1) << p
        for i, p in enumerate(rest):
            j |= ((b >> i) & 1) << p
        return j

    for a in range(1 << k):
        for a2 in range(1 << k):
            acc = 0j
            for b in range(1 << len(rest)):
                acc += x[index(a, b)] * np.conj(x[index(a2, b)])
            out[a, a2] = acc
    return out


def bars(ref):
    """float64[2^k, 2^k]: the bar of every entry"""
    d = np.sqrt(np.maximum(np.diag(ref).real, 0.0))
    return BAR * np.outer(d, d)


def worst_ratio(got, ref):
    """the largest |got - ref| / bar over the entries (an entry whose bar is zero has to be exactly zero: inf otherwise)"""
    bar, err = bars(ref), np.abs(np.asarray(got) - ref)
    ratio = np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(np.max(ratio))


def exact_structure(rho):
    """the lower triangle is the bit-exact conjugate of the upper and every diagonal imaginary part is +0.0"""
    rho = np.asarray(rho)
    i, j = np.triu_indices(rho.shape[0], 1)
    lower, mirrored = np.ascontiguousarray(rho[j, i]), np.ascontiguousarray(np.conj(rho[i, j]))
    diag_im = np.ascontiguousarray(np.diag(rho).imag)
    return bool(np.array_equal(lower.view(np.uint8), mirrored.view(np.uint8))) and not np.any(diag_im.view(np.uint64))


def permuted(rho, perm):
    """rho of the index list [indices[p] for p in perm] from rho of `indices`: bit i of the new row index is bit perm[i] of the old"""
    k = len(perm)
    old = np.zeros(1 << k, dtype=np.int64)
    for new in range(1 << k):
        for i, p in enumerate(perm):
            old[new] |= ((new >> i) & 1) << p
    return np.asarray(rho)[np.ix_(old, old)]


def scrambled(positions, seed):
    """a fixed order of `positions` that is not ascending (when there are two or more)"""
    positions = list(positions)
    if len(positions) < 2:
        return positions
    order = [int(v) for v in np.random.default_rng(seed).permutation(len(positions))]
    if order == sorted(order):
        order = order[1:] + order[:1]
    return [positions[i] for i in order]


def position_sets(n, k):
    """the position sets of the one-block cases, each ascending: the lowest k bits (bit 0 is the half of a packed Complex<f32>
    element), the top k bits, bit 0 with the top bit plus scattered bits, and a set on either side of position 8"""
    sets = [list(range(k)), list(range(n - k, n)),
            sorted(([0, n - 1] + [b for b in (3, 5, 2, 6, 7, 4) if b < n - 1])[:k]),
            sorted([b for b in (8, 7, 9, 6, 10, 5) if b < n][:k])]
    out = []
    for s in sets:
        if len(s) == k and len(set(s)) == k and s not in out:
            out.append(s)
    return out


def few_column_sets(n, k):
    """the position sets of the few-column cases: the lowest k bits, the top k bits, and k evenly spread bits (bit 0 and the top
    bit among them) in a scrambled order"""
    spread = sorted({(i * (n - 1)) // (k - 1) for i in range(k)}) if k >= 2 else [n // 2]
    out = []
    for s in (list(range(k)), list(range(n - k, n)), scrambled(spread, 10 * n + k)):
        if len(s) == k and s not in out:
            out.append(s)
    return out


def ordered_subsets(n):
    """every ordered subset of the qubits of an n-qubit state, k = 1 .. n"""
    for k in range(1, n + 1):
        yield from (list(p) for p in itertools.permutations(range(n), k))
