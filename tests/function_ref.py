"""A reference for the classical-function call (include/qip_hipx.h: qipx_state_apply_function), by index arithmetic alone:
for every basis index j, x and y are gathered bit by bit from j, y' = y ^ values[x] or (y + values[x]) mod 2^k is scattered back
into j, and new[j'] = w(x) old[j].  Nothing of the kernel's tiles, rows or passes appears here.  With phases, w and the product
are formed in complex128."""
import numpy as np

DTYPES = (np.complex128, np.complex64)
UNIT = {np.complex128: 2.0 ** -53, np.complex64: 2.0 ** -24}


def gather(n, j, qubits):
    """the register value of every index in j: bit i = the bit of qubit qubits[i] = index bit n-1-qubits[i]"""
    v = np.zeros_like(j)
    for i, q in enumerate(qubits):
        v |= ((j >> np.uint64(n - 1 - q)) & np.uint64(1)) << np.uint64(i)
    return v


def scatter(n, v, qubits):
    j = np.zeros_like(v)
    for i, q in enumerate(qubits):
        j |= ((v >> np.uint64(i)) & np.uint64(1)) << np.uint64(n - 1 - q)
    return j


def destination(n, in_qubits, out_qubits, values, mode):
    """j' for every j = 0 .. 2^n - 1, and x of every j"""
    j = np.arange(2 ** n, dtype=np.uint64)
    x = gather(n, j, in_qubits)
    if len(out_qubits) == 0:
        return j, x
    v = np.asarray(values, dtype=np.uint64)[x]
    y = gather(n, j, out_qubits)
    if mode == "xor":
        y2 = y ^ v
    else:
        y2 = (y + v) & np.uint64(2 ** len(out_qubits) - 1)
    return (j & ~scatter(n, np.full_like(j, 2 ** len(out_qubits) - 1), out_qubits)) | scatter(n, y2, out_qubits), x


def apply_function_ref(n, psi, in_qubits, out_qubits, values=None, phases=None, mode="xor"):
    """the new state: psi's dtype without phases (a pure move: the bits of psi), complex128 with phases"""
    to, x = destination(n, in_qubits, out_qubits, values, mode)
    if phases is None:
        out = np.empty_like(psi)
        out[to] = psi
        return out
    ph = np.asarray(phases, dtype=np.float64)
    w = (np.cos(ph) + 1j * np.sin(ph))[x]
    out = np.empty(len(psi), dtype=np.complex128)
    out[to] = w * psi.astype(np.complex128)
    return out


def permutation_rows(n_sub, in_count, out_count, values, mode):
    """The same map as a SparseMatrix op on qubits 0 .. m+k-1 of an (m+k)-qubit register, in the op's own convention (the op's
    qubit t is sub-index bit m+k-1-t): rows[r] = [(column, 1.0)] with new[r] = old[column].  The op's qubits are the in register's
    (bit i of x = op qubit i) followed by the out register's."""
    assert n_sub == in_count + out_count
    to, _ = destination(n_sub, list(range(in_count)), list(range(in_count, n_sub)), values, mode)
    rows = [None] * (2 ** n_sub)
    for j, t in enumerate(to):
        rows[int(t)] = [(int(j), 1.0)]
    return rows


def make_state(n, seed, dtype):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(2 ** n) + 1j * rng.standard_normal(2 ** n)
    x /= np.linalg.norm(x)
    return x.astype(dtype)
