"""An exact restatement of the trajectory rule of the noise-channel calls (include/qip_hipx.h: qipx_state_apply_reduce,
qipx_state_apply_channels) in complex128 / float64 — shared by tests/test_noise_cpu.py and tests/test_gpu_f3_noise.py.  A plain
helper module: numpy only, dense reshape / tensordot on the full vector.

Qubit q is amplitude-index bit n - 1 - q; bit i of a row of an operator on `qubits` is the bit of qubit qubits[i] (the conventions
of tests/reduced_density_ref.py, whose density_ref is the density used here).

The rule, for a channel {K_i} on `qubits` and one uniform sample u in [0, 1]:
    rho  = the raw reduced density matrix of the current state on `qubits`,  N = tr rho
    w_i  = Re Tr(K_i^H K_i rho),  W = sum_i w_i
    i*   = the smallest i with u * W < w_0 + .. + w_i; if there is none, the last i with w_i > 0
    psi <- sqrt(N / w_i*) K_i* psi"""
import itertools

import numpy as np

from reduced_density_ref import density_ref

MARGIN = 1e-6  # a sample has a defined outcome when u * W is at least MARGIN * W away from every cumulative boundary


def apply_matrix(n, qubits, matrix, x):
    """complex128[2^n]: (matrix on `qubits`) x"""
    qubits = [int(q) for q in qubits]
    k = len(qubits)
    cube = np.asarray(x).astype(np.complex128).reshape((2,) * n)  # axis q is qubit q
    m = np.asarray(matrix, dtype=np.complex128).reshape((2,) * (2 * k))  # row bits k-1 .. 0, then column bits k-1 .. 0
    out = np.tensordot(m, cube, axes=(list(range(k, 2 * k)), qubits[::-1]))  # axes: row bits k-1 .. 0, then the other qubits
    return np.moveaxis(out, list(range(k)), qubits[::-1]).reshape(-1)


def weights(kraus, rho):
    """float64[count]: w_i = Re Tr(K_i^H K_i rho)"""
    return np.array([float(np.real(np.trace(np.conj(K).T @ K @ rho))) for K in np.asarray(kraus, dtype=np.complex128)])


def select(w, u):
    """(i*, the distance of u * W from the nearest cumulative boundary in units of W)"""
    w = np.asarray(w, dtype=np.float64)
    W = float(np.sum(w))
    assert W > 0
    r, cum = u * W, np.cumsum(w)
    margin = float(np.min(np.abs(cum[:-1] - r))) / W if len(w) > 1 else 1.0
    for i in range(len(w)):
        if r < cum[i]:
            return i, margin
    return int(np.max(np.nonzero(w > 0)[0])), margin


def step(n, qubits, kraus, x, u):
    """one channel: (i*, weights, the scaled operator that is applied, new state, margin)"""
    kraus = np.asarray(kraus, dtype=np.complex128)
    rho = density_ref(n, qubits, x)
    w = weights(kraus, rho)
    i, margin = select(w, u)
    op = np.sqrt(float(np.real(np.trace(rho))) / w[i]) * kraus[i]
    return i, w, op, apply_matrix(n, qubits, op, x), margin


class Trajectory:
    """chosen[c], weights[c], applied[c] (the scaled operator), states[c] (after channel c), state (the last), margin (the smallest)"""


def trajectory(n, channels, x, us, store=None):
    """channels: (qubits, kraus) pairs.  store = numpy.complex64: the state is rounded to that type after every channel, as a
    Complex<f32> device state stores it (the weights of the next channel are those of the STORED state)."""
    t = Trajectory()
    t.chosen, t.weights, t.applied, t.states, t.margin = [], [], [], [], 1.0
    x = np.asarray(x).astype(np.complex128)
    for (qubits, kraus), u in zip(channels, us):
        i, w, op, x, m = step(n, qubits, kraus, x, float(u))
        if store is not None:
            x = x.astype(store).astype(np.complex128)
        t.chosen.append(i)
        t.weights.append(w)
        t.applied.append(op)
        t.states.append(x)
        t.margin = min(t.margin, m)
    t.state = x
    return t


def apply_reduce(n, indices, matrix, next_indices, x):
    """(the state after the matrix, the reduced density matrix of that state on next_indices)"""
    y = apply_matrix(n, indices, matrix, x)
    return y, density_ref(n, next_indices, y)


def branches(n, channels, x):
    """every branch of the chain with its probability, by exact enumeration: [(p, state)], sum of p = 1 for complete channels"""
    x = np.asarray(x).astype(np.complex128)
    out = []
    for picks in itertools.product(*[range(len(kraus)) for _, kraus in channels]):
        y, p = x, 1.0
        for (qubits, kraus), i in zip(channels, picks):
            kraus = np.asarray(kraus, dtype=np.complex128)
            rho = density_ref(n, qubits, y)
            w = weights(kraus, rho)
            if not w[i] > 0:
                p = 0.0
                break
            p *= w[i] / float(np.sum(w))
            y = apply_matrix(n, qubits, np.sqrt(float(np.real(np.trace(rho))) / w[i]) * kraus[i], y)
        if p > 0:
            out.append((p, y))
    return out


def kraus_map(n, channels, rho):
    """the chain of Kraus maps applied to a full density matrix: rho -> sum_i K_i rho K_i^H per channel"""
    dim = 1 << n
    for qubits, kraus in channels:
        full = [np.stack([apply_matrix(n, qubits, K, np.eye(dim)[:, j]) for j in range(dim)], axis=1) for K in np.asarray(kraus, dtype=np.complex128)]
        rho = sum(F @ rho @ np.conj(F).T for F in full)
    return rho
