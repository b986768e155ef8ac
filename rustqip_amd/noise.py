"""Noise channels on a device state by quantum trajectories, each a thin call of HipState.apply_channels (include/qip_hipx.h:
qipx_state_apply_channels): no kernels of its own.

A channel is a list of Kraus operators {K_i} on one or two qubits.  A trajectory draws branch i with probability
|K_i psi|^2 / |psi|^2 and replaces psi by K_i psi, rescaled to the old norm; the average of <psi| O |psi> over trajectories is
Tr(O E(rho)) for the channel E(rho) = sum_i K_i rho K_i^H.  Bit i of a row of an operator is the bit of qubit qubits[i]."""
from __future__ import annotations

from typing import Callable, Sequence

import numpy as np

from .ops import CircuitError
from .state import HipState

_I = np.eye(2, dtype=np.complex128)
_X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
_Y = np.array([[0, -1j], [1j, 0]], dtype=np.complex128)
_Z = np.array([[1, 0], [0, -1]], dtype=np.complex128)


class Channel:
    """Kraus operators `kraus` (count x 2^k x 2^k) on the k qubits `qubits`"""

    def __init__(self, qubits: Sequence[int], kraus):
        self.qubits = [int(q) for q in qubits]
        ks = np.asarray(kraus, dtype=np.complex128)
        if ks.ndim == 2:
            ks = ks[None]
        m = 1 << len(self.qubits)
        if ks.ndim != 3 or ks.shape[1:] != (m, m):
            raise CircuitError(f"operators of shape {ks.shape[1:]} on {len(self.qubits)} qubits")
        self.kraus = np.ascontiguousarray(ks)

    def completeness_defect(self) -> float:
        """max |sum_i K_i^H K_i - 1|"""
        total = np.einsum("iba,ibc->ac", np.conj(self.kraus), self.kraus)
        return float(np.max(np.abs(total - np.eye(total.shape[0]))))

    def check(self, tol: float = 1e-12) -> "Channel":
        """raises unless sum_i K_i^H K_i = 1 to `tol` (trace preserving)"""
        defect = self.completeness_defect()
        if not defect <= tol:
            raise CircuitError(f"the operators on qubits {self.qubits} are not complete: |sum K^H K - 1| = {defect:.3e} > {tol:.1e}")
        return self


def _probability(p: float, what: str) -> float:
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise CircuitError(f"{what}: {p} is not a probability")
    return p


def gate(qubits: Sequence[int], matrix) -> Channel:
    """one operator, taken with certainty: a plain gate between channels (any matrix; the norm is carried through)"""
    return Channel(qubits, np.asarray(matrix, dtype=np.complex128)[None])


def pauli_channel(qubit: int, px: float, py: float, pz: float) -> Channel:
    """X, Y, Z with probabilities px, py, pz, nothing with the rest"""
    px, py, pz = (_probability(p, "pauli_channel") for p in (px, py, pz))
    p0 = 1.0 - px - py - pz
    if p0 < -1e-15:
        raise CircuitError(f"pauli_channel: the probabilities add up to {px + py + pz}")
    return Channel([qubit], [np.sqrt(max(p0, 0.0)) * _I, np.sqrt(px) * _X, np.sqrt(py) * _Y, np.sqrt(pz) * _Z]).check()


def bit_flip(qubit: int, p: float) -> Channel:
    p = _probability(p, "bit_flip")
    return Channel([qubit], [np.sqrt(1.0 - p) * _I, np.sqrt(p) * _X]).check()


def phase_flip(qubit: int, p: float) -> Channel:
    p = _probability(p, "phase_flip")
    return Channel([qubit], [np.sqrt(1.0 - p) * _I, np.sqrt(p) * _Z]).check()


def depolarizing(qubits, p: float) -> Channel:
    """rho -> (1 - p) rho + p 1 / 2^k tr rho on one qubit (an int or a list of one) or two: every non-identity Pauli string with
    probability p / 4^k"""
    p = _probability(p, "depolarizing")
    qubits = [int(qubits)] if np.isscalar(qubits) else [int(q) for q in qubits]
    k = len(qubits)
    if k not in (1, 2):
        raise CircuitError(f"depolarizing on {k} qubits: one or two are supported")
    paulis = [_I, _X, _Y, _Z]
    strings = paulis if k == 1 else [np.kron(b, a) for b in paulis for a in paulis]  # (bit 0 of a row = qubits[0]: the right factor)
    each = p / 4 ** k
    ops = [np.sqrt(1.0 - p + each) * strings[0]] + [np.sqrt(each) * s for s in strings[1:]]
    return Channel(qubits, ops).check()


def amplitude_damping(qubit: int, gamma: float) -> Channel:
    """|1> decays to |0> with probability gamma"""
    g = _probability(gamma, "amplitude_damping")
    return Channel([qubit], [[[1, 0], [0, np.sqrt(1.0 - g)]], [[0, np.sqrt(g)], [0, 0]]]).check()


def generalized_amplitude_damping(qubit: int, gamma: float, p: float) -> Channel:
    """amplitude damping towards the mixture p |0><0| + (1 - p) |1><1|"""
    g, p = _probability(gamma, "generalized_amplitude_damping"), _probability(p, "generalized_amplitude_damping")
    a, b, c = np.sqrt(1.0 - g), np.sqrt(g), np.sqrt(p)
    d = np.sqrt(1.0 - p)
    return Channel([qubit], [c * np.array([[1, 0], [0, a]]), c * np.array([[0, b], [0, 0]]),
                             d * np.array([[a, 0], [0, 1]]), d * np.array([[0, 0], [b, 0]])]).check()


def phase_damping(qubit: int, lam: float) -> Channel:
    """the off-diagonal element shrinks by sqrt(1 - lam)"""
    lam = _probability(lam, "phase_damping")
    return Channel([qubit], [[[1, 0], [0, np.sqrt(1.0 - lam)]], [[0, 0], [0, np.sqrt(lam)]]]).check()


def trajectory(state: HipState, channels: Sequence[Channel], seed):
    """One trajectory of `channels` (in order) on `state`, in place; the uniforms come from numpy.random.default_rng(seed), one
    per channel.  Returns (chosen, weights) of HipState.apply_channels."""
    channels = list(channels)
    return state.apply_channels(channels, np.random.default_rng(seed).random(len(channels)))


def average(fn: Callable[[HipState], object], make_state: Callable[[], HipState], channels: Sequence[Channel], shots: int, seed):
    """The mean of fn(state) over `shots` trajectories of `channels`, each on a fresh make_state().  A plain loop that holds one
    state at a time; trajectory t draws from numpy.random.default_rng([seed, t])."""
    shots = int(shots)
    if shots < 1:
        raise CircuitError(f"average over {shots} trajectories")
    total = None
    for t in range(shots):
        with make_state() as st:
            trajectory(st, channels, [int(seed), t])
            v = np.asarray(fn(st))
        total = v if total is None else total + v
    return total / shots
