"""Multiplexed (uniformly controlled) gates on a device state, each a thin call of HipState.apply_multiplexed (include/qip_hipx.h:
qipx_state_apply_multiplexed): one in-place pass for all 2^m values of the select register, no multi-controlled gate per table
entry, no kernels of its own.

A register is a sequence of qubits, least significant bit first: bit i of the select value x is the bit of qubit select[i], bit i of a
matrix row or column is the bit of qubit targets[i].

Measured at n = 30 (profiles/multiplex.md), Complex<f64> / Complex<f32>: one call 5.8 - 6.4 / 2.9 - 3.1 ms for up to 10 select qubits and a
target among the six low index bits, 1.07 - 1.21 / 1.06 - 1.12 plain gate passes; 16 controlled gates through apply_ops take 14 - 19 / 13 - 18 ms.
For 2 select qubits the 4 controlled gates (Complex<f64>) and for up to 5 (Complex<f32>: 4) qubits in all one block-diagonal dense op
through apply_op are 2 - 14 % faster than the call.  prepare_register of a whole state of 10 / 19 qubits 0.32 / 23 ms (19 passes, each with a
table built on the host) against 0.02 / 0.15 - 0.23 ms for upload of the same amplitudes: it is for registers INSIDE a state that is
already on the device, not a replacement for upload."""
from __future__ import annotations

from typing import Sequence

import numpy as np

from .ops import CircuitError
from .state import HipState


def rotation_matrices(axis: str, angles) -> np.ndarray:
    """the (len(angles), 2, 2) complex128 table of Rx, Ry or Rz(angle) = exp(-i angle/2 P): cos and sin of the half angle by
    numpy in double"""
    half = np.asarray(angles, dtype=np.float64).reshape(-1) / 2
    c, s = np.cos(half), np.sin(half)
    out = np.zeros((len(half), 2, 2), dtype=np.complex128)
    ax = str(axis).lower()
    if ax == "x":
        out[:, 0, 0], out[:, 0, 1], out[:, 1, 0], out[:, 1, 1] = c, -1j * s, -1j * s, c
    elif ax == "y":
        out[:, 0, 0], out[:, 0, 1], out[:, 1, 0], out[:, 1, 1] = c, -s, s, c
    elif ax == "z":
        out[:, 0, 0], out[:, 1, 1] = c - 1j * s, c + 1j * s
    else:
        raise CircuitError(f"rotation: axis {axis!r} is none of 'x', 'y', 'z'")
    return out


def rotation(st: HipState, axis: str, select: Sequence[int], target: int, angles) -> None:
    """|x>|t> -> |x> R_axis(angles[x])|t>: a multiplexed Rx, Ry or Rz on `target`, 2^m angles"""
    mats = rotation_matrices(axis, angles)
    if len(mats) != 1 << len(select):
        raise CircuitError(f"rotation: {len(mats)} angles for a select register of {len(select)} qubits")
    st.apply_multiplexed(select, [target], mats)


def _gate_table(gates, m: int, k: int, what: str) -> np.ndarray:
    mats = np.asarray(gates, dtype=np.complex128)
    if mats.size != (1 << m) * 4 ** k:
        raise CircuitError(f"{what}: {len(mats)} gates of {mats.shape[1:]} for {m} select and {k} target qubits")
    return mats.reshape(1 << m, 1 << k, 1 << k)


def select_gates(st: HipState, select: Sequence[int], targets: Sequence[int], gates) -> None:
    """|x>|t> -> |x> gates[x]|t>: a list of 2^m gates on one or two target qubits (2^k x 2^k each, flat or square)"""
    st.apply_multiplexed(select, targets, _gate_table(gates, len(select), len(targets), "select_gates"))


def controlled_table(n_controls: int, gates: np.ndarray) -> np.ndarray:
    """the table of `controlled`: the select value's low bits choose the gate, its top n_controls bits are the controls; wherever
    one of them reads 0 the matrix is the exact identity"""
    count, dim = gates.shape[0], gates.shape[1]
    out = np.empty((count << n_controls, dim, dim), dtype=np.complex128)
    out[:] = np.eye(dim, dtype=np.complex128)
    out[len(out) - count:] = gates
    return out


def controlled(st: HipState, controls: Sequence[int], select: Sequence[int], targets: Sequence[int], gates) -> None:
    """select_gates where every qubit of `controls` reads 1, the identity elsewhere: each control is one more select bit whose unset
    half of the table is the exact identity, so those amplitudes keep their bits"""
    mats = _gate_table(gates, len(select), len(targets), "controlled")
    st.apply_multiplexed(list(select) + list(controls), targets, controlled_table(len(controls), mats))


def prepare_tables(amplitudes):
    """(angle tables, phases) of prepare_register: angles[i] holds the 2^i Ry angles of pass i, selected by the register's bits
    below i, phases[r] = arg amplitudes[r].  Pass i splits the weight of every branch x (the bits below i) between bit i = 0 and
    bit i = 1: angle 2 atan2(sqrt(w1), sqrt(w0)); a branch of zero norm gets angle 0."""
    a = np.asarray(amplitudes, dtype=np.complex128).reshape(-1)
    k = max(len(a).bit_length() - 1, 0)
    if len(a) != 1 << k or k < 1:
        raise CircuitError(f"prepare_register: {len(a)} amplitudes are not those of a register of one or more qubits")
    w = a.real * a.real + a.imag * a.imag
    weights = [w]  # weights[j][x]: the weight of the branch whose bits below k - j read x
    for _ in range(k):
        w = w.reshape(2, -1).sum(axis=0)
        weights.append(w)
    if not np.isclose(weights[k][0], 1.0, rtol=0, atol=1e-6):
        raise CircuitError(f"prepare_register: the amplitudes have squared norm {weights[k][0]}, not 1")
    angles = []
    for i in range(k):
        split = weights[k - i - 1].reshape(2, -1)  # [bit i, x]
        angles.append(2.0 * np.arctan2(np.sqrt(split[1]), np.sqrt(split[0])))
    return angles, np.angle(a)


def prepare_register(st: HipState, qubits: Sequence[int], amplitudes) -> None:
    """takes the register `qubits` from |0...0> to sum_r amplitudes[r] |r> (normalised; bit i of r = qubit qubits[i]), whatever
    the rest of the state holds: k multiplexed Ry passes, qubit i selected by the qubits before it, then one phase table through
    apply_function.  (Where the register does not read 0 the map is the same product of rotations: unitary, but not a load.)"""
    qubits = list(qubits)
    angles, phases = prepare_tables(amplitudes)
    if len(angles) != len(qubits):
        raise CircuitError(f"prepare_register: {1 << len(angles)} amplitudes for a register of {len(qubits)} qubits")
    for i, th in enumerate(angles):
        rotation(st, "y", qubits[:i], qubits[i], th)
    st.apply_function(qubits, (), phases=phases)
