"""Parametrised gates and the host side of HipState.circuit_gradient: what a gate and its derivative are, how a circuit is cut
into blocks and passes, and how a gate's matrix meets a reduced transition matrix.  Pure host bookkeeping (numpy): nothing here
touches amplitudes.

Two index conventions meet here.  A MatrixOp's FIRST listed qubit is the MOST significant bit of its matrix index (a Control
op lists its controls first).  Bit i of a row index of HipState.transition_matrix(ket, indices) is the bit of qubit indices[i]:
the first listed qubit is the LEAST significant.  `reduce_transition` is the one place that converts.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Sequence

import numpy as np

from .ops import CircuitError, MatrixOp, flatten, make_control_op, make_matrix_op

_I2 = np.eye(2, dtype=np.complex128)
_PAULI = {"I": _I2, "X": np.array([[0, 1], [1, 0]], dtype=np.complex128), "Y": np.array([[0, -1j], [1j, 0]], dtype=np.complex128),
          "Z": np.array([[1, 0], [0, -1]], dtype=np.complex128)}
MAX_GATE_QUBITS = 3  # controls included: the widest set HipState.transition_matrix takes


@dataclass
class ParamGate:
    """A gate W(theta) on `targets`, applied where every qubit of `controls` is 1.  `matrix(theta)` and `dmatrix(theta)` give W
    and dW/dtheta on the targets as 2^t x 2^t arrays, the first target the most significant bit (the MatrixOp convention)."""

    targets: List[int]
    controls: List[int]
    matrix: Callable[[float], np.ndarray]
    dmatrix: Callable[[float], np.ndarray]

    def __post_init__(self):
        self.targets = [int(q) for q in self.targets]
        self.controls = [int(q) for q in self.controls]
        if not self.targets:
            raise CircuitError("a parametrised gate needs at least one target qubit")
        if len(set(self.qubits)) != len(self.qubits) or min(self.qubits) < 0:
            raise CircuitError(f"a parametrised gate's qubits must be distinct and non-negative, not {self.qubits}")

    @property
    def qubits(self) -> List[int]:
        """controls first, then targets: the index list of the lowered op"""
        return self.controls + self.targets

    def lower(self, theta: float) -> MatrixOp:
        """the MatrixOp of W(theta): make_control_op(controls, make_matrix_op(targets, W))"""
        op = make_matrix_op(self.targets, self.matrix(float(theta)))
        return make_control_op(self.controls, op) if self.controls else op

    def _embed(self, block: np.ndarray, identity: bool) -> np.ndarray:
        side, t = 1 << len(self.qubits), 1 << len(self.targets)
        full = np.eye(side, dtype=np.complex128) if identity else np.zeros((side, side), dtype=np.complex128)
        full[side - t:, side - t:] = np.asarray(block, dtype=np.complex128).reshape(t, t)
        return full

    def full(self, theta: float) -> np.ndarray:
        """W on controls + targets (the controls the most significant bits): the identity outside the all-ones control block"""
        return self._embed(self.matrix(float(theta)), True)

    def dfull(self, theta: float) -> np.ndarray:
        """dW/dtheta on controls + targets: zero outside the all-ones control block"""
        return self._embed(self.dmatrix(float(theta)), False)

    def a_matrix(self, theta: float) -> np.ndarray:
        """A = dW/dtheta W^H on controls + targets: d<l|W psi>/dtheta = <l| A |W psi>"""
        return self.dfull(theta) @ self.full(theta).conj().T


def _involution_gate(targets: Sequence[int], p: np.ndarray, scale: float, controls: Sequence[int]) -> ParamGate:
    """exp(-i theta scale P) for P^2 = 1: cos(phi) 1 - i sin(phi) P with phi = scale * theta, in closed form"""
    one = np.eye(len(p), dtype=np.complex128)
    return ParamGate(list(targets), list(controls),
                     lambda th: np.cos(scale * th) * one - 1j * np.sin(scale * th) * p,
                     lambda th: scale * (-np.sin(scale * th) * one - 1j * np.cos(scale * th) * p))


def rx(q: int, controls: Sequence[int] = ()) -> ParamGate:
    """rx(theta) = exp(-i theta X / 2), the usual half-angle convention"""
    return _involution_gate([q], _PAULI["X"], 0.5, controls)


def ry(q: int, controls: Sequence[int] = ()) -> ParamGate:
    """ry(theta) = exp(-i theta Y / 2)"""
    return _involution_gate([q], _PAULI["Y"], 0.5, controls)


def rz(q: int, controls: Sequence[int] = ()) -> ParamGate:
    """rz(theta) = exp(-i theta Z / 2) = diag(e^(-i theta/2), e^(i theta/2))"""
    return _involution_gate([q], _PAULI["Z"], 0.5, controls)


def phase(q: int, controls: Sequence[int] = ()) -> ParamGate:
    """phase(theta) = diag(1, e^(i theta))"""
    return ParamGate([q], list(controls), lambda th: np.diag([1.0, np.exp(1j * th)]), lambda th: np.diag([0.0, 1j * np.exp(1j * th)]))


def rxx(q0: int, q1: int, controls: Sequence[int] = ()) -> ParamGate:
    """rxx(theta) = exp(-i theta X(x)X / 2)"""
    return _involution_gate([q0, q1], np.kron(_PAULI["X"], _PAULI["X"]), 0.5, controls)


def ryy(q0: int, q1: int, controls: Sequence[int] = ()) -> ParamGate:
    """ryy(theta) = exp(-i theta Y(x)Y / 2)"""
    return _involution_gate([q0, q1], np.kron(_PAULI["Y"], _PAULI["Y"]), 0.5, controls)


def rzz(q0: int, q1: int, controls: Sequence[int] = ()) -> ParamGate:
    """rzz(theta) = exp(-i theta Z(x)Z / 2)"""
    return _involution_gate([q0, q1], np.kron(_PAULI["Z"], _PAULI["Z"]), 0.5, controls)


def pauli_rotation(term, controls: Sequence[int] = ()) -> ParamGate:
    """exp(-i theta P) — this project's convention for Pauli rotations (HipState.apply_pauli_rotations), NO half angle — for a
    term given as a mapping {qubit: "X" | "Y" | "Z"} (I factors are dropped); the targets are the term's qubits ascending"""
    factors = sorted((int(q), str(p).upper()) for q, p in dict(term).items())
    for _, p in factors:
        if p not in _PAULI:
            raise CircuitError(f"not a Pauli factor: {p!r} (use I, X, Y or Z)")
    factors = [(q, p) for q, p in factors if p != "I"]
    if not factors:
        raise CircuitError("a Pauli rotation needs at least one factor that is not I")
    mat = np.ones((1, 1), dtype=np.complex128)
    for _, p in factors:
        mat = np.kron(mat, _PAULI[p])
    return _involution_gate([q for q, _ in factors], mat, 1.0, controls)


def generator_gate(targets: Sequence[int], g, controls: Sequence[int] = ()) -> ParamGate:
    """exp(-i theta G) for a Hermitian G on `targets` (first target = most significant bit), through numpy.linalg.eigh on the host"""
    targets = list(targets)
    g = np.asarray(g, dtype=np.complex128)
    side = 1 << len(targets)
    if g.shape != (side, side):
        raise CircuitError(f"the generator of a gate on {len(targets)} qubits is {side} x {side}, not {g.shape}")
    if not np.all(np.isfinite(g)) or not np.allclose(g, g.conj().T, rtol=0.0, atol=1e-12 * max(1.0, float(np.max(np.abs(g))))):
        raise CircuitError("the generator is not a finite Hermitian matrix")
    w, v = np.linalg.eigh(g)
    return ParamGate(targets, list(controls),
                     lambda th: (v * np.exp(-1j * th * w)) @ v.conj().T,
                     lambda th: (v * (-1j * w * np.exp(-1j * th * w))) @ v.conj().T)


# ---- blocks and passes -------------------------------------------------------------------------------------------------------------

def _op_qubits(op: MatrixOp) -> List[int]:
    return [int(q) for q in op.indices]


def circuit_items(circuit):
    """[(gate or op, parameter index or None, qubits)] of a circuit: its items are a MatrixOp (fixed) or a pair (ParamGate, p)"""
    items = []
    for i, item in enumerate(circuit):
        if isinstance(item, MatrixOp):
            flatten(item)  # (a Control op whose lists do not match raises here)
            items.append((item, None, _op_qubits(item)))
        elif isinstance(item, (tuple, list)) and len(item) == 2 and isinstance(item[0], ParamGate):
            gate, p = item
            if isinstance(p, bool) or not isinstance(p, (int, np.integer)) or int(p) < 0:
                raise CircuitError(f"circuit item {i}: the parameter index is {p!r}")
            if len(gate.qubits) > MAX_GATE_QUBITS:
                raise CircuitError(f"circuit item {i}: a parametrised gate on {len(gate.qubits)} qubits, controls included "
                                   f"(at most {MAX_GATE_QUBITS})")
            items.append((gate, int(p), list(gate.qubits)))
        else:
            raise CircuitError(f"circuit item {i} is neither a MatrixOp nor a pair (ParamGate, parameter index)")
    return items


def gradient_plan(circuit) -> List[dict]:
    """How HipState.circuit_gradient walks `circuit` backwards: a list of blocks, the LAST block of the circuit first.  A block is
    {"gates": the circuit indices of its gates in circuit order, "passes": [{"qubits": [...], "gates": [...]}, ...]}.

    Blocks: walking from the end with `used` = the qubits of the gates already in the block, a gate joins unless it is
    parametrised and its qubits (controls included) meet `used`; then the block closes and the gate starts the next one.  So
    every later gate of a block commutes with A = dW W^H of each of its parametrised gates, and all of them are differentiated
    from the pair of states as it is after the whole block.  Passes: the block's parametrised gates in circuit order, first-fit
    into sets whose union has at most three qubits; one transition_matrix call per set, over "qubits" (in order of first use)."""
    items = circuit_items(circuit)
    blocks: List[dict] = []
    gates: List[int] = []
    used: set = set()
    for i in range(len(items) - 1, -1, -1):
        _, p, qubits = items[i]
        if p is not None and used & set(qubits):
            blocks.append({"gates": gates[::-1]})
            gates, used = [], set()
        gates.append(i)
        used |= set(qubits)
    if gates:
        blocks.append({"gates": gates[::-1]})
    for block in blocks:
        passes: List[dict] = []
        for i in block["gates"]:
            _, p, qubits = items[i]
            if p is None:
                continue
            for ps in passes:
                if len(set(ps["qubits"]) | set(qubits)) <= MAX_GATE_QUBITS:
                    ps["qubits"] += [q for q in qubits if q not in ps["qubits"]]
                    ps["gates"].append(i)
                    break
            else:
                passes.append({"qubits": list(qubits), "gates": [i]})
        block["passes"] = passes
    return blocks


def reduce_transition(m: np.ndarray, set_qubits: Sequence[int], gate_qubits: Sequence[int]) -> np.ndarray:
    """The transition matrix of `gate_qubits` from the one of `set_qubits` (a superset): the partial trace over the other qubits,
    re-indexed from transition_matrix's convention (bit i of an index = set_qubits[i]) to a MatrixOp's (gate_qubits[0] = the most
    significant bit), so that <bra| A |ket> = trace(A @ result) for A on gate_qubits."""
    set_qubits, gate_qubits = list(set_qubits), list(gate_qubits)
    k = len(set_qubits)
    t = np.asarray(m, dtype=np.complex128).reshape((2,) * (2 * k))
    # reshape lists the most significant bit first: axis j of the row index is qubit set_qubits[k - 1 - j]
    letters = "abcdefghijklmnopqrstuvwxyz"
    row = {q: letters[j] for j, q in enumerate(reversed(set_qubits))}
    col = {q: (letters[k + j] if q in gate_qubits else row[q]) for j, q in enumerate(reversed(set_qubits))}
    spec = "".join(row[q] for q in reversed(set_qubits)) + "".join(col[q] for q in reversed(set_qubits)) + "->" + \
        "".join(row[q] for q in gate_qubits) + "".join(col[q] for q in gate_qubits)
    side = 1 << len(gate_qubits)
    return np.einsum(spec, t).reshape(side, side)
