"""The quantum Fourier transform of a qubit register of a device state and the algorithms it closes, each a thin call of
HipState.apply_qft (include/qip_hipx.h: qipx_state_apply_qft): no kernels of its own.

A register is a sequence of qubits, least significant bit first: bit i of the register's value is the bit of qubit reg[i]."""
from __future__ import annotations

import cmath
import math
from typing import List, Sequence

import numpy as np

from . import classical
from .circuits import H
from .ops import CircuitError, MatrixOp, make_control_op, make_matrix_op, make_swap_op
from .state import HipState


def qft(st: HipState, reg: Sequence[int], reversed: bool = False) -> None:
    """|x> -> 2^(-m/2) sum_y exp(+2 pi i x y / 2^m) |y> on `reg`; `reversed` leaves y with its bits in reversed order"""
    st.apply_qft(reg, inverse=False, reversed=reversed)


def iqft(st: HipState, reg: Sequence[int], reversed: bool = False) -> None:
    """the inverse of qft; with `reversed` it reads the register in the order qft(.., reversed=True) leaves it"""
    st.apply_qft(reg, inverse=True, reversed=reversed)


def qft_ops(reg: Sequence[int], inverse: bool = False, reversed: bool = False) -> List[MatrixOp]:
    """The same transform lowered to m Hadamards, m(m-1)/2 controlled phases and m/2 swaps for any register (circuits.c3_qft
    is qft_ops(range(n)[::-1])): what apply_qft is tested and measured against through apply_ops.  `reversed` omits the swaps."""
    reg = [int(q) for q in reg]
    m = len(reg)
    if len(set(reg)) != m:
        raise CircuitError("qft_ops: a qubit is repeated")
    sign = -1.0 if inverse else 1.0
    ops: List[MatrixOp] = []
    for r in range(m - 1, -1, -1):
        ops.append(make_matrix_op([reg[r]], H))
        for lower in range(r - 1, -1, -1):
            ph = cmath.rect(1.0, sign * math.pi / (1 << (r - lower)))
            ops.append(make_control_op([reg[lower]], make_matrix_op([reg[r]], [1, 0, 0, ph])))
    swaps = [] if reversed else [make_swap_op([reg[r]], [reg[m - 1 - r]]) for r in range(m // 2)]
    # (every gate above is symmetric, so the inverse is the conjugated gates in the opposite order)
    return swaps + ops[::-1] if inverse else ops + swaps


def phase_estimation_readout(st: HipState, counting: Sequence[int], shots: int, seed: int, reversed: bool = False) -> np.ndarray:
    """The last step of phase estimation: the inverse transform of the counting register, then `shots` samples of its value
    (HipState.sample: the state keeps the transformed amplitudes).  `reversed`: the register holds its phases in the order
    qft(.., reversed=True) leaves them, and the inverse needs no bit reversal."""
    iqft(st, counting, reversed=reversed)
    return st.sample(list(counting), shots, seed)


def order_finding(st: HipState, counting: Sequence[int], work: Sequence[int], base: int, modulus: int) -> None:
    """Shor's order-finding circuit on a state whose counting and work registers read 0: Hadamards on the counting register,
    |x>|0> -> |x>|base^x mod modulus> by table (classical.exp_mod_into), the inverse transform of the counting register.
    measure_probs(counting) then peaks at the multiples of 2^m / r for the order r of `base`."""
    if math.gcd(int(base), int(modulus)) != 1:
        raise CircuitError(f"order_finding: {base} and {modulus} are not coprime")
    st.apply_ops([make_matrix_op([int(q)], H) for q in counting])
    classical.exp_mod_into(st, counting, work, base, modulus)
    iqft(st, counting)
