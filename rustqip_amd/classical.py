"""Classical reversible arithmetic on qubit registers of a device state, each a thin call of HipState.apply_function
(include/qip_hipx.h: qipx_state_apply_function): no Toffoli networks, no carry or scratch qubits, no kernels of its own.

A register is a sequence of qubits, least significant bit first: bit i of the register's value is the bit of qubit reg[i]."""
from __future__ import annotations

from typing import Sequence

import numpy as np

from .ops import CircuitError
from .state import HipState


def _same_width(a: Sequence[int], b: Sequence[int], what: str) -> None:
    if len(a) != len(b):
        raise CircuitError(f"{what}: registers of {len(a)} and {len(b)} qubits")


def copy(st: HipState, a: Sequence[int], b: Sequence[int]) -> None:
    """|a>|b> -> |a>|a ^ b>"""
    _same_width(a, b, "copy")
    st.apply_function(a, b, values=lambda x: x, mode="xor")


def add(st: HipState, a: Sequence[int], b: Sequence[int]) -> None:
    """|a>|b> -> |a>|(a + b) mod 2^k>, k = len(b) >= len(a)"""
    if len(a) > len(b):
        raise CircuitError(f"add: a register of {len(a)} qubits into one of {len(b)}")
    st.apply_function(a, b, values=lambda x: x, mode="add")


def add_const(st: HipState, b: Sequence[int], c: int, controls: Sequence[int] = ()) -> None:
    """|b> -> |(b + c) mod 2^k> where every qubit of `controls` reads 1"""
    k, nc = len(b), len(controls)
    c = int(c) % (1 << k) if k else 0
    st.apply_function(controls, b, values=lambda x: np.where(x == np.uint64((1 << nc) - 1), np.uint64(c), np.uint64(0)), mode="add")


def exp_mod_into(st: HipState, x: Sequence[int], out: Sequence[int], base: int, modulus: int) -> None:
    """|x>|y> -> |x>|y ^ (base^x mod modulus)>"""
    if modulus < 1 or (modulus - 1) >> len(out):
        raise CircuitError(f"exp_mod_into: residues modulo {modulus} do not fit {len(out)} qubits")
    table = np.empty(1 << len(x), dtype=np.uint64)
    v = 1 % modulus
    for i in range(len(table)):  # (Python integers: no overflow for any modulus)
        table[i] = v
        v = v * base % modulus
    st.apply_function(x, out, values=table, mode="xor")


def phase_oracle(st: HipState, reg: Sequence[int], marked, phi: float = np.pi) -> None:
    """|x> -> e^{i phi} |x> for every x in `marked` (an iterable of register values, or a callable on the array of all values
    that returns a mask), every other x unchanged"""
    size = 1 << len(reg)
    if callable(marked):
        mask = np.asarray(marked(np.arange(size, dtype=np.uint64)), dtype=bool)
    else:
        mask = np.zeros(size, dtype=bool)
        for v in marked:
            if not 0 <= int(v) < size:
                raise CircuitError(f"phase_oracle: {v} is not a value of a register of {len(reg)} qubits")
            mask[int(v)] = True
    st.apply_function(reg, (), phases=np.where(mask, float(phi), 0.0))
