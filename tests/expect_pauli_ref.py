"""A reference for expectation values of Pauli strings, independent of the code under test, and the terms the tests run —
shared by tests/test_expect_pauli_cpu.py and tests/test_gpu_f1_expect_pauli.py.  A plain helper module: numpy only, no fixtures.

A term is a mapping {qubit: "I" | "X" | "Y" | "Z"}; qubit q is amplitude-index bit n - 1 - q.  With x = the index bits under X
or Y, z = those under Z or Y and n_Y the number of Y factors,

    <psi|P|psi> = sum_j conj(psi[j ^ x]) * i^n_Y * (-1)^popcount(j & z) * psi[j].

The 2^n products are formed in complex128 from the amplitudes widened to double, and their real parts are summed with
math.fsum (the imaginary parts cancel pair by pair).  The states are those of tests/measure_ref.py."""
import math

import numpy as np

from measure_ref import DTYPES, make_state, seed_of  # noqa: F401  (the deterministic states the measurement tests share)

CODES = {"I": 0, "X": 1, "Y": 2, "Z": 3}


def masks(n, term):
    """(x, z, n_Y) of a term"""
    x = z = ny = 0
    for qb, p in term.items():
        bit = 1 << (n - 1 - int(qb))
        assert 0 <= int(qb) < n and p in CODES
        if p in "XY":
            x |= bit
        if p in "ZY":
            z |= bit
        ny += p == "Y"
    return x, z, ny


_PARITY16 = None


def parity(v):
    """popcount mod 2 of every element (values below 2^48), through a table of the 16-bit parities"""
    global _PARITY16
    if _PARITY16 is None:
        t = np.arange(1 << 16, dtype=np.uint32)
        for s in (8, 4, 2, 1):
            t ^= t >> s
        _PARITY16 = (t & 1).astype(np.int8)
    v = np.asarray(v, dtype=np.int64)
    assert v.size == 0 or (0 <= int(v.min()) and int(v.max()) < 1 << 48)
    return (_PARITY16[v & 0xFFFF] ^ _PARITY16[(v >> 16) & 0xFFFF] ^ _PARITY16[v >> 32]).astype(np.int64)


_INDEX = {}


def _indices(n):
    if n not in _INDEX:
        _INDEX.clear()  # (one size at a time: 2^22 indices are 32 MiB)
        _INDEX[n] = np.arange(1 << n, dtype=np.int64)
    return _INDEX[n]


def expect_ref(n, term, amps):
    """<psi|P|psi> of one term on the state `amps` (complex64 or complex128), exactly rounded sum of double products"""
    x, z, ny = masks(n, term)
    psi = np.asarray(amps).astype(np.complex128)
    j = _indices(n)
    sign = 1.0 - 2.0 * parity(j & z)
    prod = np.conj(psi[j ^ x]) * ((1j) ** (ny % 4)) * sign * psi
    return math.fsum(prod.real)


def expect_ref_many(n, terms, amps):
    return np.array([expect_ref(n, t, amps) for t in terms], dtype=np.float64)


def term_of_masks(n, x, z):
    """the term with X on x & ~z, Z on z & ~x and Y on x & z (masks over amplitude-index bits)"""
    term = {}
    for b in range(n):
        bx, bz = (x >> b) & 1, (z >> b) & 1
        if bx or bz:
            term[n - 1 - b] = "Y" if bx and bz else ("X" if bx else "Z")
    return term


def term_of_string(s):
    """character q of `s` acts on qubit q"""
    return {qb: p for qb, p in enumerate(s) if p != "I"}


def all_strings(n):
    out = [""]
    for _ in range(n):
        out = [s + p for s in out for p in "IXYZ"]
    return out


def norm_sqr_ref(amps):
    psi = np.asarray(amps).astype(np.complex128)
    return math.fsum((psi.real * psi.real).tolist() + (psi.imag * psi.imag).tolist())


def mask_cases(n):
    """the masks of the one-block / several-block tests as (name, x, z): x = 0 with z empty, bit 0, the top bit, all bits; x = bit
    0 alone (inside a packed Complex<f32> element), the top bit alone, all bits; x and z overlapping with n_Y = 1..5"""
    top, full = 1 << (n - 1), (1 << n) - 1
    cases = [("z_empty", 0, 0), ("z_bit0", 0, 1), ("z_top", 0, top), ("z_all", 0, full),
             ("x_bit0", 1, 0), ("x_top", top, 0), ("x_all", full, 0)]
    spread = [0, n - 1, 3, n - 3, 5]  # the index bits that carry the Y factors: bit 0, the top bit, some between
    for ny in range(1, 6):
        y = sum(1 << b for b in spread[:ny])
        # Y on `y` (bit 0 among them: x's bit 0 set), X on bit 1, Z on bit 2 and bit n - 2
        cases.append((f"ny{ny}", y | 2, y | 4 | (1 << (n - 2))))
        # and the same with bit 0 left alone: x's bit 0 clear (the packed Complex<f32> pair pass), Y factors from bit n - 1 down
        y2 = sum(1 << b for b in range(n - 1, n - 1 - ny, -1))
        cases.append((f"ny{ny}_x0clear", y2 | 2, y2 | 1 | 4))
    return cases
