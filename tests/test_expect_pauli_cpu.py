"""Expectation values of Pauli strings (include/qip_hipx.h), the parts that need no GPU: the tests' reference against dense
Kronecker-product matrices, the grouping into passes (qipx_expect_pauli_passes runs the grouping code of the device call), the
refusals, and a null handle (there is no CPU fall-back)."""
import ctypes as C

import numpy as np
import pytest

import expect_pauli_ref as E
import rustqip_amd as q
from rustqip_amd import _ffi

G = 16  # the default of state option "expect_group" (include/qip_hipx.h)
PAULI = {"I": np.eye(2), "X": np.array([[0, 1], [1, 0]]), "Y": np.array([[0, -1j], [1j, 0]]), "Z": np.diag([1, -1])}


def _dense(s):
    """the matrix of the string `s`: character q acts on qubit q, qubit 0 is the most significant index bit"""
    m = np.eye(1, dtype=np.complex128)
    for p in s:
        m = np.kron(m, PAULI[p])
    return m


def _state(n, dtype=np.complex128, norm=1.0):
    return E.make_state(n, E.seed_of(n, dtype), dtype, norm=norm)


# ---- the reference ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 2, 3, 4))
def test_reference_is_the_dense_quadratic_form(n):
    """every Pauli string on n <= 4 qubits — all single-qubit Paulis and every mixed string, n_Y = 0..4 — on a state of norm^2
    0.7 (the raw quadratic form), Complex<f64> and widened Complex<f32>"""
    for dtype in E.DTYPES:
        x = _state(n, dtype, norm=0.7)
        psi = x.astype(np.complex128)
        scale = float(np.vdot(psi, psi).real)
        for s in E.all_strings(n):
            want = np.vdot(psi, _dense(s) @ psi)
            assert abs(want.imag) <= 1e-15 * scale
            assert abs(E.expect_ref(n, E.term_of_string(s), x) - want.real) <= 1e-14 * scale, s


def test_reference_with_five_y_factors():
    """n_Y = 1..5 needs five qubits: Y on the first k qubits, X and Z beside them"""
    n = 5
    x = _state(n)
    for s in ("YIIII", "YYIXZ", "YYYZX", "YYYYX", "YYYYY", "ZYXYI", "IYZYY"):
        want = np.vdot(x, _dense(s) @ x)
        assert abs(E.expect_ref(n, E.term_of_string(s), x) - want.real) <= 1e-14, s
    assert E.masks(n, E.term_of_string("YYYYY")) == (31, 31, 5)
    assert E.masks(n, E.term_of_string("XIZIY")) == (0b10001, 0b00101, 1)
    assert E.term_of_masks(5, 0b10001, 0b00101) == E.term_of_string("XIZIY")
    assert abs(E.norm_sqr_ref(x) - E.expect_ref(n, {}, x)) <= 1e-15


# ---- passes -------------------------------------------------------------------------------------------------------------------
def _same_x(count, n=8):
    """`count` terms (Z factors varying) that share the x mask of X on qubit 2, Y on qubit 5"""
    terms = []
    for i in range(count):
        term = {2: "X", 5: "Y"}
        term.update({qb: "Z" for qb in range(n) if qb not in (2, 5) and (i + 1) >> (qb % 6) & 1})
        terms.append(term)
    return terms


@pytest.mark.parametrize("count,passes", ((1, 1), (G, 1), (G + 1, 2), (2 * G + 1, 3)))
def test_terms_of_one_x_mask_share_passes(count, passes):
    terms = _same_x(count)
    assert q.expect_pauli_passes(8, terms) == passes
    assert q.expect_pauli_passes(8, terms, G) == passes
    assert q.expect_pauli_passes(8, terms, 1) == count
    assert q.expect_pauli_passes(8, list(reversed(terms))) == passes


def test_distinct_x_masks_do_not_share_a_pass():
    n = 8
    xs = [{0: "X"}, {0: "Y"}, {1: "X"}, {0: "X", 1: "Y"}, {7: "X"}, {3: "Z"}, {}, {4: "Z", 5: "Z"}, "IIIIIIII", "XIIIIIIZ", "YZIIIIII"]
    # x masks: qubit 0 (terms 0, 1, 9, 10), qubit 1, qubits 0 + 1, qubit 7, and zero (terms 5 - 8: Z strings and empty terms)
    k = 5
    assert q.expect_pauli_passes(n, xs) == k
    assert q.expect_pauli_passes(n, xs, 1) == len(xs)  # an empty term is a term of x = 0 and takes a slot
    assert q.expect_pauli_passes(n, xs, 2) == 2 + 1 + 1 + 1 + 2
    interleaved = [t for pair in zip(_same_x(G + 1), [{1: "X", 3: "Z"}] * (G + 1)) for t in pair]
    assert q.expect_pauli_passes(n, interleaved) == 4
    assert q.expect_pauli_passes(n, []) == 0


def _raw(n, start, qubits, paulis, count, group=0, null=()):
    out = C.c_uint64(99)
    args = [(C.c_uint64 * len(start))(*start), (C.c_uint64 * max(len(qubits), 1))(*qubits), (C.c_uint8 * max(len(paulis), 1))(*paulis)]
    for i in null:
        args[i] = None
    return _ffi.lib.qipx_expect_pauli_passes(n, args[0], args[1], args[2], count, group, C.byref(out)), out.value


def test_refusals():
    ok = ([0, 2, 3], [0, 3, 1], [1, 3, 2])
    for group in (0, 1):
        assert _raw(4, *ok, 2, group) == (_ffi.QIP_OK, 2)
        for null in ((0,), (1,), (2,), (0, 1, 2)):
            assert _raw(4, *ok, 2, group, null=null)[0] == _ffi.QIP_ERR_INVALID
        assert _raw(4, [1, 2, 3], [0, 3, 1], [1, 3, 2], 2, group)[0] == _ffi.QIP_ERR_INVALID  # term_start[0] != 0
        assert _raw(4, [0, 2, 1], [0, 3, 1], [1, 3, 2], 2, group)[0] == _ffi.QIP_ERR_INVALID  # decreasing
        assert _raw(4, [0, 2, 3], [0, 4, 1], [1, 3, 2], 2, group)[0] == _ffi.QIP_ERR_INVALID  # qubit = n
        assert _raw(4, [0, 2, 3], [3, 3, 1], [1, 3, 2], 2, group)[0] == _ffi.QIP_ERR_INVALID  # repeated inside a term
        assert _raw(4, [0, 2, 3], [0, 3, 1], [1, 4, 2], 2, group)[0] == _ffi.QIP_ERR_INVALID  # code 4
        assert _raw(4, [0, 2, 3], [0, 3, 0], [1, 3, 2], 2, group) == (_ffi.QIP_OK, 2 if group else 1)  # the same qubit in two terms is fine (and the same x mask)
        assert _raw(4, [0], [], [], 0, group, null=(0, 1, 2)) == (_ffi.QIP_OK, 0)             # no terms: null arrays allowed
    assert _raw(4, *ok, 2, 33)[0] == _ffi.QIP_ERR_INVALID
    assert _raw(4, *ok, 2, 32) == (_ffi.QIP_OK, 2)
    assert _ffi.lib.qipx_expect_pauli_passes(4, None, None, None, 0, 0, None) == _ffi.QIP_ERR_INVALID  # null output
    _raw(4, [0, 2, 3], [0, 4, 1], [1, 3, 2], 2)
    assert "out of range" in _ffi.last_error()
    with pytest.raises(q.CircuitError):
        q.expect_pauli_passes(4, ["XXI"])
    with pytest.raises(q.CircuitError):
        q.expect_pauli_passes(4, [{0: "Q"}])
    with pytest.raises(q.CircuitError):
        q.expect_pauli_passes(4, [{4: "X"}])
    assert q.expect_pauli_passes(4, ["IIII", {0: "I", 2: "I"}, {}], 1) == 3  # terms of I factors only are the empty term


def test_expect_pauli_without_a_device_fails_loudly():
    """no CPU fall-back: without a device there is no handle, and a null handle is refused"""
    start = (C.c_uint64 * 2)(0, 1)
    qubits = (C.c_uint64 * 1)(0)
    paulis = (C.c_uint8 * 1)(3)
    out = (C.c_double * 1)()
    assert _ffi.lib.qipx_state_expect_pauli(None, start, qubits, paulis, 1, out) == _ffi.QIP_ERR_INVALID
    assert _ffi.lib.qipx_state_expect_pauli(None, None, None, None, 0, None) == _ffi.QIP_ERR_INVALID
