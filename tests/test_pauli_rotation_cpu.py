"""Pauli-string rotations (include/qip_hipx.h), the parts that need no GPU: the grouping into passes
(qipx_pauli_rotation_passes runs the grouping code of the device call), the refusals, a null handle (there is no CPU
fall-back), the tests' reference against dense Kronecker-product matrices, and the specified arithmetic restated in numpy held to
the two bars of tests/pauli_rotation_ref.py on the GPU tests' cases: the bars are meetable."""
import ctypes as C

import numpy as np
import pytest

import pauli_rotation_ref as P
import rustqip_amd as q
from rustqip_amd import _ffi

G = 16  # the default of state option "rotate_group" (include/qip_hipx.h)
PAULI = {"I": np.eye(2), "X": np.array([[0, 1], [1, 0]]), "Y": np.array([[0, -1j], [1j, 0]]), "Z": np.diag([1, -1])}


def _dense(s):
    """the matrix of the string `s`: character q acts on qubit q, qubit 0 is the most significant index bit"""
    m = np.eye(1, dtype=np.complex128)
    for p in s:
        m = np.kron(m, PAULI[p])
    return m


def _state(n, dtype=np.complex128, norm=1.0):
    return P.make_state(n, P.seed_of(n, dtype), dtype, norm=norm)


# ---- passes -------------------------------------------------------------------------------------------------------------------
def test_consecutive_terms_of_one_x_mask_share_passes():
    n = 6
    a, b = {0: "X", 3: "Y"}, {1: "X"}
    a2, a3 = {0: "Y", 3: "X", 4: "Z"}, {0: "X", 3: "X", 5: "Z"}  # the x mask of a, other z masks
    terms = [a, a2, b, a3, {2: "Z"}, {}, "IIIIIZ"]  # x masks [a, a, b, a, 0, 0, 0]
    assert [P.masks(n, P.term_of_string(t) if isinstance(t, str) else t)[0] for t in terms] == [36, 36, 16, 36, 0, 0, 0]
    assert q.pauli_rotation_passes(n, terms, 2) == 5
    assert q.pauli_rotation_passes(n, terms, 1) == 7
    assert q.pauli_rotation_passes(n, terms, 32) == 4
    assert q.pauli_rotation_passes(n, terms) == q.pauli_rotation_passes(n, terms, G)
    assert q.pauli_rotation_passes(n, [a] * (G + 1)) == 2 and q.pauli_rotation_passes(n, [a] * G) == 1  # group 0 is the default
    with pytest.raises(q.CircuitError):
        q.pauli_rotation_passes(n, terms, 33)
    assert q.pauli_rotation_passes(n, []) == 0
    # the order is kept: the terms are not sorted by mask (expect_pauli sorts: its terms commute with the sum)
    assert q.pauli_rotation_passes(n, [a, b] * 5, 32) == 10 and q.expect_pauli_passes(n, [a, b] * 5, 32) == 2


@pytest.mark.parametrize("n", (9, 13))
def test_passes_of_the_batch_case(n):
    terms, _ = P.batch_case(n)
    for group in (1, 4, 16, 32):
        assert q.pauli_rotation_passes(n, terms, group) == P.batch_passes(group)


def _raw(fn, n, start, qubits, paulis, count, group=0, null=()):
    out = C.c_uint64(99)
    args = [(C.c_uint64 * len(start))(*start), (C.c_uint64 * max(len(qubits), 1))(*qubits), (C.c_uint8 * max(len(paulis), 1))(*paulis)]
    for i in null:
        args[i] = None
    return fn(n, args[0], args[1], args[2], count, group, C.byref(out)), out.value


MALFORMED = (  # (start, qubits, paulis)
    ([1, 2, 3], [0, 3, 1], [1, 3, 2]),  # term_start[0] != 0
    ([0, 2, 1], [0, 3, 1], [1, 3, 2]),  # decreasing
    ([0, 2, 3], [0, 4, 1], [1, 3, 2]),  # qubit = n
    ([0, 2, 3], [3, 3, 1], [1, 3, 2]),  # repeated inside a term
    ([0, 2, 3], [0, 3, 1], [1, 4, 2]),  # code 4
)


def test_refuses_what_expect_pauli_passes_refuses():
    rot, exp = _ffi.lib.qipx_pauli_rotation_passes, _ffi.lib.qipx_expect_pauli_passes
    ok = ([0, 2, 3], [0, 3, 1], [1, 3, 2])
    for group in (0, 1):
        assert _raw(rot, 4, *ok, 2, group) == (_ffi.QIP_OK, 2)
        for null in ((0,), (1,), (2,), (0, 1, 2)):
            assert _raw(exp, 4, *ok, 2, group, null=null)[0] == _ffi.QIP_ERR_INVALID
            assert _raw(rot, 4, *ok, 2, group, null=null)[0] == _ffi.QIP_ERR_INVALID
        for bad in MALFORMED:
            assert _raw(exp, 4, *bad, 2, group)[0] == _ffi.QIP_ERR_INVALID
            message = _ffi.last_error()
            assert message.startswith("expect_pauli: ")
            assert _raw(rot, 4, *bad, 2, group)[0] == _ffi.QIP_ERR_INVALID
            # the same check, the same text, under the name of the call it came from
            assert _ffi.last_error() == "pauli_rotations: " + message[len("expect_pauli: "):]
        assert _raw(rot, 4, [0, 2, 3], [0, 3, 0], [1, 3, 2], 2, group) == (_ffi.QIP_OK, 2 if group else 1)  # the same qubit in two terms is fine
        assert _raw(rot, 4, [0], [], [], 0, group, null=(0, 1, 2)) == (_ffi.QIP_OK, 0)  # no terms: null arrays allowed
    assert _raw(rot, 4, *ok, 2, 33)[0] == _ffi.QIP_ERR_INVALID
    assert _raw(rot, 4, *ok, 2, 32) == (_ffi.QIP_OK, 2)
    assert rot(4, None, None, None, 0, 0, None) == _ffi.QIP_ERR_INVALID  # null output
    for bad in (["XXI"], [{0: "Q"}], [{4: "X"}]):
        with pytest.raises(q.CircuitError):
            q.pauli_rotation_passes(4, bad)
    assert q.pauli_rotation_passes(4, ["IIII", {0: "I", 2: "I"}, {}], 1) == 3  # terms of I factors only are the empty term


def test_rotations_without_a_device_fail_loudly():
    """no CPU fall-back: without a device there is no handle, and a null handle is refused"""
    start = (C.c_uint64 * 2)(0, 1)
    qubits = (C.c_uint64 * 1)(0)
    paulis = (C.c_uint8 * 1)(3)
    angles = (C.c_double * 1)(0.5)
    call = _ffi.lib.qipx_state_apply_pauli_rotations
    assert call(None, start, qubits, paulis, angles, 1) == _ffi.QIP_ERR_INVALID
    assert call(None, None, None, None, None, 0) == _ffi.QIP_ERR_INVALID
    assert q.ext_abi_version() == 1


# ---- the reference ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 2, 3))
def test_reference_is_the_dense_exponential(n):
    """every Pauli string on n <= 3 qubits against cos theta I - i sin theta P built by Kronecker products, at the sequence bar
    with R = 1 (both sides are complex128 arithmetic)"""
    x = _state(n, norm=0.7)
    for s in P.all_strings(n):
        for theta in (0.3, -2.5):
            want = (np.cos(theta) * np.eye(1 << n) - 1j * np.sin(theta) * _dense(s)) @ x
            ok, worst = P.within_sequence_bar(1, P.rotate_ref(n, P.term_of_string(s), theta, x), want, x)
            assert ok, (s, theta, worst)


def test_reference_is_unitary_and_ordered():
    n = 4
    x = _state(n)
    t1, t2 = {0: "X"}, {0: "Z"}
    a = P.rotate_many_ref(n, [t1, t2], [0.6, 0.6], x)
    b = P.rotate_many_ref(n, [t2, t1], [0.6, 0.6], x)
    assert abs(np.linalg.norm(a) - 1.0) <= 1e-15 and np.linalg.norm(a - b) > 0.1
    back = P.rotate_ref(n, {1: "Y", 3: "Z"}, -0.9, P.rotate_ref(n, {1: "Y", 3: "Z"}, 0.9, x))
    assert np.linalg.norm(back - x) <= 1e-15


# ---- the bars are meetable ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", P.DTYPES, ids=("c128", "c64"))
def test_specified_arithmetic_meets_both_bars(dtype):
    """the precision-P restatement on the GPU tests' cases: every string at n = 1, 2, 3; the single rotations of n = 9 and 13 on
    both norms; the 67-term batch of n = 9 and 13"""
    worst_el = worst_seq = 0.0
    for n in (1, 2, 3):
        x = _state(n, dtype)
        for s in P.all_strings(n):
            for theta in (0.3, -2.5):
                t = P.term_of_string(s)
                ok, w = P.within_element_bar(n, t, P.rotate_spec(n, t, theta, x), P.rotate_ref(n, t, theta, x), x)
                assert ok, (n, s, theta, w)
                worst_el = max(worst_el, w)
    for n in (9, 13):
        for norm in (1.0, 0.5):
            x = _state(n, dtype, norm)
            for name, t, theta in P.single_cases(n):
                ok, w = P.within_element_bar(n, t, P.rotate_spec(n, t, theta, x), P.rotate_ref(n, t, theta, x), x)
                assert ok, (n, name, theta, w)
                worst_el = max(worst_el, w)
        x = _state(n, dtype)
        terms, angles = P.batch_case(n)
        ok, w = P.within_sequence_bar(len(terms), P.rotate_many_spec(n, terms, angles, x), P.rotate_many_ref(n, terms, angles, x), x)
        assert ok, (n, w)
        worst_seq = max(worst_seq, w)
    print(f"{np.dtype(dtype).name}: worst element error {worst_el:.2f} u (|psi_j| + |psi_jx|), worst sequence error {worst_seq:.3f} R u |psi|; bar {P.BAR}")
    assert {theta for n in (9, 13) for _, _, theta in P.single_cases(n)} == set(P.ANGLES)
