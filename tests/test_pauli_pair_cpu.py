"""The two-state Pauli calls and the adjoint gradient (include/qip_hipx.h), the parts that need no GPU: the tests' references
against each other and against finite differences, the grouping into passes (qipx_pauli_sum_passes runs the grouping code of
the device call), the refusals of that host-only call, null handles (there is no CPU fall-back), and the specified arithmetic of
the Pauli sum restated in numpy held to the element bar of tests/pauli_pair_ref.py: the bar is meetable."""
import ctypes as C

import numpy as np
import pytest

import expect_pauli_ref as E
import pauli_pair_ref as P
import rustqip_amd as q
from rustqip_amd import _ffi

G = 16  # the default of state option "sum_group" (include/qip_hipx.h)


def _state(n, dtype=np.complex128, norm=1.0, salt=0):
    return P.make_state(n, P.seed_of(n, dtype) + salt, dtype, norm=norm)


# ---- the references -------------------------------------------------------------------------------------------------------------
def test_adjoint_gradient_ref_agrees_with_central_differences():
    """n = 4, T = 6, step h = 1e-5.  As a function of one angle, E = a + A cos(2 theta + phi) with |A| <= S ||psi||^2
    (S = sum |c_t| bounds the norm of H), so |E'''| <= 8 S ||psi||^2 and the central difference (E(theta + h) - E(theta - h)) / 2h
    errs by at most h^2 / 6 * 8 S ||psi||^2: that remainder is the bar.  The energies of the difference are formed in long double,
    whose rounding — (24 T + count + 8) eps S ||psi||^2 per energy by the bound of pauli_pair_ref, divided by h — is added to the
    bar as it is: three orders below the remainder where long double is the x87 format."""
    n, T, h = 4, 6, 1e-5
    rng = np.random.default_rng(404)
    rot = [P.term_of_string("".join(rng.choice(list("IXYZ"), n))) for _ in range(T)]
    rot[2] = P.term_of_masks(n, P.masks(n, rot[1])[0], 0b0110)  # two consecutive strings of one x mask
    rot[4] = {1: "Z", 3: "Z"}
    angles = rng.uniform(-3.0, 3.0, T)
    obs = [P.term_of_string("".join(rng.choice(list("IXYZ"), n))) for _ in range(4)] + [{}]
    coeffs = rng.standard_normal(len(obs))
    psi0 = _state(n, norm=0.8)
    S, norm2 = float(np.sum(np.abs(coeffs))), float(np.linalg.norm(psi0)) ** 2
    energy, grad = P.adjoint_gradient_ref(n, rot, angles, obs, coeffs, psi0)
    eps = float(np.finfo(np.longdouble).eps)
    bar = h * h / 6 * 8 * S * norm2 + (24 * T + len(obs) + 8) * eps * S * norm2 / h
    wide = lambda a: P.energy_ref(n, rot, a, obs, coeffs, psi0, np.clongdouble)  # noqa: E731
    assert abs(float(wide(angles)) - energy) <= (24 * T + len(obs) + 8) * 2.0 ** -53 * S * norm2
    for k in range(T):
        step = np.zeros(T)
        step[k] = h
        fd = float((wide(angles + step) - wide(angles - step)) / (2 * np.longdouble(h)))
        print(f"angle {k}: adjoint {grad[k]:+.12f}, central difference {fd:+.12f}, apart {abs(fd - grad[k]):.3e}, bar {bar:.3e}")
        assert abs(fd - grad[k]) <= bar, k
    assert np.max(np.abs(grad)) > 1e3 * bar  # (the gradient is not small against the bar)


@pytest.mark.parametrize("dtype", P.DTYPES, ids=("c128", "c64"))
def test_matrix_element_ref_on_one_state_is_expect_ref(dtype):
    n = 7
    psi = _state(n, dtype, 0.5)
    for name, cx, cz in E.mask_cases(n):
        term = P.term_of_masks(n, cx, cz)
        got = P.matrix_element_ref(n, term, psi, psi)
        want = E.expect_ref(n, term, psi)
        # the same 2^n products summed exactly, but formed in another order (conj(psi_j) (P psi)_j here, conj(psi_{j^x}) psi_j
        # there): a complex product errs by at most sqrt(8) u |psi_j| |psi_{j^x}|, on either side, and sum_j |psi_j| |psi_{j^x}| <=
        # norm^2 = 0.5 by Cauchy-Schwarz: 6 u norm^2
        assert abs(got.real - want) <= 6 * 2.0 ** -53 * 0.5 and abs(got.imag) <= 6 * 2.0 ** -53 * 0.5, name


def test_pauli_sum_ref_against_dense_matrices():
    n = 3
    pauli = {"I": np.eye(2), "X": np.array([[0, 1], [1, 0]]), "Y": np.array([[0, -1j], [1j, 0]]), "Z": np.diag([1, -1])}
    psi, phi = _state(n), _state(n, salt=1)
    for s in P.all_strings(n):
        m = np.eye(1)
        for p in s:
            m = np.kron(m, pauli[p])
        assert np.allclose(P.apply_term(n, P.term_of_string(s), psi), m @ psi, atol=1e-15), s
        assert abs(P.matrix_element_ref(n, P.term_of_string(s), phi, psi) - np.vdot(phi, m @ psi)) <= 1e-15, s


# ---- passes -------------------------------------------------------------------------------------------------------------------
def test_terms_of_one_x_mask_share_passes_wherever_they_stand():
    n = 6
    a, b = {0: "X", 3: "Y"}, {1: "X"}
    a2, a3 = {0: "Y", 3: "X", 4: "Z"}, {0: "X", 3: "X", 5: "Z"}  # the x mask of a, other z masks
    terms = [a, a2, b, a3, {2: "Z"}, {}, "IIIIIZ"]  # x masks [a, a, b, a, 0, 0, 0]: runs of 3 (a), 1 (b), 3 (zero) once sorted
    assert q.pauli_sum_passes(n, terms, 2) == 2 + 1 + 2
    assert q.pauli_sum_passes(n, terms, 1) == 7
    assert q.pauli_sum_passes(n, terms, 32) == 3
    assert q.pauli_sum_passes(n, terms) == q.pauli_sum_passes(n, terms, G) == 3
    assert q.pauli_sum_passes(n, [a] * (G + 1)) == 2 and q.pauli_sum_passes(n, [a] * G) == 1  # group 0 is the default
    assert q.pauli_sum_passes(n, [a] * 33, 32) == 2 and q.pauli_sum_passes(n, [a] * 65, 32) == 3  # a run longer than 32
    assert q.pauli_sum_passes(n, [a, b] * 5, 32) == 2  # sorted, unlike the rotations: the terms of a sum commute
    assert q.pauli_sum_passes(n, [{}]) == 1 and q.pauli_sum_passes(n, [{}, "ZIIIII", {}], 2) == 2  # the empty term is x = 0
    assert q.pauli_sum_passes(n, []) == 0
    with pytest.raises(q.CircuitError):
        q.pauli_sum_passes(n, terms, 33)


@pytest.mark.parametrize("n", (9, 13))
def test_passes_of_the_batch_case(n):
    terms, _ = P.batch_case(n)
    for group in (1, 4, 16, 32):
        assert q.pauli_sum_passes(n, terms, group) == P.batch_passes(group) == len(P.sum_plan(n, terms, group))


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
    fn, exp = _ffi.lib.qipx_pauli_sum_passes, _ffi.lib.qipx_expect_pauli_passes
    ok = ([0, 2, 3], [0, 3, 1], [1, 3, 2])
    for group in (0, 1):
        assert _raw(fn, 4, *ok, 2, group) == (_ffi.QIP_OK, 2)
        for null in ((0,), (1,), (2,), (0, 1, 2)):
            assert _raw(fn, 4, *ok, 2, group, null=null)[0] == _ffi.QIP_ERR_INVALID
        for bad in MALFORMED:
            assert _raw(exp, 4, *bad, 2, group)[0] == _ffi.QIP_ERR_INVALID
            message = _ffi.last_error()
            assert message.startswith("expect_pauli: ")
            assert _raw(fn, 4, *bad, 2, group)[0] == _ffi.QIP_ERR_INVALID
            # the same check, the same text, under the name of the call it came from
            assert _ffi.last_error() == "pauli_sum: " + message[len("expect_pauli: "):]
        assert _raw(fn, 4, [0], [], [], 0, group, null=(0, 1, 2)) == (_ffi.QIP_OK, 0)  # no terms: null arrays allowed
    assert _raw(fn, 4, *ok, 2, 33)[0] == _ffi.QIP_ERR_INVALID
    assert _raw(fn, 4, *ok, 2, 32) == (_ffi.QIP_OK, 2)
    assert fn(4, None, None, None, 0, 0, None) == _ffi.QIP_ERR_INVALID  # null output
    for bad in (["XXI"], [{0: "Q"}], [{4: "X"}]):
        with pytest.raises(q.CircuitError):
            q.pauli_sum_passes(4, bad)


def test_without_a_device_both_calls_fail_loudly():
    """no CPU fall-back: without a device there is no handle, and a null handle is refused"""
    start, qubits, paulis = (C.c_uint64 * 2)(0, 1), (C.c_uint64 * 1)(0), (C.c_uint8 * 1)(3)
    coeffs, values = (C.c_double * 2)(1.0, 0.0), (C.c_double * 2)(7.0, 7.0)
    assert _ffi.lib.qipx_state_apply_pauli_sum(None, None, start, qubits, paulis, coeffs, 1, 0) == _ffi.QIP_ERR_INVALID
    assert _ffi.last_error()
    assert _ffi.lib.qipx_state_apply_pauli_sum(None, None, None, None, None, None, 0, 1) == _ffi.QIP_ERR_INVALID
    assert _ffi.lib.qipx_state_pauli_matrix_elements(None, None, start, qubits, paulis, 1, values) == _ffi.QIP_ERR_INVALID
    assert _ffi.last_error() and list(values) == [7.0, 7.0]
    assert _ffi.lib.qipx_state_pauli_matrix_elements(None, None, None, None, None, 0, None) == _ffi.QIP_ERR_INVALID


# ---- the specified arithmetic meets the bar ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (9, 13))
@pytest.mark.parametrize("dtype", P.DTYPES, ids=("c128", "c64"))
def test_the_specified_arithmetic_stays_inside_the_element_bar(dtype, n):
    src, old = _state(n, dtype), _state(n, dtype, 0.5, salt=1)
    rng = np.random.default_rng(9)
    worst = 0.0
    for name, cx, cz in P.mask_cases(n):
        terms, coeffs = [P.term_of_masks(n, cx, cz)], rng.standard_normal(1) + 1j * rng.standard_normal(1)
        ok, w = P.within_bar(P.pauli_sum_spec(n, terms, coeffs, src), P.pauli_sum_ref(n, terms, coeffs, src), P.sum_bar(n, terms, coeffs, src))
        assert ok, name
        worst = max(worst, w)
    print(f"n={n} single terms: worst {worst * 9:.2f} u scale, bar 9")
    terms, coeffs = P.batch_case(n)
    for group in (1, 4, 16, 32):
        for dst_old in (None, old):
            got = P.pauli_sum_spec(n, terms, coeffs, src, dst_old, group)
            ok, w = P.within_bar(got, P.pauli_sum_ref(n, terms, coeffs, src, dst_old), P.sum_bar(n, terms, coeffs, src, dst_old))
            print(f"n={n} batch group={group} accumulate={dst_old is not None}: worst {w * 75:.2f} u scale, bar 75")
            assert ok, (group, dst_old is not None)
    assert np.array_equal(P.pauli_sum_spec(n, [], [], src, old), old) and not np.any(P.pauli_sum_spec(n, [], [], src))
