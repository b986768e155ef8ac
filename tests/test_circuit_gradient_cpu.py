"""Host side of HipState.circuit_gradient, no GPU: the planner (parametric.gradient_plan), inverse_op through the CPU oracle, the
parametrised gates, the argument checks that need no device, and a numpy emulation of the driver (tests/circuit_gradient_ref.py)
held to the bars the GPU tests use, on the circuits the GPU tests use."""
import numpy as np
import pytest

import circuit_gradient_ref as R
import rustqip_amd as q
from rustqip_amd import parametric as G

S = np.sqrt(0.5)


def _cnot(c, t):
    return q.make_control_op([c], q.make_matrix_op([t], [0, 1, 1, 0]))


def _plan(circuit):
    return [(b["gates"], [(p["qubits"], p["gates"]) for p in b["passes"]]) for b in G.gradient_plan(circuit)]


# ---- the planner ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 3, 4, 7))
def test_plan_layer_of_single_qubit_gates(n):
    plan = _plan([(G.ry(qb), qb) for qb in range(n)])
    assert len(plan) == 1 and plan[0][0] == list(range(n))
    assert len(plan[0][1]) == -(-n // 3)
    assert plan[0][1] == [(list(range(s, min(s + 3, n))), list(range(s, min(s + 3, n)))) for s in range(0, n, 3)]


def test_plan_parametrised_gate_under_a_later_fixed_gate_closes_the_block():
    # ry(0), then CNOT(0, 1): A of the ry does not commute with the CNOT, which is already in the block when the walk meets it
    plan = _plan([(G.ry(0), 0), _cnot(0, 1), (G.rz(2), 1)])
    assert plan == [([1, 2], [([2], [2])]), ([0], [([0], [0])])]


def test_plan_fixed_gate_under_a_later_parametrised_gate_joins():
    plan = _plan([_cnot(0, 1), (G.ry(0), 0), (G.ry(1), 1)])
    assert plan == [([0, 1, 2], [([0, 1], [1, 2])])]


def test_plan_shared_parameter_and_first_fit():
    # two layers on qubits 0..3 with one parameter each; controls count as qubits; first-fit fills an earlier set when it can
    circuit = [(G.ry(0), 0), (G.ry(1), 0), (G.rz(3, controls=[2]), 1), (G.rx(4), 2), (G.ry(0), 0)]
    plan = _plan(circuit)
    assert plan == [([1, 2, 3, 4], [([1, 2, 3], [1, 2]), ([4, 0], [3, 4])]), ([0], [([0], [0])])]
    assert _plan([]) == [] and _plan([_cnot(0, 1)]) == [([0], [])]


def test_plan_refusals():
    with pytest.raises(q.CircuitError, match="4 qubits"):
        G.gradient_plan([(G.rzz(0, 1, controls=[2, 3]), 0)])
    for bad in ([(G.ry(0), -1)], [(G.ry(0), 0.5)], [("ry", 0)], [G.ry(0)], [(G.ry(0), True)]):
        with pytest.raises(q.CircuitError):
            G.gradient_plan(bad)
    with pytest.raises(q.CircuitError):
        G.rzz(1, 1)
    with pytest.raises(q.CircuitError):
        G.generator_gate([0], [[0, 1], [2, 0]])  # not Hermitian


# ---- inverse_op -------------------------------------------------------------------------------------------------------------------
def _op_cases():
    rng = np.random.default_rng(11)
    u2, u4 = R._random_unitary(rng, 4), R._random_unitary(rng, 16)
    sparse = q.make_sparse_matrix_op([1, 3], [[(0, 1.0)], [(1, S), (2, 1j * S)], [(1, 1j * S), (2, S)], [(3, -1.0)]])
    perm = q.make_sparse_matrix_op([4, 0], [[(2, 1j)], [(0, -1.0)], [(3, 1.0)], [(1, -1j)]])
    return {
        "x": (q.make_matrix_op([2], [0, 1, 1, 0]), True),
        "y": (q.make_matrix_op([0], [0, -1j, 1j, 0]), True),
        "dense2": (q.make_matrix_op([3, 1], u2), False),
        "dense4": (q.make_matrix_op([4, 0, 2, 1], u4), False),
        "sparse": (sparse, False),
        "sparse_perm": (perm, True),
        "swap": (q.make_swap_op([0, 1], [3, 4]), True),
        "cnot": (_cnot(4, 0), True),
        "controlled_dense": (q.make_control_op([2], q.make_matrix_op([3, 1], u2)), False),
        "controlled_swap": (q.make_control_op([2], q.make_swap_op([0], [4])), True),
        "nested": (q.make_control_op([0], q.make_control_op([4], q.make_matrix_op([2], [S, S, S, -S]))), False),
        "nested_sparse": (q.make_control_op([2], q.make_control_op([0], perm.__class__("SparseMatrix", [4, 1], rows=perm.rows))), True),
    }


@pytest.mark.parametrize("name", sorted(_op_cases()))
@pytest.mark.parametrize("dtype", (np.complex128, np.complex64), ids=("c128", "c64"))
def test_inverse_op_undoes_the_op(name, dtype, oracle):
    """inverse_op after op through the CPU oracle is the identity on a random state: exact for 0 / +-1 / +-i matrices, within
    2 gamma u ||x|| (tests/circuit_gradient_ref.py) otherwise"""
    n = 5
    op, exact = _op_cases()[name]
    inv = q.inverse_op(op)
    assert inv.kind == op.kind and inv.indices == op.indices and q.inverse_op(inv).kind == op.kind
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)).astype(dtype)
    mid, back = np.zeros_like(x), np.zeros_like(x)
    oracle.apply_op_overwrite(n, op, x, mid)
    oracle.apply_op_overwrite(n, inv, mid, back)
    err = float(np.linalg.norm(back.astype(np.complex128) - x.astype(np.complex128)))
    bar = 0.0 if exact else 2 * R.op_gamma(op) * R.unit_roundoff(dtype) * float(np.linalg.norm(x.astype(np.complex128)))
    print(f"{name}: |back - x| = {err:.3e}, bar {bar:.3e}")
    assert err <= bar
    assert np.allclose(R.op_matrix(inv) @ R.op_matrix(op), np.eye(1 << len(op.indices)), atol=1e-14)


# ---- the gates --------------------------------------------------------------------------------------------------------------------
def _gates():
    rng = np.random.default_rng(5)
    h = rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4))
    return {"rx": G.rx(0), "ry": G.ry(1), "rz": G.rz(2), "phase": G.phase(0), "rxx": G.rxx(0, 1), "ryy": G.ryy(1, 0), "rzz": G.rzz(2, 0),
            "pauli1": G.pauli_rotation({1: "Y"}), "pauli3": G.pauli_rotation({2: "X", 0: "Y", 1: "Z", 3: "I"}),
            "generator": G.generator_gate([1, 0], (h + h.conj().T) / 2), "crz": G.rz(1, controls=[0]), "ccry": G.ry(2, controls=[0, 1])}


@pytest.mark.parametrize("name", sorted(_gates()))
def test_gate_is_unitary_and_dmatrix_is_its_derivative(name):
    g = _gates()[name]
    side, h = 1 << len(g.targets), 1e-6
    for theta in (-2.1, 0.0, 0.37, 1.9):
        w, dw = np.asarray(g.matrix(theta)), np.asarray(g.dmatrix(theta))
        assert w.shape == (side, side) and dw.shape == (side, side)
        assert np.max(np.abs(w.conj().T @ w - np.eye(side))) <= 1e-14
        diff = (np.asarray(g.matrix(theta + h)) - np.asarray(g.matrix(theta - h))) / (2 * h)
        assert np.max(np.abs(diff - dw)) <= 1e-8, name
        full, dfull = g.full(theta), g.dfull(theta)
        t = side
        assert np.array_equal(full[:-t, :-t], np.eye(len(full) - t)) and not np.any(dfull[:-t, :]) and not np.any(dfull[:, :-t])
        assert np.allclose(R.op_matrix(g.lower(theta)), full, atol=0, rtol=0)
    a = g.a_matrix(0.37)
    assert np.max(np.abs(a + a.conj().T)) <= 1e-14  # dW W^H is anti-Hermitian for a unitary family


def test_gate_conventions():
    assert np.allclose(G.rx(0).matrix(np.pi), -1j * np.array([[0, 1], [1, 0]]))          # exp(-i pi X / 2)
    assert np.allclose(G.pauli_rotation({0: "X"}).matrix(np.pi / 2), -1j * np.array([[0, 1], [1, 0]]))  # exp(-i theta P): no half
    assert G.pauli_rotation({3: "Z", 1: "X"}).targets == [1, 3]
    assert np.allclose(G.rzz(0, 1).matrix(0.4), np.diag(np.exp(-0.2j * np.array([1, -1, -1, 1]))))


def test_reduce_transition_conventions():
    """trace(A @ reduce(M)) = <bra| A |ket> for A on a subset of the pass's qubits, whatever the order of either list"""
    import transition_ref as T

    n = 5
    rng = np.random.default_rng(9)
    bra, ket = (rng.standard_normal((2, 1 << n)) + 1j * rng.standard_normal((2, 1 << n)))
    for set_qubits, gate_qubits in (([3, 0, 4], [4, 3]), ([1, 2], [1, 2]), ([2, 4, 1], [1]), ([0], [0]), ([4, 1, 0], [0, 4, 1])):
        a = rng.standard_normal((1 << len(gate_qubits),) * 2) + 1j * rng.standard_normal((1 << len(gate_qubits),) * 2)
        m = T.transition_ref(n, set_qubits, bra, ket)
        got = np.trace(a @ G.reduce_transition(m, set_qubits, gate_qubits))
        want = np.vdot(bra, R.apply_matrix(n, gate_qubits, a, ket))
        assert abs(got - want) <= 1e-12, (set_qubits, gate_qubits)


# ---- the driver, emulated ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (np.complex128, np.complex64), ids=("c128", "c64"))
@pytest.mark.parametrize("n", R.SIZES)
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_emulated_driver_meets_the_bars(name, n, dtype):
    circuit, params, terms, coeffs, psi0 = R.case(name, n, dtype)
    e_ref, g_ref = R.circuit_gradient_ref(n, circuit, params, terms, coeffs, psi0)
    bar_e, bar_g, bar_r = R.bars(circuit, params, coeffs, psi0)
    e, g, psi, passes = R.emulate(n, circuit, params, terms, coeffs, psi0)
    worst_g = float(np.max(np.abs(g - g_ref) / np.where(bar_g > 0, bar_g, 1.0)))
    back = float(np.linalg.norm(psi.astype(np.complex128) - psi0.astype(np.complex128)))
    print(f"{name} n={n}: |E - ref| / bar = {abs(e - e_ref) / bar_e:.3e}, grad worst / bar = {worst_g:.3e}, restore / bar = {back / bar_r:.3e}, "
          f"max |grad| / max bar = {np.max(np.abs(g_ref)) / np.max(bar_g):.3e}, {passes} passes")
    assert abs(e - e_ref) <= bar_e
    assert np.all(np.abs(g - g_ref) <= bar_g)
    assert back <= bar_r
    assert np.max(np.abs(g_ref)) >= 100 * np.max(bar_g)  # the bars are tight enough to tell a wrong gradient from a right one
    assert passes == sum(len(b["passes"]) for b in G.gradient_plan(circuit))


def test_reference_and_emulation_agree_with_central_differences():
    n = 5
    circuit, params, terms, coeffs, psi0 = R.case("mixed", n, np.complex128)
    g_ref = R.circuit_gradient_ref(n, circuit, params, terms, coeffs, psi0)[1]
    g_cd = R.central_differences(n, circuit, params, terms, coeffs, psi0)
    g_em = R.emulate(n, circuit, params, terms, coeffs, psi0)[1]
    print(f"reference against central differences {np.max(np.abs(g_ref - g_cd)):.3e}, emulation {np.max(np.abs(g_em - g_cd)):.3e}")
    assert np.max(np.abs(g_ref - g_cd)) <= 1e-9 and np.max(np.abs(g_em - g_cd)) <= 1e-9
    assert g_ref[6] == 0.0 and g_em[6] == 0.0  # a parameter no gate uses


# ---- argument checks that need no device --------------------------------------------------------------------------------------------
class _NoDevice(q.HipState):
    """a HipState without a handle: circuit_gradient's checks run before the library is called"""

    def __init__(self, n, dtype=np.complex128):
        import ctypes

        self.n, self.np_dtype, self.device = n, np.dtype(dtype), 0
        self.dtype = 0 if dtype == np.complex128 else 1
        self._h = ctypes.c_void_p(id(self))  # (never dereferenced: every call below is refused first)
        self._borrowed = True


def test_circuit_gradient_refusals_without_a_device():
    n = 4
    st, work = _NoDevice(n), _NoDevice(n)
    terms, coeffs = [{0: "Z"}], [1.0]
    good = [(G.ry(0), 0), _cnot(0, 1)]
    bad_calls = [
        ([(G.rzz(0, 1, controls=[2, 3]), 0)], [0.1], terms, coeffs, work),   # a parametrised gate on four qubits
        (good, [], terms, coeffs, work),                                      # parameter index out of range
        (good, [np.nan], terms, coeffs, work),                                # a non-finite parameter
        (good, [0.1], terms, [np.inf], work),                                 # a non-finite coefficient
        (good, [0.1], terms, [1.0, 2.0], work),                               # terms and coefficients differ in number
        (good, [0.1], terms, coeffs, st),                                     # work is self
        (good, [0.1], terms, coeffs, _NoDevice(n + 1)),                       # another size
        (good, [0.1], terms, coeffs, _NoDevice(n, np.complex64)),             # another precision
        (good, [0.1], [{0: "Q"}], coeffs, work),                              # not a Pauli factor
        (good, [0.1], [{n: "Z"}], coeffs, work),                              # a term's qubit out of range
        ([(G.ry(n), 0)], [0.1], terms, coeffs, work),                         # a gate's qubit out of range
        ([q.MatrixOp.new_matrix([0], np.eye(4))], [0.1], terms, coeffs, work),  # a malformed fixed op (16 entries on one qubit)
        ([("ry", 0)], [0.1], terms, coeffs, work),                            # not a circuit item
    ]
    for args in bad_calls:
        with pytest.raises(q.CircuitError):
            st.circuit_gradient(*args)
