"""HipState.circuit_gradient on the device: the energy, the gradient and the restored state against the clongdouble reference of
tests/circuit_gradient_ref.py, held to the bars derived there (bar(E), bar(grad_p), the restore bar), on the circuits
tests/test_circuit_gradient_cpu.py shows a correct driver to meet them on:
  layers     two layers of ry on every qubit, a CNOT chain after each
  mixed      a controlled rz on non-adjacent qubits, rzz listed high qubit first, a doubly controlled ry, a generator gate on two
             qubits, shared parameters, a phase gate, a Swap op, a fixed sparse op, a fixed dense 4-qubit op, an unused parameter
  rotations  Pauli rotations only: also against the existing adjoint_gradient
at n = 4, 9 and 13 in both precisions.  Every test prints its worst ratios before it asserts."""
from gpu_common import *  # noqa: F401,F403

import circuit_gradient_ref as R
import pauli_pair_ref as P
from rustqip_amd import parametric as G

pytestmark = pytest.mark.gpu

_IDS = ("c128", "c64")
_DTYPES = (np.complex128, np.complex64)
_REFS = {}


def _case(name, n, dtype):
    """the case with its reference and bars: computed once, shared, never written to"""
    key = (name, n, np.dtype(dtype))
    if key not in _REFS:
        circuit, params, terms, coeffs, psi0 = R.case(name, n, dtype)
        psi0.setflags(write=False)
        _REFS[key] = (circuit, params, terms, coeffs, psi0, R.circuit_gradient_ref(n, circuit, params, terms, coeffs, psi0),
                      R.bars(circuit, params, coeffs, psi0))
    return _REFS[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("dtype", _DTYPES, ids=_IDS)
@pytest.mark.parametrize("n", R.SIZES)
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_against_the_reference(name, n, dtype):
    circuit, params, terms, coeffs, psi0, (e_ref, g_ref), (bar_e, bar_g, bar_r) = _case(name, n, dtype)
    planned = sum(len(b["passes"]) for b in G.gradient_plan(circuit))
    with q.HipState(n, dtype) as st, q.HipState(n, dtype) as work:
        st.upload(psi0)
        e, g = st.circuit_gradient(circuit, params, terms, coeffs, work)
        back = st.download()
        passes = getattr(work, "transition_passes", 0)
    worst_g = float(np.max(np.abs(g - g_ref) / np.where(bar_g > 0, bar_g, 1.0)))
    restore = float(np.linalg.norm(back.astype(np.complex128) - psi0.astype(np.complex128)))
    print(f"{name} n={n}: |E - ref| / bar = {abs(e - e_ref) / bar_e:.3e}, grad worst / bar = {worst_g:.3e}, "
          f"restore / bar = {restore / bar_r:.3e}, {passes} transition passes for {planned} planned")
    assert g.dtype == np.float64 and g.shape == (len(params),)
    assert abs(e - e_ref) <= bar_e
    assert np.all(np.abs(g - g_ref) <= bar_g)
    assert restore <= bar_r
    assert passes == planned
    if name == "mixed":
        assert g[6] == 0.0  # the parameter no gate uses


@pytest.mark.parametrize("dtype", _DTYPES, ids=_IDS)
@pytest.mark.parametrize("n", R.SIZES)
def test_rotations_against_adjoint_gradient(n, dtype):
    """the same rotations through the existing adjoint_gradient: the two device results agree within the sum of their bars"""
    circuit, params, terms, coeffs, psi0, _, (bar_e, bar_g, _) = _case("rotations", n, dtype)
    rot = R.rotation_terms(n)
    old_e, old_g = P.gradient_bars(len(rot), coeffs, psi0)
    with q.HipState(n, dtype) as st, q.HipState(n, dtype) as work:
        st.upload(psi0)
        e, g = st.circuit_gradient(circuit, params, terms, coeffs, work)
        st.upload(psi0)
        e2, g2 = st.adjoint_gradient(rot, params, terms, coeffs, work)
    print(f"rotations n={n}: |dE| / bars = {abs(e - e2) / (bar_e + old_e):.3e}, grad worst / bars = {np.max(np.abs(g - g2) / (bar_g + old_g)):.3e}")
    assert abs(e - e2) <= bar_e + old_e
    assert np.all(np.abs(g - g2) <= bar_g + old_g)


@pytest.mark.parametrize("dtype", _DTYPES, ids=_IDS)
@pytest.mark.parametrize("n", R.SIZES)
def test_shift_rule(n, dtype):
    """parameters of the layers circuit that one ry uses alone: dE/dtheta = [E(theta + pi/2) - E(theta - pi/2)] / 2 exactly, the
    two energies through apply_ops + expectation, within 2 bar(E)"""
    circuit, params, terms, coeffs, psi0, _, (bar_e, _, _) = _case("layers", n, dtype)
    with q.HipState(n, dtype) as st, q.HipState(n, dtype) as work:
        st.upload(psi0)
        _, g = st.circuit_gradient(circuit, params, terms, coeffs, work)
        for p in (0, n - 1, n + n // 2):
            energies = []
            for shift in (np.pi / 2, -np.pi / 2):
                shifted = np.array(params)
                shifted[p] += shift
                st.upload(psi0)
                st.apply_ops([item if isinstance(item, q.MatrixOp) else item[0].lower(shifted[item[1]]) for item in circuit])
                energies.append(st.expectation(terms, coeffs))
            rule = (energies[0] - energies[1]) / 2
            print(f"layers n={n}: parameter {p}: adjoint {g[p]!r}, shift rule {rule!r}, |difference| / (2 bar(E)) = {abs(g[p] - rule) / (2 * bar_e):.3e}")
            assert abs(g[p] - rule) <= 2 * bar_e


@pytest.mark.parametrize("dtype", _DTYPES, ids=_IDS)
def test_no_parameters_and_refusals(dtype):
    """a circuit without parametrised gates returns the energy and zeros; every refusal leaves both states bit-equal"""
    n = 9
    circuit, params, terms, coeffs, psi0, _, _ = _case("mixed", n, dtype)
    fixed = [item for item in circuit if isinstance(item, q.MatrixOp)]
    other = np.complex64 if dtype == np.complex128 else np.complex128
    w0 = R.product_state(n, 99, dtype)
    with q.HipState(n, dtype) as st, q.HipState(n, dtype) as work, q.HipState(n, other) as prec:
        st.upload(psi0)
        e, g = st.circuit_gradient(fixed, [0.3, 0.4], terms, coeffs, work)
        e_ref, _ = R.circuit_gradient_ref(n, fixed, [0.3, 0.4], terms, coeffs, psi0)
        bar_e, _, bar_r = R.bars(fixed, [0.3, 0.4], coeffs, psi0)
        print(f"no parameters: |E - ref| / bar = {abs(e - e_ref) / bar_e:.3e}")
        assert abs(e - e_ref) <= bar_e and np.array_equal(g, np.zeros(2))
        assert np.linalg.norm(st.download().astype(np.complex128) - psi0.astype(np.complex128)) <= bar_r
        st.upload(psi0)
        work.upload(w0)
        bad_calls = [
            ([(G.rzz(0, 1, controls=[2, 3]), 0)], params, terms, coeffs, work),
            (circuit, params[:3], terms, coeffs, work),
            (circuit, np.where(np.arange(len(params)) == 1, np.nan, params), terms, coeffs, work),
            (circuit, params, terms, [np.inf, 1.0, 1.0], work),
            (circuit, params, terms, coeffs, st),
            (circuit, params, terms, coeffs, prec),
            (circuit, params, [{n: "Z"}, {0: "X"}, {1: "Y"}], coeffs, work),
            (circuit + [(G.ry(n), 0)], params, terms, coeffs, work),
        ]
        for args in bad_calls:
            with pytest.raises(q.CircuitError):
                st.circuit_gradient(*args)
            assert np.array_equal(_bits(st.download()), _bits(psi0)) and np.array_equal(_bits(work.download()), _bits(w0))
