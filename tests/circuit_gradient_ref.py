"""A reference for HipState.circuit_gradient, the bars the device call is held to, a numpy emulation of the driver and the
circuits the tests run — shared by tests/test_circuit_gradient_cpu.py and tests/test_gpu_f2_circuit_gradient.py.  The reference
and the bars are numpy only; `emulate` and `cases` use the host-only parts of rustqip_amd (ops, parametric).

Reference.  The circuit is simulated densely in clongdouble, every op as the matrix on its own qubits (a MatrixOp's first
listed qubit is the most significant bit of its matrix index).  E = <psi_T| H |psi_T>.  The contribution of a parametrised gate g
to the gradient is 2 Re <psi_T| H |psi'>, psi' the circuit with dW_g/dtheta IN PLACE OF W_g; it is evaluated as
2 Re <(W_{g+1}^H .. W_G^H) H psi_T | dW_g psi_{g-1}>, which is the same number for any matrices, unitary or not.

Bars, derived from what the project already states.  u is the unit roundoff of the state (2^-53, 2^-24).
  * hard_bound(k) of tests/numeric_ref.py: for a dense op on k target qubits every real component of an output amplitude is
    within (4 2^k + 8) u a_r of exact, a_r = the absolute row sum over its group, and a_r <= 2 ||x_group||_2 for a row of a
    unitary (|G_re|, |G_im| rows of norm <= 1 against x_re, x_im); a group has 2 * 2^k real components, so
        || fl(W psi) - W psi ||_2 <= gamma(k) u ||psi||_2,   gamma(k) = 2 sqrt(2^(k+1)) (4 2^k + 8).
    Controls only remove groups; a sparse op has fewer terms per row than the dense one of its size; Swaps move amplitudes
    exactly (gamma = 0).
  * Gamma = sum of gamma over the lowered ops of the circuit: psi_T is within Gamma u ||psi_0|| of exact (unitaries keep the
    norm), and after the way back within 2 Gamma u ||psi_0||: the restore bar.
  * S = sum |c_t|, `count` observable terms: lambda = H psi_T has norm <= S ||psi_0||, inherits S Gamma u ||psi_0|| from psi_T and
    adds the Pauli sum's (count + 8) u S ||psi_0|| (tests/pauli_pair_ref.py); pulled back it gains at most Gamma u S ||psi_0|| more.
  * E = Re <lambda|psi_T>: errors of both factors, and the matrix element's 1e-12 ||lambda|| ||psi||:
        bar(E) = S ||psi_0||^2 ((2 Gamma + count + 8) u + 1e-12).
  * dE/dtheta_g = 2 Re trace(A_g M_g) = 2 Re <lambda| A_g |psi> on states that have been through the circuit forward and (partly)
    back: psi off by at most 2 Gamma u, lambda by at most (2 Gamma + count + 8) u S, times ||A_g||_2; every entry of M_g carries
    the transition bar 1e-12 sqrt(rho_psi[a][a] rho_lambda[a'][a']) (a partial trace adds bars of disjoint columns, Cauchy-Schwarz
    again), so |trace(A_g dM)| <= 1e-12 ||A_g||_F ||lambda|| ||psi||:
        bar(grad_p) = sum over the gates g that use p of 2 S ||psi_0||^2 (||A_g||_2 (4 Gamma + count + 8) u + ||A_g||_F 1e-12).
These have the shape of pauli_pair_ref.gradient_bars and restore_bar (there gamma is the rotations' 12)."""
import numpy as np

import pauli_pair_ref as P
import transition_ref as TR

assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble has no 64-bit significand here: no reference for complex128"

MELEM_BAR = 1e-12


def unit_roundoff(dtype):
    return 2.0 ** -53 if np.dtype(dtype) == np.complex128 else 2.0 ** -24


def gamma(k):
    """|| fl(W psi) - W psi ||_2 <= gamma(k) u ||psi||_2 for a unitary dense op on k target qubits"""
    return 2.0 * np.sqrt(2.0 ** (k + 1)) * (4 * 2 ** k + 8)


# ---- ops as matrices ------------------------------------------------------------------------------------------------------------
def _innermost(op):
    """(number of controls, innermost op) of a MatrixOp, nested controls accumulated"""
    nc = 0
    while op.kind == "Control":
        nc, op = nc + op.n_controls, op.inner
    return nc, op


def op_gamma(op):
    nc, inner = _innermost(op)
    return 0.0 if inner.kind == "Swap" else gamma(len(op.indices) - nc)


def op_matrix(op):
    """complex128[2^k, 2^k] of a MatrixOp on its own index list (first listed qubit = most significant bit)"""
    k = len(op.indices)
    nc, inner = _innermost(op)
    t = k - nc
    if inner.kind == "Matrix":
        block = np.asarray(inner.data, dtype=np.complex128).reshape(1 << t, 1 << t)
    elif inner.kind == "SparseMatrix":
        block = np.zeros((1 << t, 1 << t), dtype=np.complex128)
        for r, row in enumerate(inner.rows):
            for c, v in row:
                block[r, c] += v
    elif inner.kind == "Swap":
        h = inner.half
        block = np.zeros((1 << t, 1 << t), dtype=np.complex128)
        for j in range(1 << t):
            a, b = j >> h, j & ((1 << h) - 1)  # (the A indices are listed first: the high half of the index)
            block[(b << h) | a, j] = 1.0
    else:
        raise ValueError(inner.kind)
    full = np.eye(1 << k, dtype=np.complex128)
    full[(1 << k) - (1 << t):, (1 << k) - (1 << t):] = block
    return full


def apply_matrix(n, qubits, mat, psi):
    """(mat on `qubits`, first = most significant bit) psi, in the precision of psi; qubit q is axis q of the 2 x .. x 2 cube"""
    k = len(qubits)
    cube = psi.reshape((2,) * n)
    m = np.asarray(mat).astype(psi.dtype).reshape((2,) * (2 * k))
    out = np.tensordot(m, cube, axes=(list(range(k, 2 * k)), list(qubits)))  # axes: the k new ones first, then the rest in order
    rest = [q for q in range(n) if q not in qubits]
    order = list(qubits) + rest
    return np.transpose(out, np.argsort(order)).reshape(-1)


def _items(circuit):
    """[(qubits, W, dW or None, parameter or None)] for given parameters is built by the callers; here: the split of an item"""
    out = []
    for item in circuit:
        if isinstance(item, (tuple, list)):
            out.append((item[0], int(item[1])))
        else:
            out.append((item, None))
    return out


def pauli_sum(n, terms, coeffs, psi):
    out = np.zeros_like(psi)
    for term, c in zip(terms, coeffs):
        out = out + psi.real.dtype.type(c) * P.apply_term(n, term, psi)
    return out


def circuit_gradient_ref(n, circuit, params, obs_terms, obs_coeffs, psi0, ctype=np.clongdouble):
    """(E, grad) by dense simulation in `ctype`"""
    params = np.asarray(params, dtype=np.float64)
    items = _items(circuit)
    mats = []
    for g, p in items:
        mats.append((list(g.indices), op_matrix(g), None) if p is None else (list(g.qubits), g.full(params[p]), g.dfull(params[p])))
    psis = [np.asarray(psi0).astype(ctype)]
    for qubits, w, _ in mats:
        psis.append(apply_matrix(n, qubits, w, psis[-1]))
    lam = pauli_sum(n, obs_terms, obs_coeffs, psis[-1])
    energy = float(np.vdot(lam, psis[-1]).real)
    grad = np.zeros(len(params), dtype=np.longdouble)
    for j in range(len(mats) - 1, -1, -1):
        qubits, w, dw = mats[j]
        if dw is not None:
            grad[items[j][1]] += 2 * np.vdot(lam, apply_matrix(n, qubits, dw, psis[j])).real
        lam = apply_matrix(n, qubits, w.conj().T, lam)
    return energy, grad.astype(np.float64)


def central_differences(n, circuit, params, obs_terms, obs_coeffs, psi0, h=1e-5):
    params = np.asarray(params, dtype=np.float64)
    grad = np.zeros(len(params))
    for p in range(len(params)):
        up, dn = params.copy(), params.copy()
        up[p] += h
        dn[p] -= h
        grad[p] = (circuit_gradient_ref(n, circuit, up, obs_terms, obs_coeffs, psi0)[0]
                   - circuit_gradient_ref(n, circuit, dn, obs_terms, obs_coeffs, psi0)[0]) / (2 * h)
    return grad


def bars(circuit, params, obs_coeffs, psi0):
    """(bar of E, float64[len(params)] bars of the gradient, the restore bar) for a state of psi0's precision"""
    psi0 = np.asarray(psi0)
    params = np.asarray(params, dtype=np.float64)
    u, count = unit_roundoff(psi0.dtype), len(obs_coeffs)
    S = float(np.sum(np.abs(obs_coeffs)))
    norm = float(np.linalg.norm(psi0.astype(np.complex128)))
    items = _items(circuit)
    big_gamma = sum(op_gamma(g if p is None else g.lower(params[p])) for g, p in items)
    bar_e = S * norm ** 2 * ((2 * big_gamma + count + 8) * u + MELEM_BAR)
    bar_g = np.zeros(len(params))
    for g, p in items:
        if p is not None:
            a = g.a_matrix(params[p])
            bar_g[p] += 2 * S * norm ** 2 * (np.linalg.norm(a, 2) * (4 * big_gamma + count + 8) * u + np.linalg.norm(a, "fro") * MELEM_BAR)
    return bar_e, bar_g, 2 * big_gamma * u * norm


# ---- the driver, restated in numpy in the state's precision ------------------------------------------------------------------------
def emulate(n, circuit, params, obs_terms, obs_coeffs, psi0):
    """(E, grad, psi at the end, passes made): HipState.circuit_gradient with numpy vectors of psi0's precision in place of
    device states: the plan of parametric.gradient_plan, exact transition matrices (transition_ref), the host's partial traces
    and A_g, the inverses of ops.inverse_op"""
    import rustqip_amd as q
    from rustqip_amd.parametric import gradient_plan, reduce_transition

    psi = np.asarray(psi0).copy()
    params = np.asarray(params, dtype=np.float64)
    items = _items(circuit)
    lowered = [g if p is None else g.lower(params[p]) for g, p in items]
    inverses = [q.inverse_op(op) for op in lowered]
    for op in lowered:
        psi = apply_matrix(n, list(op.indices), op_matrix(op), psi)
    lam = P.pauli_sum_ref(n, obs_terms, obs_coeffs, psi).astype(psi.dtype)
    energy = float(np.vdot(lam.astype(np.complex128), psi.astype(np.complex128)).real)
    grad = np.zeros(len(params))
    passes = 0
    for block in gradient_plan(circuit):
        for ps in block["passes"]:
            m = TR.transition_ref(n, ps["qubits"], lam, psi)
            passes += 1
            for i in ps["gates"]:
                g, p = items[i]
                grad[p] += 2.0 * float(np.trace(g.a_matrix(params[p]) @ reduce_transition(m, ps["qubits"], g.qubits)).real)
        for i in reversed(block["gates"]):
            op = inverses[i]
            psi = apply_matrix(n, list(op.indices), op_matrix(op), psi)
            lam = apply_matrix(n, list(op.indices), op_matrix(op), lam)
    return energy, grad, psi, passes


# ---- the cases of the tests -----------------------------------------------------------------------------------------------------------
def product_state(n, seed, dtype):
    """a normalised product of n random single-qubit states: dense amplitudes, and local observables keep gradients of order one"""
    rng = np.random.default_rng(seed)
    psi = np.ones(1, dtype=np.complex128)
    for _ in range(n):
        v = rng.standard_normal(2) + 1j * rng.standard_normal(2)
        psi = np.kron(psi, v / np.linalg.norm(v))
    return psi.astype(dtype)


def _cnot(q, c, t):
    return q.make_control_op([c], q.make_matrix_op([t], [0, 1, 1, 0]))


def _random_unitary(rng, side):
    z = rng.standard_normal((side, side)) + 1j * rng.standard_normal((side, side))
    u, r = np.linalg.qr(z)
    return u * (np.diag(r) / np.abs(np.diag(r)))


def observable(n):
    """three terms, S = 2: a ZZ pair at the low end, X on the last qubit, Y in the middle"""
    return [{0: "Z", 1: "Z"}, {n - 1: "X"}, {n // 2: "Y"}], np.array([0.9, 0.7, -0.4])


def case_layers(n):
    """(i) two layers of ry on every qubit, a CNOT chain after each: 2n parameters"""
    import rustqip_amd as q
    from rustqip_amd import parametric as G

    rng = np.random.default_rng(7100 + n)
    circuit = []
    for layer in range(2):
        circuit += [(G.ry(qb), layer * n + qb) for qb in range(n)]
        circuit += [_cnot(q, qb, qb + 1) for qb in range(n - 1)]
    return circuit, rng.uniform(-1.5, 1.5, 2 * n)


MIXED_SEED = {4: 28, 5: 21, 9: 36, 13: 16}  # (picked so that the largest gradient component stands 100 bars high in Complex<f32> too)


def case_mixed(n):
    """(ii) n >= 4: a controlled rz on non-adjacent qubits, rzz listed high qubit first, a doubly controlled ry, a generator
    gate on two qubits, a phase gate, parameters 0, 1 and 2 each shared by two gates, a Swap op, a fixed sparse op and a fixed dense
    4-qubit op; 7 parameters, parameter 6 used by no gate"""
    import rustqip_amd as q
    from rustqip_amd import parametric as G

    rng = np.random.default_rng(7200 + n + 100 * MIXED_SEED[n])
    h = rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4))
    gen = (h + h.conj().T) / 8
    s = np.sqrt(0.5)
    sparse = q.make_sparse_matrix_op([1, 2], [[(0, 1.0)], [(1, s), (2, 1j * s)], [(1, 1j * s), (2, s)], [(3, -1.0)]])
    dense4 = q.make_matrix_op([n - 1, 0, n // 2, 1], _random_unitary(rng, 16))
    circuit = [
        (G.ry(0), 2), (G.ry(1), 0), (G.ry(n - 1), 1),
        _cnot(q, 0, n - 1),
        (G.rz(n - 1, controls=[0]), 3),
        q.make_swap_op([0], [n - 1]),
        (G.rzz(n - 1, 1), 4),
        sparse,
        (G.ry(3, controls=[0, 2]), 5),
        dense4,
        (G.generator_gate([1, n - 2], gen), 0),
        (G.rx(n - 1), 2),
        q.make_matrix_op([2], [s, s, s, -s]),
        (G.phase(2), 1),
    ]
    return circuit, np.concatenate([rng.uniform(-1.5, 1.5, 6), [0.3]])


def rotation_terms(n):
    return [{0: "X", 1: "Y"}, {2: "Z"}, {n - 1: "Y", 0: "Z", 2: "X"}, {1: "X"}, {n - 1: "Z", 1: "Z"}, {n - 2: "Y"}, {0: "X", 1: "Y"}, {3: "X", n - 1: "X"}]


def case_rotations(n):
    """(iii) Pauli rotations exp(-i theta P) only, every one with its own parameter: what adjoint_gradient takes too"""
    from rustqip_amd import parametric as G

    rng = np.random.default_rng(7300 + n)
    terms = rotation_terms(n)
    return [(G.pauli_rotation(t), i) for i, t in enumerate(terms)], rng.uniform(-1.5, 1.5, len(terms))


CASES = {"layers": case_layers, "mixed": case_mixed, "rotations": case_rotations}
SIZES = (4, 9, 13)


def case(name, n, dtype):
    """(circuit, params, obs_terms, obs_coeffs, psi0)"""
    circuit, params = CASES[name](n)
    terms, coeffs = observable(n)
    return circuit, params, terms, coeffs, product_state(n, 7000 + n, dtype)
