"""References for the vector arithmetic of device states (linear_combination, inner_products) and for the Krylov solvers built on
it (krylov_basis, ground_state, krylov_evolve), independent of the code under test, and the bars the tests hold them to.  Shared
by tests/test_krylov_cpu.py and tests/test_gpu_f3_krylov.py.  A plain helper module: numpy only, no fixtures.

The combination is held to its bits: lincomb_spec restates the arithmetic include/qip_hipx.h fixes in the state's own precision.
Inner products are held to pauli_pair_ref.melem_bar (1e-12 |bra| |ket|) against math.fsum; the norm of a combination to
1e-12 of the exact sum of the stored squares.

The solvers are held to

    B = K * m * (T + 8) * u * S,

m the basis dimension, T the number of terms, S = sum |c_t|, u the unit roundoff of the state's precision.  K is a measurement,
not a choice: the numpy restatement below, run in the state's own precision on the inputs of the tests
(solver_checks), against references in extended precision or from the dense matrix; the worst error / (m (T + 8) u S) over all
solver checks was (tests/test_krylov_cpu.py prints them; profiles/krylov.md repeats them)

    complex128   0.0217  (orthonormality of the Ising chain's basis at n = 8, m = 4: 2.2e-16, one unit in the last place of a
                         squared norm, against m (T + 8) u = 1.0e-14)
                 0.0095  (next: the breakdown case, the Ritz values of the XXZ chain at n = 3 against eigh's eigenvalues, 1.8e-15)
                 0.0066  (ground_state on the Ising chain at n = 10, the energy against the lowest eigenvalue, 7.1e-15)
    complex64    0.0108  (the same orthonormality check, 5.9e-8)

8 * 0.0217 = 0.17, rounded up to a power of two: K = 1/4 (rustqip_amd.state.KRYLOV_K is the same number; it is also the
breakdown threshold of krylov_basis and the stopping residual of ground_state, and the figures above were taken with it in that
role).  The factor 8 covers the other summation order of the device's reductions and the f32 rounding of the coefficients;
test_krylov_cpu.py asserts that the restatement alone meets every bar with K / 8, so the GPU tests cannot hide a failure behind
a loose constant."""
import math

import numpy as np

import pauli_pair_ref as P
from measure_ref import DTYPES, make_state, seed_of  # noqa: F401

K = 0.25
NORM_BAR = 1e-12  # the norm of a combination, relative to the exact sum of the stored squares


def unit_roundoff(dtype):
    return P.unit_roundoff(dtype)


def bar(m, terms, coeffs, dtype, k=K):
    """B = k m (T + 8) u S"""
    return k * m * (len(terms) + 8) * unit_roundoff(dtype) * float(np.sum(np.abs(coeffs)))


# ---- the two kernels ------------------------------------------------------------------------------------------------------------
def lincomb_spec(srcs, coeffs, dtype):
    """sum_i c_i srcs[i] by the arithmetic of include/qip_hipx.h, in the precision of `dtype`: c_i rounded once, per amplitude
    p_i = (fl(fl(cr sr) - fl(ci si)), fl(fl(cr si) + fl(ci sr))), acc = p_0, then acc = fl(acc + p_i) in source order.  Bit-exact
    by construction: numpy rounds every elementwise operation once and fuses nothing."""
    dtype = np.dtype(dtype)
    real = np.float32 if dtype == np.complex64 else np.float64
    coeffs = np.asarray(coeffs, dtype=np.complex128).reshape(-1)
    assert len(coeffs) == len(srcs) >= 1
    ar = ai = None
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        for s, c in zip(srcs, coeffs):
            s = np.asarray(s)
            assert s.dtype == dtype
            sr, si = s.real.astype(real), s.imag.astype(real)
            cr, ci = real(c.real), real(c.imag)
            pr, pi = cr * sr - ci * si, cr * si + ci * sr
            assert pr.dtype == real
            ar, ai = (pr, pi) if ar is None else (ar + pr, ai + pi)
    out = np.empty(len(ar), dtype=dtype)
    out.real, out.imag = ar, ai
    return out


def norm_exact(x):
    """sum_j |x_j|^2 of the stored amplitudes: the squares in double (exact for f32 amplitudes, one rounding of 2^-53 for f64),
    added by math.fsum"""
    x = np.asarray(x)
    re, im = x.real.astype(np.float64), x.imag.astype(np.float64)
    return math.fsum(re * re) + math.fsum(im * im)


def inner_ref(bra, ket):
    """<bra|ket>: the four real products per amplitude in double from the amplitudes widened to double (one rounding of 2^-53
    each; formed part by part: a complex multiplication may be fused), all of them summed with math.fsum"""
    p, a = np.asarray(bra).astype(np.complex128), np.asarray(ket).astype(np.complex128)
    return complex(math.fsum(np.concatenate([p.real * a.real, p.imag * a.imag])),
                   math.fsum(np.concatenate([p.real * a.imag, -(p.imag * a.real)])))


def inner_bar(bra, ket):
    return P.melem_bar(bra, ket)


# ---- Hamiltonians ---------------------------------------------------------------------------------------------------------------
def ising_chain(n, coupling=1.0, field=1.5):
    """(terms, coeffs) of -J sum Z_q Z_q+1 - h sum X_q, open ends: 2n - 1 terms, two x-mask classes (0 and single bits)"""
    terms = [{q: "Z", q + 1: "Z"} for q in range(n - 1)] + [{q: "X"} for q in range(n)]
    return terms, np.array([-coupling] * (n - 1) + [-field] * n, dtype=np.float64)


def xxz_chain(n, delta=0.7, field=0.3):
    """(terms, coeffs) of sum (X X + Y Y + delta Z Z)_{q,q+1} + sum_q h (1 + q / n) Z_q, open ends: 4n - 3 terms; Y strings, and
    the X X and Y Y terms of a bond share an x mask"""
    terms, coeffs = [], []
    for q in range(n - 1):
        for p, c in (("X", 1.0), ("Y", 1.0), ("Z", delta)):
            terms.append({q: p, q + 1: p})
            coeffs.append(c)
    for q in range(n):
        terms.append({q: "Z"})
        coeffs.append(field * (1.0 + q / n))
    return terms, np.array(coeffs, dtype=np.float64)


HAMILTONIANS = {"ising": ising_chain, "xxz": xxz_chain}


def dense_matrix(n, terms, coeffs):
    """complex128[2^n, 2^n]: H = sum_t c_t P_t, for small n"""
    size = 1 << n
    h = np.zeros((size, size), dtype=np.complex128)
    j = np.arange(size)
    for term, c in zip(terms, coeffs):
        k, f = P._partner(n, term)
        h[j, k] += c * f  # (P psi)[j] = f[j] psi[k[j]]
    return h


_EIGH = {}


def spectrum(name, n):
    """(eigenvalues ascending, eigenvectors, terms, coeffs) of a test Hamiltonian: computed once, shared, never written to"""
    if (name, n) not in _EIGH:
        terms, coeffs = HAMILTONIANS[name](n)
        lam, vec = np.linalg.eigh(dense_matrix(n, terms, coeffs))
        lam.setflags(write=False)
        vec.setflags(write=False)
        _EIGH[name, n] = (lam, vec, terms, coeffs)
    return _EIGH[name, n]


def propagate_exact(name, n, t, psi):
    """exp(-i H t) psi through the dense eigendecomposition, in complex128"""
    lam, vec, _, _ = spectrum(name, n)
    return vec @ (np.exp(-1j * lam * t) * (vec.conj().T @ np.asarray(psi).astype(np.complex128)))


# ---- the solvers restated ---------------------------------------------------------------------------------------------------------
class Arith:
    """The vector operations of the solvers.  ctype None: the state's own precision `dtype` with the arithmetic the device
    fixes (pauli_pair_ref.pauli_sum_spec, lincomb_spec) and double reductions in numpy's order; otherwise plain numpy in
    `ctype` (np.clongdouble: the reference the restatement is measured against)."""

    def __init__(self, n, terms, coeffs, dtype, ctype=None):
        self.n, self.terms, self.coeffs, self.dtype, self.ctype = n, list(terms), np.asarray(coeffs, dtype=np.float64), np.dtype(dtype), ctype

    def load(self, psi):
        return np.asarray(psi).astype(self.dtype).astype(self.ctype or self.dtype)

    def apply_h(self, v):
        if self.ctype is None:
            return P.pauli_sum_spec(self.n, self.terms, self.coeffs, v)
        out = np.zeros_like(v)
        for term, c in zip(self.terms, self.coeffs):
            out = out + v.real.dtype.type(c) * P.apply_term(self.n, term, v)
        return out

    def lincomb(self, srcs, coeffs):
        """(sum_i c_i srcs[i], its squared norm)"""
        if self.ctype is None:
            out = lincomb_spec(srcs, coeffs, self.dtype)
            wide = out.astype(np.complex128)
            return out, float(np.sum(wide.real * wide.real + wide.imag * wide.imag))
        out = sum(self.ctype(c) * s for c, s in zip(coeffs, srcs))
        return out, float(np.vdot(out, out).real)

    def inner(self, bra, ket):
        if self.ctype is None:
            return complex(np.vdot(bra.astype(np.complex128), ket.astype(np.complex128)))
        return complex(np.vdot(bra, ket))


def tridiagonal(alphas, betas):
    k = len(alphas)
    b = np.asarray(betas, dtype=np.float64)[:k - 1]
    return np.diag(np.asarray(alphas, dtype=np.float64)) + np.diag(b, 1) + np.diag(b, -1)


def lanczos(ar, psi, m, reorthogonalize, breakdown):
    """HipState.krylov_basis restated: (alphas, betas, basis, |psi|)"""
    v0, norm2 = ar.lincomb([psi], [1.0])
    norm = math.sqrt(norm2)
    basis = [ar.lincomb([v0], [1.0 / norm])[0]]
    alphas, betas = [], []
    for j in range(m):
        v = basis[j]
        w = ar.apply_h(v)
        alpha = ar.inner(v, w).real
        if j == 0:
            w, norm2 = ar.lincomb([w, v], [1.0, -alpha])
        else:
            w, norm2 = ar.lincomb([w, v, basis[j - 1]], [1.0, -alpha, -betas[-1]])
        if reorthogonalize:
            h = np.array([ar.inner(b, w) for b in basis[:j + 1]])
            w, norm2 = ar.lincomb([w] + basis[:j + 1], np.concatenate([[1.0], -h]))
        alphas.append(alpha)
        betas.append(math.sqrt(norm2))
        if not betas[-1] > breakdown:
            basis.append(w)
            break
        basis.append(ar.lincomb([w], [1.0 / betas[-1]])[0])
    return np.array(alphas), np.array(betas), basis, norm


def ground_state(ar, psi, m, restarts, breakdown):
    """HipState.ground_state restated: (energy, residual, the Ritz vector, rounds run)"""
    psi = ar.load(psi)
    energy = residual = float("nan")
    rounds = 0
    for _ in range(restarts):
        rounds += 1
        alphas, betas, basis, _ = lanczos(ar, psi, m, True, breakdown)
        theta, y = np.linalg.eigh(tridiagonal(alphas, betas))
        energy, residual = float(theta[0]), float(betas[-1] * abs(y[-1, 0]))
        psi, norm2 = ar.lincomb(basis[:len(alphas)], y[:, 0])
        psi = ar.lincomb([psi], [1.0 / math.sqrt(norm2)])[0]
        if residual <= breakdown:
            break
    return energy, residual, psi, rounds


def propagator_column(alphas, betas, tau):
    """exp(-i T tau) e_0 by Taylor series in ceil(|T|_1 |tau|) steps, the three-term rows written out: every entry keeps its
    relative accuracy, the tiny last one included (the eigendecomposition would leave it an absolute error of 2^-53)"""
    k = len(alphas)
    a, b = np.asarray(alphas, dtype=np.float64), np.asarray(betas, dtype=np.float64)[:k - 1]
    norm1 = max(abs(a[i]) + (b[i - 1] if i else 0.0) + (b[i] if i < k - 1 else 0.0) for i in range(k))
    steps = max(1, math.ceil(norm1 * abs(tau)))
    column = np.zeros(k, dtype=np.complex128)
    column[0] = 1.0
    for _ in range(steps):
        term = column
        for order in range(1, k + 26):
            applied = a * term
            applied[:-1] += b * term[1:]
            applied[1:] += b * term[:-1]
            term = (-1j * tau / steps / order) * applied
            column = column + term
    return column


def krylov_evolve(ar, psi, t, m, substeps, breakdown):
    """HipState.krylov_evolve restated: (the evolved vector, the largest a-posteriori estimate)"""
    psi = ar.load(psi)
    tau, worst = t / substeps, 0.0
    for _ in range(substeps):
        alphas, betas, basis, norm = lanczos(ar, psi, m, True, breakdown)
        column = propagator_column(alphas, betas, tau)
        worst = max(worst, float(betas[-1] * abs(tau) * abs(column[-1]) * norm))
        psi = ar.lincomb(basis[:len(alphas)], norm * column)[0]
    return psi, worst


# ---- the cases of the solver tests (CPU and GPU run the same ones) ---------------------------------------------------------------
BASIS_CASES = [(name, n, m, reorth) for name, n in (("ising", 8), ("xxz", 10)) for m in (4, 15) for reorth in (True, False)]
BREAKDOWN_CASE = ("xxz", 3, 15)
GROUND_CASES = [("ising", 10, 15, 40), ("xxz", 10, 15, 40)]  # (name, n, m, restarts)
EVOLVE_CASES = [("ising", 8, 15, 0.3, 3), ("xxz", 8, 15, 0.2, 2)]  # (name, n, m, t, substeps)


def start_state(n, dtype, salt=0):
    """the start vector of the solver cases: norm^2 = 0.8, nothing zeroed"""
    x = make_state(n, seed_of(n, dtype) + 77 + 1000 * salt, dtype, zero_every=1 << 30, norm=0.8)
    x.setflags(write=False)
    return x


def weight(coeffs):
    return float(np.sum(np.abs(coeffs)))


def basis_defect(inner, basis):
    """the largest of |<v_i|v_last>|, i < last, |<v_0|v_i>|, i > 0, | |v_last|^2 - 1 | and | |v_0|^2 - 1 |: `inner(bra, ket)` is
    the restatement's or the device's inner product"""
    last = len(basis) - 1
    worst = max(abs(inner(basis[last], basis[last]) - 1.0), abs(inner(basis[0], basis[0]) - 1.0))
    for i in range(1, last + 1):
        worst = max(worst, abs(inner(basis[i - 1], basis[last])), abs(inner(basis[0], basis[i])))
    return float(worst)


def ritz_values(alphas, betas):
    return np.linalg.eigvalsh(tridiagonal(alphas, betas))


def nearest(lam, value):
    return float(np.min(np.abs(np.asarray(lam) - value)))


def solver_checks(dtype):
    """[(what, error, unit = m (T + 8) u S)] of every solver check for the restatement in the precision `dtype`: the figures K
    was measured from.  error / unit <= K / 8 is the condition tests/test_krylov_cpu.py asserts."""
    out = []
    u = unit_roundoff(dtype)
    for name, n, m, reorth in BASIS_CASES:
        _, _, terms, coeffs = spectrum(name, n)
        unit = bar(m, terms, coeffs, dtype, 1.0)
        psi = start_state(n, dtype)
        own, ref = Arith(n, terms, coeffs, dtype), Arith(n, terms, coeffs, dtype, np.clongdouble)
        a, b, basis, _ = lanczos(own, own.load(psi), m, reorth, K * unit)
        ra, rb, _, _ = lanczos(ref, ref.load(psi), m, reorth, K * unit)
        assert len(a) == len(ra) == m
        out.append((f"basis {name} n={n} m={m} reorth={reorth}", float(max(np.max(np.abs(a - ra)), np.max(np.abs(b - rb)))), unit))
        if reorth:  # (in units of B / S: overlaps are pure numbers)
            out.append((f"basis {name} n={n} m={m}: orthonormality of the first and the last vector", basis_defect(own.inner, basis), unit / weight(coeffs)))
    name, n, m = BREAKDOWN_CASE
    lam, _, terms, coeffs = spectrum(name, n)
    unit = bar(m, terms, coeffs, dtype, 1.0)
    own = Arith(n, terms, coeffs, dtype)
    a, b, _, _ = lanczos(own, own.load(start_state(n, dtype)), m, True, K * unit)
    assert len(a) <= 1 << n, "no breakdown"
    out.append((f"breakdown {name} n={n}: {len(a)} steps", max(nearest(lam, th) for th in ritz_values(a, b)), unit))
    for name, n, m, restarts in GROUND_CASES:
        lam, _, terms, coeffs = spectrum(name, n)
        unit = bar(m, terms, coeffs, dtype, 1.0)
        own = Arith(n, terms, coeffs, dtype)
        energy, residual, vec, rounds = ground_state(own, start_state(n, dtype), m, restarts, K * unit)
        assert residual <= K * unit, f"{name}: residual {residual} after {rounds} rounds"
        out.append((f"ground {name} n={n}: nearest eigenvalue beyond the residual ({rounds} rounds)", max(nearest(lam, energy) - residual, 0.0), unit))
        out.append((f"ground {name} n={n}: energy against the lowest eigenvalue", abs(energy - lam[0]), unit))
        out.append((f"ground {name} n={n}: norm of the Ritz vector", abs(math.sqrt(norm_exact(vec)) - 1.0), unit))
    for name, n, m, t, substeps in EVOLVE_CASES:
        _, _, terms, coeffs = spectrum(name, n)
        unit = bar(m, terms, coeffs, dtype, 1.0)
        psi = start_state(n, dtype)
        norm = math.sqrt(norm_exact(psi))
        wide = Arith(n, terms, coeffs, np.complex128)
        conv, est = krylov_evolve(wide, psi, t, m, substeps, K * unit)
        exact = propagate_exact(name, n, t, psi)
        # the condition on t: the complex128 restatement has converged below this precision's bar
        assert float(np.linalg.norm(conv - exact)) <= K * unit * norm and est <= K * unit * norm, (name, t, est)
        own = Arith(n, terms, coeffs, dtype)
        got, est = krylov_evolve(own, psi, t, m, substeps, K * unit)
        out.append((f"evolve {name} n={n} t={t}: state", float(np.linalg.norm(got.astype(np.complex128) - exact)) / norm, unit))
        out.append((f"evolve {name} n={n} t={t}: norm", abs(math.sqrt(norm_exact(got)) - norm), unit))
    return out
