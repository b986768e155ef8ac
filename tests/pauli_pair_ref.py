"""References for the two-state Pauli calls — dst (+)= (sum_t c_t P_t) src, <bra| P |ket> and the adjoint gradient built from
them — independent of the code under test, and the bars the tests hold the device calls to.  Shared by
tests/test_pauli_pair_cpu.py and tests/test_gpu_f2_pauli_pair.py.  A plain helper module: numpy only, no fixtures.

A term is a mapping {qubit: "I" | "X" | "Y" | "Z"}; qubit q is amplitude-index bit n - 1 - q.  With x, z, n_Y as in
tests/expect_pauli_ref.py,

    (P psi)[j] = i^n_Y (-1)^popcount((j ^ x) & z) psi[j ^ x],        <phi| P |psi> = sum_j conj(phi[j]) (P psi)[j].

The bars, with u the unit roundoff of the state's precision (2^-53 for Complex<f64>, 2^-24 for Complex<f32>):

    Pauli sum, element by element:   |got_j - ref_j| <= (count + 8) u (sum_t |c_t| |src[j ^ x_t]| + |dst_old[j]|)
        at most count - 1 additions of coefficients, three roundings of a complex product, at most count accumulations, the
        final rounding; the same again, in double, for the reference.  (include/qip_hipx.h's own bound for the arithmetic it
        fixes is (m + 3) u sum + P u (sum + |dst_old|) for P passes of at most m terms, m + P <= count + 1: inside this bar.)
    matrix element:                  |got - ref| <= 1e-12 ||phi||_2 ||psi||_2
        expect_pauli's bar, with Cauchy-Schwarz in place of the square: double products, double sums.
    adjoint gradient, S = sum_t |c_t| over the observable, T rotations, `count` observable terms:
        |grad_k - ref_k| <= 2 S ||psi_0||^2 ((48 T + count + 8) u + 1e-12)
        |E - ref|        <=   S ||psi_0||^2 ((24 T + count + 8) u + 1e-12)
        from the bars above and the rotations' 12 R u ||psi||_2 (tests/pauli_rotation_ref.py): psi sees at most 2T rotations,
        lambda = H psi_T (||lambda|| <= S ||psi||) at most T plus the error it inherits from psi_T, then the sum's bar and the
        matrix element's bar."""
import math

import numpy as np

from expect_pauli_ref import all_strings, mask_cases, masks, parity, term_of_masks, term_of_string  # noqa: F401
from measure_ref import DTYPES, make_state, seed_of  # noqa: F401

SUM_SLACK = 8.0      # the "+ 8" of the Pauli sum's element bar
MELEM_BAR = 1e-12    # in units of ||phi||_2 ||psi||_2
ROTATION_BAR = 12.0  # R rotations: 12 R u ||psi||_2 (tests/pauli_rotation_ref.py)


def unit_roundoff(dtype):
    return 2.0 ** -53 if np.dtype(dtype) == np.complex128 else 2.0 ** -24


def _partner(n, term, ctype=np.complex128):
    """(k = j ^ x, i^n_Y (-1)^popcount(k & z)) for every j"""
    x, z, ny = masks(n, term)
    k = np.arange(1 << n, dtype=np.int64) ^ x
    sign = (1 - 2 * parity(k & z))
    phase = (1, 1j, -1, -1j)[ny % 4]
    return k, (phase * sign).astype(ctype)  # (exact: the entries are +-1 and +-i)


def apply_term(n, term, psi):
    """P psi, in the precision of `psi`"""
    k, f = _partner(n, term, psi.dtype)
    return f * psi[k]


def pauli_sum_ref(n, terms, coeffs, src, dst_old=None):
    """dst_old + (sum_t c_t P_t) src in complex128, from the amplitudes widened to double"""
    psi = np.asarray(src).astype(np.complex128)
    out = np.zeros(1 << n, dtype=np.complex128) if dst_old is None else np.asarray(dst_old).astype(np.complex128)
    for term, c in zip(terms, np.asarray(coeffs, dtype=np.complex128)):
        out = out + c * apply_term(n, term, psi)
    return out


def sum_bar(n, terms, coeffs, src, dst_old=None):
    """float64[2^n]: (count + 8) u (sum_t |c_t| |src[j ^ x_t]| + |dst_old[j]|), u that of src's precision"""
    a = np.abs(np.asarray(src).astype(np.complex128))
    j = np.arange(1 << n, dtype=np.int64)
    scale = np.zeros(1 << n) if dst_old is None else np.abs(np.asarray(dst_old).astype(np.complex128))
    for term, c in zip(terms, np.asarray(coeffs, dtype=np.complex128)):
        scale = scale + abs(c) * a[j ^ masks(n, term)[0]]
    return (len(terms) + SUM_SLACK) * unit_roundoff(np.asarray(src).dtype) * scale


def within_bar(got, ref, bar):
    """(ok, worst |got_j - ref_j| / bar_j over the elements with a positive bar)"""
    err = np.abs(np.asarray(got).astype(np.complex128) - ref)
    nz = bar > 0
    return bool(np.all(err <= bar)), (float(np.max(err[nz] / bar[nz])) if np.any(nz) else 0.0)


def sum_plan(n, terms, group):
    """the passes of the device call as lists of term numbers: sorted stably by x mask, every run cut at `group` terms"""
    order = sorted(range(len(terms)), key=lambda t: masks(n, terms[t])[0])
    passes = []
    for t in order:
        if passes and len(passes[-1]) < group and masks(n, terms[passes[-1][0]])[0] == masks(n, terms[t])[0]:
            passes[-1].append(t)
        else:
            passes.append([t])
    return passes


def pauli_sum_spec(n, terms, coeffs, src, dst_old=None, group=16):
    """The arithmetic include/qip_hipx.h fixes, restated in the precision of `src` (complex64 or complex128): per pass the
    signed sum of the coefficients k_t = c_t i^n_Y (rounded once) from +0 in term order, one complex product with separately
    rounded products, then a store (first pass, not accumulating) or one addition per component.  Only
    tests/test_pauli_pair_cpu.py uses it, to show that the bar can be met."""
    src = np.asarray(src)
    real = np.float32 if src.dtype == np.complex64 else np.float64
    coeffs = np.asarray(coeffs, dtype=np.complex128)
    sr, si = src.real.astype(real), src.imag.astype(real)
    j = np.arange(1 << n, dtype=np.int64)
    have = dst_old is not None
    dr = np.asarray(dst_old).real.astype(real) if have else np.zeros(1 << n, dtype=real)
    di = np.asarray(dst_old).imag.astype(real) if have else np.zeros(1 << n, dtype=real)
    if not terms and not have:
        return (dr + 1j * di).astype(src.dtype)
    for ids in sum_plan(n, terms, group):
        x = masks(n, terms[ids[0]])[0]
        k = j ^ x
        wr, wi = np.zeros(1 << n, dtype=real), np.zeros(1 << n, dtype=real)
        for t in ids:
            _, z, ny = masks(n, terms[t])
            kt = coeffs[t] * (1, 1j, -1, -1j)[ny % 4]
            sigma = (1 - 2 * parity(k & z)).astype(real)
            wr, wi = wr + sigma * real(kt.real), wi + sigma * real(kt.imag)
        pr, pi = wr * sr[k] - wi * si[k], wr * si[k] + wi * sr[k]
        assert pr.dtype == real
        dr, di = (dr + pr, di + pi) if have else (pr, pi)
        have = True
    out = np.empty(1 << n, dtype=src.dtype)
    out.real, out.imag = dr, di
    return out


def matrix_element_ref(n, term, bra, ket):
    """<bra| P |ket> of one term: the 2^n products in complex128 from the amplitudes widened to double, their real and their
    imaginary parts each summed with math.fsum"""
    phi = np.asarray(bra).astype(np.complex128)
    prod = np.conj(phi) * apply_term(n, term, np.asarray(ket).astype(np.complex128))
    return complex(math.fsum(prod.real), math.fsum(prod.imag))


def matrix_elements_ref(n, terms, bra, ket):
    return np.array([matrix_element_ref(n, t, bra, ket) for t in terms], dtype=np.complex128)


def melem_bar(bra, ket):
    norm = lambda v: float(np.linalg.norm(np.asarray(v).astype(np.complex128)))  # noqa: E731
    return MELEM_BAR * norm(bra) * norm(ket)


def rotate(n, term, theta, psi):
    """exp(-i theta P) psi = cos theta psi - i sin theta P psi, in the precision of `psi` (complex128 or clongdouble)"""
    real = psi.real.dtype.type
    return np.cos(real(theta)) * psi - psi.dtype.type(1j) * (np.sin(real(theta)) * apply_term(n, term, psi))


def ansatz_ref(n, rot_terms, angles, psi0, ctype=np.complex128):
    psi = np.asarray(psi0).astype(ctype)
    for term, theta in zip(rot_terms, angles):
        psi = rotate(n, term, theta, psi)
    return psi


def energy_ref(n, rot_terms, angles, obs_terms, obs_coeffs, psi0, ctype=np.complex128):
    """<psi_T| H |psi_T> of psi_T = R_{T-1} .. R_0 psi_0, in the precision `ctype`"""
    psi = ansatz_ref(n, rot_terms, angles, psi0, ctype)
    lam = np.zeros_like(psi)
    for term, c in zip(obs_terms, obs_coeffs):
        lam = lam + psi.real.dtype.type(c) * apply_term(n, term, psi)
    return np.vdot(lam, psi).real


def adjoint_gradient_ref(n, rot_terms, angles, obs_terms, obs_coeffs, psi0):
    """(E, grad) by the adjoint method on complex128 vectors: lambda = H psi_T, E = Re <lambda|psi_T>, then for k = T-1 .. 0:
    grad_k = 2 Im <lambda| P_k |psi> and both vectors rotated back by -theta_k"""
    psi = ansatz_ref(n, rot_terms, angles, psi0)
    lam = pauli_sum_ref(n, obs_terms, obs_coeffs, psi)
    energy = float(np.vdot(lam, psi).real)
    grad = np.zeros(len(rot_terms))
    for k in range(len(rot_terms) - 1, -1, -1):
        grad[k] = 2.0 * np.vdot(lam, apply_term(n, rot_terms[k], psi)).imag
        psi = rotate(n, rot_terms[k], -angles[k], psi)
        lam = rotate(n, rot_terms[k], -angles[k], lam)
    return energy, grad


def gradient_bars(rot_count, obs_coeffs, psi0):
    """(bar of E, bar of every grad_k) for a state of psi0's precision"""
    psi0 = np.asarray(psi0)
    S = float(np.sum(np.abs(obs_coeffs)))
    norm2 = float(np.linalg.norm(psi0.astype(np.complex128))) ** 2
    u, T, count = unit_roundoff(psi0.dtype), rot_count, len(obs_coeffs)
    return S * norm2 * ((24 * T + count + 8) * u + MELEM_BAR), 2 * S * norm2 * ((48 * T + count + 8) * u + MELEM_BAR)


def restore_bar(rot_count, psi0):
    """12 * 2T * u ||psi_0||_2: how far the state may be from psi_0 after T rotations forward and T back"""
    psi0 = np.asarray(psi0)
    return ROTATION_BAR * 2 * rot_count * unit_roundoff(psi0.dtype) * float(np.linalg.norm(psi0.astype(np.complex128)))


# ---- the cases of the GPU tests -------------------------------------------------------------------------------------------------
def batch_case(n):
    """(terms, coeffs) of the batch test, shaped like the rotation tests' batch_case: 67 terms over three x masks — 33 of a mask
    with bit 0 set (more than one pass under any group), the empty term, 20 of a mask with bit 0 clear, 5 of x = 0 (Z strings)
    and 8 of the first mask again; complex coefficients"""
    rng = np.random.default_rng(5200 + n)
    xa, xb = (1 << (n - 1)) | 0x21, 0x1C2
    terms = []
    for cx, count in ((xa, 33), (None, 1), (xb, 20), (0, 5), (xa, 8)):
        if cx is None:
            terms.append({})
            continue
        terms += [term_of_masks(n, cx, int(rng.integers(1, 1 << n))) for _ in range(count)]
    assert len(terms) == 67
    return terms, rng.standard_normal(67) + 1j * rng.standard_normal(67)


def batch_passes(group):
    """the passes batch_case makes at `group` terms per pass: sorted by mask, the runs are 6 (x = 0: the empty term and the Z
    strings), 20 and 41 terms long"""
    return sum(-(-run // group) for run in (6, 20, 41))


def gradient_case(n, seed=0):
    """(rot_terms, angles, obs_terms, obs_coeffs): T = 12 random strings with angles in (-3, 3), two consecutive ones of one x mask
    (positions 3 and 4) and a Z-only string (position 7); an observable of 10 terms with real coefficients, the identity among them"""
    rng = np.random.default_rng(6300 + 17 * n + seed)
    string = lambda: "".join(rng.choice(list("IXYZ"), n))  # noqa: E731
    rot = [term_of_string(string()) for _ in range(12)]
    x3, _, _ = masks(n, rot[3])
    rot[4] = term_of_masks(n, x3, int(rng.integers(1, 1 << n)))
    rot[7] = term_of_masks(n, 0, int(rng.integers(1, 1 << n)))
    assert masks(n, rot[3])[0] == masks(n, rot[4])[0] and masks(n, rot[7])[0] == 0
    angles = rng.uniform(-3.0, 3.0, 12)
    obs = [term_of_string(string()) for _ in range(9)] + [{}]
    return rot, angles, obs, rng.standard_normal(10)
