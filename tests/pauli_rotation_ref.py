"""A reference for Pauli-string rotations exp(-i theta P), independent of the code under test, the two bars the tests hold the
device call to, and the cases they run — shared by tests/test_pauli_rotation_cpu.py and tests/test_gpu_f1_pauli_rotation.py.  A
plain helper module: numpy only, no fixtures.

A term is a mapping {qubit: "I" | "X" | "Y" | "Z"}; qubit q is amplitude-index bit n - 1 - q.  With x, z, n_Y as in
tests/expect_pauli_ref.py,

    exp(-i theta P) psi = cos theta psi - i sin theta P psi,      (P psi)[j] = i^n_Y (-1)^popcount((j ^ x) & z) psi[j ^ x].

The bars (include/qip_hipx.h fixes the arithmetic: c = cos theta and s = sin theta rounded once to the state's precision, every
new component fl(fl(c u) + fl(s v)), the factor -i i^n_Y (+-1) exact).  With u the unit roundoff — 2^-53 for Complex<f64>, 2^-24
for Complex<f32> — a component errs by at most 4u(|c||u_comp| + |s||v_comp|): two products, one sum, the rounding of c and s.
By Cauchy-Schwarz:

    one rotation, element by element:   |got_j - ref_j| <= 12 u (|psi_j| + |psi_{j^x}|)
                                        (5.7 for the code under test, the same again for a complex128 reference, rounded up)
    R rotations in sequence:            ||got - ref||_2 <= 12 R u ||psi||_2          (every rotation is unitary)

Both hold for every correct implementation."""
import numpy as np

from expect_pauli_ref import all_strings, mask_cases, masks, parity, term_of_masks, term_of_string  # noqa: F401
from measure_ref import DTYPES, make_state, seed_of  # noqa: F401

BAR = 12.0
ANGLES = (0.0, 0.7, -1.9, 4.0)


def unit_roundoff(dtype):
    return 2.0 ** -53 if np.dtype(dtype) == np.complex128 else 2.0 ** -24


def _partner(n, term):
    """(k = j ^ x, i^n_Y (-1)^popcount(k & z)) for every j"""
    x, z, ny = masks(n, term)
    k = np.arange(1 << n, dtype=np.int64) ^ x
    return k, ((1j) ** (ny % 4)) * (1.0 - 2.0 * parity(k & z))


def rotate_ref(n, term, theta, amps):
    """exp(-i theta P) psi in complex128, from the amplitudes widened to double"""
    psi = np.asarray(amps).astype(np.complex128)
    k, f = _partner(n, term)
    return np.cos(theta) * psi - 1j * np.sin(theta) * (f * psi[k])


def rotate_many_ref(n, terms, thetas, amps):
    psi = np.asarray(amps).astype(np.complex128)
    for term, theta in zip(terms, thetas):
        psi = rotate_ref(n, term, theta, psi)
    return psi


def rotate_spec(n, term, theta, amps):
    """The arithmetic the header specifies, restated in the precision of `amps` (complex64 or complex128): c and s rounded once,
    the two products of a component rounded separately, then their sum.  Only tests/test_pauli_rotation_cpu.py uses it, to show
    that the bars can be met."""
    amps = np.asarray(amps)
    real = np.float32 if amps.dtype == np.complex64 else np.float64
    x, z, ny = masks(n, term)
    k = np.arange(1 << n, dtype=np.int64) ^ x
    sigma = (1 - 2 * parity(k & z)).astype(real)
    re, im = amps.real.astype(real), amps.imag.astype(real)
    pr, pi = re[k] * sigma, im[k] * sigma  # (exact: sigma is +-1)
    vr, vi = ((pr, pi), (-pi, pr), (-pr, -pi), (pi, -pr))[(ny + 3) % 4]  # -i i^n_Y = i^(n_Y + 3)
    c, s = real(np.cos(float(theta))), real(np.sin(float(theta)))
    out = np.empty_like(amps)
    out.real = c * re + s * vr
    out.imag = c * im + s * vi
    assert (c * re).dtype == real
    return out


def rotate_many_spec(n, terms, thetas, amps):
    for term, theta in zip(terms, thetas):
        amps = rotate_spec(n, term, theta, amps)
    return amps


def element_bar(n, term, amps):
    """float64[2^n]: 12 u (|psi_j| + |psi_{j^x}|)"""
    a = np.abs(np.asarray(amps).astype(np.complex128))
    x = masks(n, term)[0]
    return BAR * unit_roundoff(np.asarray(amps).dtype) * (a + a[np.arange(1 << n, dtype=np.int64) ^ x])


def sequence_bar(count, amps):
    """12 R u ||psi||_2"""
    a = np.asarray(amps)
    return BAR * count * unit_roundoff(a.dtype) * float(np.linalg.norm(a.astype(np.complex128)))


def within_element_bar(n, term, got, ref, amps):
    """(ok, worst |got - ref| in units of u (|psi_j| + |psi_{j^x}|))"""
    err = np.abs(np.asarray(got).astype(np.complex128) - ref)
    bar = element_bar(n, term, amps)
    ok = bool(np.all(err <= bar))
    nz = bar > 0
    worst = float(np.max(err[nz] / bar[nz])) * BAR if np.any(nz) else 0.0
    return ok, worst


def within_sequence_bar(count, got, ref, amps):
    """(ok, ||got - ref||_2 in units of R u ||psi||_2)"""
    err = float(np.linalg.norm(np.asarray(got).astype(np.complex128) - ref))
    bar = sequence_bar(count, amps)
    return err <= bar, err / bar * BAR


# ---- the cases of the GPU tests -------------------------------------------------------------------------------------------------
def single_cases(n):
    """(name, term, theta): every case of mask_cases(n) as one rotation, the angles of ANGLES in turn (shifted so that every
    angle meets x = 0 and a pair mask)"""
    return [(name, term_of_masks(n, cx, cz), ANGLES[(i + i // 4) % 4]) for i, (name, cx, cz) in enumerate(mask_cases(n))]


def batch_case(n):
    """(terms, angles) of the batch test: 67 terms in runs over three x masks — 33 of a mask with bit 0 set (longer than the
    largest group), the empty term, 20 of a mask with bit 0 clear, 5 of x = 0 (Z strings), and 8 of the first mask again after
    the others.  Random z masks: neighbouring terms of one x mask with n_Y of both parities (they anticommute)."""
    rng = np.random.default_rng(4100 + n)
    xa, xb = (1 << (n - 1)) | 0x21, 0x1C2
    terms = []
    for cx, count in ((xa, 33), (None, 1), (xb, 20), (0, 5), (xa, 8)):
        if cx is None:
            terms.append({})
            continue
        terms += [term_of_masks(n, cx, int(rng.integers(1, 1 << n))) for _ in range(count)]
    angles = rng.uniform(-3.0, 3.0, len(terms))
    assert len(terms) == 2 * 32 + 3
    ny = [masks(n, t)[2] for t in terms]
    assert any(masks(n, terms[i])[0] == masks(n, terms[i + 1])[0] != 0 and (ny[i] + ny[i + 1]) % 2 for i in range(len(terms) - 1))
    return terms, angles


def batch_passes(group):
    """the passes batch_case makes at `group` terms per pass: runs of 33, 1 + 5 apart (the empty term is x = 0 but the run of
    the second mask lies between), 20, 5, 8"""
    return sum(-(-run // group) for run in (33, 1, 20, 5, 8))
