"""A reference for the diagonal Pauli sums (include/qip_hipx.h: qipx_state_apply_diagonal, qipx_state_expect_diagonal), the stated
arithmetic restated in numpy, and the bars the tests hold the device calls to — shared by tests/test_diagonal_cpu.py and
tests/test_gpu_f2_diagonal.py.  A plain helper module: numpy only, no fixtures.

A term is a mapping {qubit: "I" | "Z"}; qubit q is amplitude-index bit n - 1 - q; z_t is the term's mask over index bits and

    D(j) = sum_t c_t (-1)^popcount(j & z_t).

The reference.  All D(j) at once are the Walsh-Hadamard transform of a[z] = sum_{t : z_t = z} c_t, formed here in np.longdouble
(64-bit significand): T + n additions of relative error 2^-64 each, 2^-11 of the double-precision budget below, which is what
"negligible" means here.  energies_brute sums term by term instead (tests/test_diagonal_cpu.py holds the two together).
phase_ref and moments_ref take the amplitudes widened to longdouble and round nothing to double.

The spec.  phase_spec and moments_spec restate the header's arithmetic: k_t = fl(gamma c_t), the energy E^ in double per tile of
2^L amplitudes (L = min(n, TILE_BITS)) — a_h[m] the sum of (+-)k_t over the terms of low mask m in the order of the call from +0,
then the butterfly over bits 0 .. L-1 ascending — then (cos, sin) in double rounded once to the state's precision and
fl(fl(c re) + fl(s im)), fl(fl(c im) - fl(s re)); for the moments p = fl(fl(re re) + fl(im im)) in double, fl(p E^), fl(fl(p E^) E^).
energy_spec is bit for bit the library's host reference (qip_diag_plan.h: diag_tile_energies).

The bars, with u the unit roundoff of the state (2^-53 Complex<f64>, 2^-24 Complex<f32>), T terms, L = TILE_BITS,
A = sum_t |gamma c_t|, A1 = sum_t |c_t|, c(n) the longest chain of additions of the moments' reduction (chain_length, as the
header states it):

    phase, element by element:   |got_j - ref_j| <= [12 u + (T + L + 8) 2^-53 A] |psi_j|
        12 u: the rotation tests' bar of one unit-modulus complex multiply with rounded c, s (tests/pauli_rotation_ref.py).
        The second part: E^ differs from gamma D(j) by one rounding of every k_t (2^-53 |k_t| each, 2^-53 A together) and at most
        T + L additions whose partial sums are bounded by A (2^-53 A each), and |exp(-i a) - exp(-i b)| <= |a - b|; a few ulps of
        the double sine and cosine, and the margin, are the 8.
    moments:   |m1 - ref| <= (T + L + c(n) + 6) 2^-53 A1 |psi|^2
               |m2 - ref| <= (2 (T + L) + c(n) + 10) 2^-53 A1^2 |psi|^2
        p_j has relative error 2 * 2^-53 (two products, one sum; the f32 amplitudes widen exactly), E^ as above with |E^| <= A1,
        one rounding per product, c(n) additions of non-cancelling magnitude at most A1 |psi|^2 (A1^2 |psi|^2); E^ enters m2 twice.

They come from the stated arithmetic and hold for every implementation of it."""
import numpy as np

from expect_pauli_ref import masks, parity, term_of_masks  # noqa: F401
from measure_ref import DTYPES, make_state, seed_of  # noqa: F401

TILE_BITS = 12  # kDiagTileBits of rustqip_amd/csrc/qip_diag_plan.h
BAR = 12.0
MAX_TERMS = 1 << 20  # the cap of one call


def unit_roundoff(dtype):
    return 2.0 ** -53 if np.dtype(dtype) == np.complex128 else 2.0 ** -24


def z_term(n, z):
    """the term of Z factors on the index bits of `z`"""
    return term_of_masks(n, 0, int(z))


def z_of(n, term):
    x, z, _ = masks(n, term)
    assert x == 0
    return z


def chain_length(n):
    """c(n) of include/qip_hipx.h (diag_chain_length)"""
    if n < TILE_BITS:
        return max(1, (1 << n) >> 8) + 11
    return 16 * max(1, 1 << max(n - 24, 0)) + 6 + 4 + min(4096, 1 << (n - TILE_BITS))


# ---- the reference -------------------------------------------------------------------------------------------------------------
def _wht(a, bits):
    """in place over the last `bits` index bits of the flat array `a`, stage bit 0 first: (u, v) -> (u + v, u - v)"""
    for s in range(bits):
        v = a.reshape(-1, 2, 1 << s)
        u0, u1 = v[:, 0, :].copy(), v[:, 1, :].copy()
        v[:, 0, :] = u0 + u1
        v[:, 1, :] = u0 - u1
    return a


def energies_ref(n, zs, coeffs):
    """longdouble[2^n]: D(j)"""
    a = np.zeros(1 << n, dtype=np.longdouble)
    np.add.at(a, np.asarray(zs, dtype=np.int64), np.asarray(coeffs, dtype=np.float64).astype(np.longdouble))
    return _wht(a, n)


def energies_brute(n, zs, coeffs):
    j = np.arange(1 << n, dtype=np.int64)
    d = np.zeros(1 << n, dtype=np.longdouble)
    for z, c in zip(zs, coeffs):
        d += np.longdouble(c) * (1 - 2 * parity(j & int(z))).astype(np.longdouble)
    return d


def _wide(amps):
    a = np.asarray(amps)
    return a.real.astype(np.longdouble), a.imag.astype(np.longdouble)


def phase_ref(n, zs, coeffs, gamma, amps):
    """(re, im) in longdouble of exp(-i gamma D(j)) psi[j]"""
    angle = np.longdouble(gamma) * energies_ref(n, zs, coeffs)
    c, s = np.cos(angle), np.sin(angle)
    re, im = _wide(amps)
    return c * re + s * im, c * im - s * re


def moments_ref(n, zs, coeffs, amps):
    d = energies_ref(n, zs, coeffs)
    re, im = _wide(amps)
    p = re * re + im * im
    return float(np.sum(p * d)), float(np.sum(p * d * d))


# ---- the stated arithmetic -----------------------------------------------------------------------------------------------------
def energy_spec(n, zs, ks):
    """float64[2^n]: E^(j) in the stated order of operations"""
    L = min(n, TILE_BITS)
    zs = np.asarray(zs, dtype=np.int64).reshape(-1)
    ks = np.asarray(ks, dtype=np.float64).reshape(-1)
    order = np.argsort(zs & ((1 << L) - 1), kind="stable")  # (groups by low mask keep the order of the call)
    zlo, zhi, k = (zs & ((1 << L) - 1))[order], (zs >> L)[order], ks[order]
    out = np.empty(1 << n, dtype=np.float64)
    for h in range(1 << (n - L)):
        a = np.zeros(1 << L, dtype=np.float64)
        np.add.at(a, zlo, np.where(parity(zhi & h) == 1, -k, k))  # (unbuffered: one addition per term, in order)
        out[h << L:(h + 1) << L] = _wht(a, L)
    return out


def phase_spec(n, zs, coeffs, gamma, amps):
    amps = np.asarray(amps)
    real = np.float32 if amps.dtype == np.complex64 else np.float64
    e = energy_spec(n, zs, np.float64(gamma) * np.asarray(coeffs, dtype=np.float64))
    c, s = np.cos(e).astype(real), np.sin(e).astype(real)
    re, im = amps.real.astype(real), amps.imag.astype(real)
    out = np.empty_like(amps)
    out.real = c * re + s * im
    out.imag = c * im - s * re
    assert (c * re).dtype == real
    return out


def moments_spec(n, zs, coeffs, amps):
    amps = np.asarray(amps)
    e = energy_spec(n, zs, coeffs)
    re, im = amps.real.astype(np.float64), amps.imag.astype(np.float64)
    pe = (re * re + im * im) * e
    return float(np.sum(pe)), float(np.sum(pe * e))


# ---- the bars ------------------------------------------------------------------------------------------------------------------
def phase_bar(n, count, weight, amps):
    """float64[2^n]: [12 u + (T + L + 8) 2^-53 A] |psi_j|, `weight` = A = sum_t |gamma c_t|"""
    a = np.asarray(amps)
    return (BAR * unit_roundoff(a.dtype) + (count + TILE_BITS + 8) * 2.0 ** -53 * weight) * np.abs(a.astype(np.complex128))


def within_phase_bar(n, count, weight, got, ref, amps):
    """(ok, the worst |got - ref| as a fraction of the bar); `ref` = phase_ref's pair"""
    g = np.asarray(got)
    dr, di = g.real.astype(np.longdouble) - ref[0], g.imag.astype(np.longdouble) - ref[1]
    err = np.sqrt(dr * dr + di * di).astype(np.float64)
    bar = phase_bar(n, count, weight, amps)
    nz = bar > 0
    worst = float(np.max(err[nz] / bar[nz])) if np.any(nz) else 0.0
    return bool(np.all(err <= bar)), worst


def moment_bars(n, count, weight1, amps=None, norm=None):
    """(bar of m1, bar of m2), `weight1` = A1 = sum_t |c_t|; the state's |psi|^2 from `amps`, or given as `norm`"""
    if norm is None:
        a = np.asarray(amps).astype(np.complex128)
        norm = float(np.sum(a.real * a.real + a.imag * a.imag))
    c = chain_length(n)
    return ((count + TILE_BITS + c + 6) * 2.0 ** -53 * weight1 * norm,
            (2 * (count + TILE_BITS) + c + 10) * 2.0 ** -53 * weight1 * weight1 * norm)


# ---- the cases -----------------------------------------------------------------------------------------------------------------
def random_case(n, count, seed, scale=1.0, low=None, high=None):
    """(z masks, coefficients): `count` random masks (repeats happen, 0 = the empty term may), normal coefficients times `scale`;
    `low` / `high`: masks confined to the index bits below / at and above that position"""
    rng = np.random.default_rng(seed)
    zs = rng.integers(0, 1 << n, count, dtype=np.int64)
    if low is not None:
        zs &= (1 << low) - 1
    if high is not None:
        zs &= ~((1 << high) - 1)
    return [int(z) for z in zs], rng.standard_normal(count) * scale


def single_cases(n):
    """(name, z masks, coefficients) with T = 1: every single Z, ZZ across the tile boundary (and across bit 0 / 1, the halves of a
    packed element), the all-Z string, the empty term alone"""
    cases = [(f"Z{b}", [1 << b], [0.9]) for b in range(n)]
    cases.append(("allZ", [(1 << n) - 1], [-1.3]))
    cases.append(("empty", [0], [0.6]))
    if n >= 2:
        cases.append(("ZZ01", [3], [1.1]))
        cases.append(("ZZtop", [(1 << (n - 1)) | 1], [0.8]))
    if n > TILE_BITS:
        cases.append(("ZZboundary", [(1 << TILE_BITS) | (1 << (TILE_BITS - 1))], [-0.7]))
    return cases
