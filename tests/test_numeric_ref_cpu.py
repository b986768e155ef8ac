"""tests/numeric_ref.py checked on the CPU: the high-precision reference against exact rational arithmetic and against the
oracle (which pins the index convention), and numpy emulations of the arithmetic forms of the matrix-core dense kernels against
every cap that tests/test_gpu_a_dense_accuracy.py sets — correct arithmetic of each form meets them, a coarse data path and a
dropped term do not."""
from fractions import Fraction

import numpy as np
import pytest

import rustqip_amd as q

import numeric_ref as nr

DTYPES = [np.complex128, np.complex64]
TOL32_OLD = 1e-5  # the absolute bar the dense tests used to be held to alone


def _op(targets, controls, G, dtype):
    op = q.make_matrix_op(list(targets), np.asarray(G).astype(dtype).ravel())
    return q.make_control_op(list(controls), op) if controls else op


def _oracle(O, case):
    out = np.zeros_like(case.x)
    O.apply_op_overwrite(case.n, _op(case.targets, case.controls, case.G, case.x.dtype), case.x, out)
    if case.controls:  # (apply_op_overwrite writes the rows the controls select; the others travel as they are)
        m = nr.untouched_mask(case.n, case.targets, case.controls)
        out[m] = case.x[m]
    return out


def _frac(v):
    """a long double (or a double) as an exact Fraction: two doubles hold its 64 bits"""
    hi = float(v)
    return Fraction(hi) + Fraction(float(v - type(v)(hi)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("targets,controls", [([2, 0], [3]), ([1, 3, 0], [])])
def test_dense_reference_against_exact_rational_arithmetic(dtype, targets, controls):
    """n = 4, k = 2 with one control and k = 3: (a) inputs of 12 significant bits, where every sum fits the reference precision:
    the reference IS the exact result; (b) full-precision Gaussian inputs: within one rounding of the reference precision of
    it, i.e. within u_ref * a_r per accumulated term pair (2 * 2^k of them: Higham's bound for any order) — 2^-11 of the
    state's own rounding for complex128, so the reference is the long double one and not a double in disguise."""
    n, k = 4, len(targets)
    S = 1 << k
    rng = np.random.default_rng(k)
    u_ref = 2.0 ** -64 if dtype == np.complex128 else 2.0 ** -53
    for bits in (12, None):
        G = rng.standard_normal((S, S)) + 1j * rng.standard_normal((S, S))
        x = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
        if bits:
            G, x = np.rint(G * 2 ** bits) / 2 ** bits, np.rint(x * 2 ** bits) / 2 ** bits
        G, x = G.astype(dtype).astype(np.complex128), x.astype(dtype)
        idx, xg, ref = nr.dense_reference(n, targets, controls, G, x)
        assert idx.shape == (1 << (n - k - len(controls)), S)
        tpos, cpos = [n - 1 - t for t in targets], [n - 1 - c for c in controls]
        seen = set()
        for g in range(idx.shape[0]):
            for r in range(S):
                i = int(idx[g, r])
                seen.add(i)
                assert all((i >> p) & 1 for p in cpos)
                assert [(i >> p) & 1 for p in tpos] == [(r >> (k - 1 - j)) & 1 for j in range(k)]
                ere = eim = Fraction(0)
                a = Fraction(0)
                for c in range(S):
                    j = i
                    for jj, p in enumerate(tpos):
                        j = (j & ~(1 << p)) | (((c >> (k - 1 - jj)) & 1) << p)
                    gre, gim = Fraction(float(G[r, c].real)), Fraction(float(G[r, c].imag))
                    xre, xim = Fraction(float(x[j].real)), Fraction(float(x[j].imag))
                    ere += gre * xre - gim * xim
                    eim += gre * xim + gim * xre
                    a += (abs(gre) + abs(gim)) * (abs(xre) + abs(xim))
                for got, want in ((ref[g, r].real, ere), (ref[g, r].imag, eim)):
                    err = abs(_frac(got) - want)
                    if bits:
                        assert err == 0, (g, r)
                    else:
                        assert err <= 2 * S * Fraction(u_ref) * a, (g, r, float(err / a))
        assert len(seen) == idx.size


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [3, 6])
def test_dense_reference_against_the_oracle(O, dtype, k):
    """every input class x matrix class: the oracle's own scaled error is within the derived bound (a wrong index convention
    gives errors of 1 / u), and its rms is what the kernels' caps are multiples of"""
    n = 14
    rng = np.random.default_rng(k)
    perm = [int(v) for v in rng.permutation(n)]
    targets, controls = perm[:k], perm[k:k + 1]
    lines = []
    for mk in nr.MATRICES:
        G = nr.make_matrix(mk, k, dtype)
        for ik in nr.INPUTS:
            x = nr.make_state(ik, n, dtype, targets=targets, controls=controls, G=G)
            case = nr.Case(n, targets, controls, G, x)
            y = _oracle(O, case)
            rms, mx = case.errors(y)
            lines.append(f"{np.dtype(dtype).name} k={k} {mk:5s} {ik:8s} oracle rms(e)={rms:.3f} max|e|={mx:.3f}")
            assert mx <= nr.hard_bound(k), lines[-1]
            assert 0 < rms, lines[-1]
            assert case.untouched_equal(y)
    print("\n".join(lines))  # (pytest -s shows the figures)


def _emulation_cases(k, dtype):
    """(form, matrix classes): the two-product form takes matrices without an imaginary part only"""
    return [(nr.emulate_four_products, ("U", "iU", "orth", "wild")), (nr.emulate_three_products, ("U", "iU", "orth", "wild")),
            (nr.emulate_two_products, ("orth",))]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [3, 5, 7])
def test_emulations_of_the_arithmetic_forms_meet_every_cap(O, dtype, k):
    """four real products as fused chains, three products in mfma3_item's order with P, R, Q built in double and rounded once,
    two products: each within the derived bound, within 4 x the oracle's rms and 8 x the oracle's maximum, on every input class"""
    n = max(k + 7, 13)
    rng = np.random.default_rng(40 + k)
    targets = [int(v) for v in rng.permutation(n)[:k]]
    lines, worst = [], 0.0
    for form, mats in _emulation_cases(k, dtype):
        for mk in mats:
            G = nr.make_matrix(mk, k, dtype)
            for ik in nr.INPUTS:
                x = nr.make_state(ik, n, dtype, targets=targets, G=G)
                case = nr.Case(n, targets, [], G, x)
                eo = case.errors(_oracle(O, case))
                ek = case.errors(nr.apply_emulation(form, case))
                bad = nr.check_caps(k, ek, eo)
                lines.append(f"{np.dtype(dtype).name} k={k} {form.__name__[8:]:14s} {mk:5s} {ik:8s} oracle {eo[0]:.3f}/{eo[1]:.2f} "
                             f"emulation {ek[0]:.3f}/{ek[1]:.2f} ratio {ek[0] / eo[0]:.2f}/{ek[1] / eo[1]:.2f}")
                assert not bad, (lines[-1], bad)
                worst = max(worst, ek[0] / eo[0])
    print("\n".join(lines) + f"\nworst rms ratio {worst:.2f}")  # (pytest -s shows the figures)


def _int_case(k, n, dtype, mk):
    rng = np.random.default_rng(70 + k)
    targets = [int(v) for v in rng.permutation(n)[:k]]
    G = nr.make_matrix(mk, k, dtype)
    return nr.Case(n, targets, [], G, nr.make_int_state(n, dtype), reference=False)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [3, 5, 7])
def test_emulations_and_oracle_are_exact_on_integer_inputs_and_a_dropped_term_is_not(O, dtype, k):
    """Gaussian-integer matrices with entries in [-3, 3]^2 and the all-ones matrix on integer states in [-256, 256]: every partial sum
    of every form is an integer below 2^24, so both precisions give the int64 result — and a chain that leaves one term out
    does not"""
    n = max(k + 4, 10)
    for mk in ("gint", "ones"):
        case = _int_case(k, n, dtype, mk)
        wr, wi = nr.int_reference(n, case.targets, [], case.G, case.x)
        outs = [_oracle(O, case), nr.apply_emulation(nr.emulate_four_products, case), nr.apply_emulation(nr.emulate_three_products, case)]
        if mk == "ones":
            outs.append(nr.apply_emulation(nr.emulate_two_products, case))
        for y in outs:
            assert np.array_equal(y.real.astype(np.int64), wr) and np.array_equal(y.imag.astype(np.int64), wi)
            assert np.array_equal(y.real, wr) and np.array_equal(y.imag, wi)
        forms = [nr.emulate_four_products, nr.emulate_three_products] + ([nr.emulate_two_products] if mk == "ones" else [])
        r, c = (int(v) for v in np.argwhere(case.G.real != 0)[-1])  # a term that is not a zero anyway
        for form in forms:
            y = nr.apply_emulation(form, case, drop=(r, c))
            assert not (np.array_equal(y.real, wr) and np.array_equal(y.imag, wi)), form.__name__


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [3, 5, 7])
def test_emulations_and_oracle_are_bit_invariant_under_powers_of_two(O, dtype, k):
    """K(2^s x) == 2^s K(x) and K_{2^s G}(x) == 2^s K_G(x), compared as words, for s = -+200 (Complex<f32>: -+40)"""
    n = max(k + 4, 10)
    rng = np.random.default_rng(90 + k)
    targets = [int(v) for v in rng.permutation(n)[:k]]
    forms = [(_oracle, "U"), (lambda O_, c: nr.apply_emulation(nr.emulate_four_products, c), "U"),
             (lambda O_, c: nr.apply_emulation(nr.emulate_three_products, c), "U"), (lambda O_, c: nr.apply_emulation(nr.emulate_two_products, c), "orth")]
    for ik in ("normal", "range"):
        x = nr.make_state(ik, n, dtype)
        for form, mk in forms:
            G = nr.make_matrix(mk, k, dtype)
            base = form(O, nr.Case(n, targets, [], G, x, reference=False))
            for s in ((-200, 200) if dtype == np.complex128 else (-40, 40)):
                f = np.ldexp(1.0, s)
                want = (base * f).astype(dtype)
                assert nr.same_bits(form(O, nr.Case(n, targets, [], G, (x * f).astype(dtype), reference=False)), want), (ik, s, "x")
                assert nr.same_bits(form(O, nr.Case(n, targets, [], G * f, x, reference=False)), want), (ik, s, "G")


def test_a_coarse_data_path_passes_the_old_bar_and_fails_the_new_one(O):
    """the gap this closes: matrix fragments rounded to 8 mantissa bits in Complex<f32> pass max|got - oracle| <= 1e-5 on a
    normalised state of 19 qubits (amplitudes of 1e-3) and miss the scale-free caps on `range` (and on `normal`) by orders of magnitude"""
    n, k, dtype = 19, 4, np.complex64
    targets = [18, 17, 0, 1]
    G = nr.make_matrix("U", k, dtype)
    x = nr.make_state("normal", n, dtype)
    case = nr.Case(n, targets, [], G, x)
    want = _oracle(O, case)
    good = nr.apply_emulation(nr.emulate_four_products, case)
    coarse = nr.apply_emulation(nr.emulate_four_products, case, frag_bits=8)
    assert np.max(np.abs(coarse - want)) <= TOL32_OLD and np.max(np.abs(good - want)) <= TOL32_OLD
    assert not nr.check_caps(k, case.errors(good), case.errors(want))
    assert len(nr.check_caps(k, case.errors(coarse), case.errors(want))) == 3
    xr = nr.make_state("range", n, dtype)
    case = nr.Case(n, targets, [], G, xr)
    want = _oracle(O, case)
    assert not nr.check_caps(k, case.errors(nr.apply_emulation(nr.emulate_four_products, case)), case.errors(want))
    assert len(nr.check_caps(k, case.errors(nr.apply_emulation(nr.emulate_four_products, case, frag_bits=8)), case.errors(want))) == 3
