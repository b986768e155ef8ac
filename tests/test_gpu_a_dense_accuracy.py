"""The matrix-core dense kernels (k_gate_kq_mfma, k_gate_tile_mfma K = 4 / 5, k_gate_big_mfma, k_gate_huge_mfma) held to scale-free
bars — needs a real MI355X (`-m gpu`).

These kernels are not bit-equal to the oracle, and max|got - oracle| <= 1e-12 / 1e-5 on a normalised state says little (in
Complex<f32> at 19 qubits it is a relative bar of per cent).  Three families of checks (tests/numeric_ref.py has the reference, the
error measure e, the derived bound and the case table; tests/test_numeric_ref_cpu.py shows that correct arithmetic of every form
meets these caps and that a coarse data path or a dropped term does not):

  3a  accuracy against a reference in higher precision, for the kernel and for the oracle on the same input:
      max|e_kernel| <= hard_bound(k), rms(e_kernel) <= 4 rms(e_oracle), max|e_kernel| <= 8 max|e_oracle| — on normalised states,
      states of 2^20, states with forty binades of dynamic range, nearly real states, nearly cancelling groups; on unitary, real
      orthogonal and non-unitary matrices with zeros and entries over twenty binades;
  3b  K(2^s x) == 2^s K(x) and K_{2^s G}(x) == 2^s K_G(x) bit for bit on the whole vector, also for one op of every other kernel
      class that apply_op chooses at n = 12;
  3c  integer matrices on integer states: every form must give the int64 result exactly, in both precisions.

Every run asserts through profile() that the intended kernel class ran.
"""
import cmath

import numpy as np
import pytest

import rustqip_amd as q

import numeric_ref as nr

pytestmark = pytest.mark.gpu

CASES = nr.kernel_cases()
IDS = [kc.id for kc in CASES]


def _measure(O, dev, kc, name, targets, controls, mk, ik):
    ek, eo = nr.measure(O, q, dev, kc, targets, controls, mk, ik)
    line = (f"{kc.id} {name} {mk} {ik}: kernel rms {ek[0]:.3f} max {ek[1]:.2f}; oracle rms {eo[0]:.3f} max {eo[1]:.2f}; "
            f"ratio {ek[0] / eo[0]:.2f} / {ek[1] / eo[1]:.2f}; hard bound {nr.hard_bound(kc.k)}")
    print(line)
    return line, nr.check_caps(kc.k, ek, eo)


accuracy_parts = nr.accuracy_parts
ACCURACY = [(kc, part) for kc in CASES for part in accuracy_parts(kc)]


@pytest.mark.parametrize("kc,part", ACCURACY, ids=[f"{kc.id}-{part}" for kc, part in ACCURACY])
def test_3a_accuracy_against_a_higher_precision_reference(O, kc, part):
    failures = []
    with nr.HipRunner(q, kc) as dev:
        for name, targets, controls, mk, ik in accuracy_parts(kc)[part]:
            line, bad = _measure(O, dev, kc, name, targets, controls, mk, ik)
            if bad:
                failures.append((line, bad))
    assert not failures, failures


@pytest.mark.parametrize("kc", CASES, ids=IDS)
def test_3b_power_of_two_homogeneity_bit_for_bit(kc):
    """K(2^s x) == 2^s K(x) and K_{2^s G}(x) == 2^s K_G(x) as words, s = -+200 (Complex<f32>: -+40), on `normal` and `range`: every
    form is exactly homogeneous in binary floating point while nothing under- or overflows, so an absolute threshold,
    zero-skipping by magnitude or a constant that does not scale breaks this"""
    pl = {name: (t, c) for name, t, c in nr.placements(kc)}
    names = ["mixed0"] + (["mixed_ctl"] if "mixed_ctl" in pl else [])
    G = nr.make_matrix(kc.matrix, kc.k, kc.dtype)
    with nr.HipRunner(q, kc) as dev:
        for name in names:
            targets, controls = pl[name]
            outside = nr.untouched_mask(kc.n, targets, controls) if controls else None
            for ik in ("normal", "range"):
                x = nr.make_state(ik, kc.n, kc.dtype)
                base = dev.run(targets, controls, G, x)
                for s in ((-200, 200) if kc.dtype == np.complex128 else (-40, 40)):
                    f = np.ldexp(1.0, s)
                    want = (base * f).astype(kc.dtype)
                    assert nr.same_bits(dev.run(targets, controls, G, (x * f).astype(kc.dtype)), want), (kc, name, ik, s, "x")
                    if controls:  # (2^s G leaves the amplitudes outside the controlled half as they are)
                        want[outside] = x[outside]
                    assert nr.same_bits(dev.run(targets, controls, G * f, x), want), (kc, name, ik, s, "G")


def _other_class_ops(n, rng):
    """one op of every other class apply_op chooses at n = 12 (k_sparse_ell: 13, below which it is never chosen): (name, op builder
    from a scale factor and a precision, profile labels of the unscaled op).  Qubit t is bit position n-1-t."""
    g1 = rng.standard_normal(4) + 1j * rng.standard_normal(4)
    g2 = rng.standard_normal(16) + 1j * rng.standard_normal(16)
    g5 = rng.standard_normal(1 << 10) + 1j * rng.standard_normal(1 << 10)
    g9 = rng.standard_normal(1 << 18) + 1j * rng.standard_normal(1 << 18)
    ph = cmath.rect(1.0, 0.37)

    def sparse(idx, k, per):  # `per` stored entries in every row, the same rows for every scale
        rows = [[(int(c), complex(v)) for c, v in zip(rng.permutation(1 << k)[:per], rng.standard_normal(per) + 1j * rng.standard_normal(per))]
                for _ in range(1 << k)]
        return lambda f, dt: q.make_sparse_matrix_op(idx, [[(c, complex(np.asarray(v).astype(dt)) * f) for c, v in row] for row in rows])

    dense = lambda idx, g: (lambda f, dt: q.make_matrix_op(idx, (g.astype(dt) * f).astype(dt)))  # noqa: E731
    return [
        ("gate1q_pair", dense([0], g1), {"k_gate1q_pair"}),
        ("gate1q_cross_lane", dense([n - 3], g1), {"k_gate1q_xlane"}),
        ("gate1q_position0", dense([n - 1], g1), {"k_gate1q_xlane"}),  # (Complex<f32>: inside one packed element)
        ("phase", dense([2, n - 2], np.diag([1, 1, 1, ph]).ravel()), {"k_phase"}),
        ("diag1q", dense([3], np.array([ph.conjugate(), 0, 0, ph])), {"k_diag1q"}),
        ("diag", dense([1, n - 1], np.diag([ph, ph.conjugate(), 1j, -1]).ravel()), {"k_diag"}),
        ("dense2_register", dense([0, n - 1], g2), {"k_gate_kq"}),
        ("sparse2", sparse([n - 1, 0], 2, 2), {"k_sparse_kq"}),
        ("sparse6_tile", sparse([1, 2, 3, n - 1, n - 2, 5], 6, 2), {"k_sparse_tile"}),
        ("sparse7_ell", sparse([n, n - 1, n - 2, n - 3, n - 4, 0, 1], 7, 2), {"k_sparse_ell"}),  # (at n + 1 = 13 qubits, its smallest state)
        ("dense9_small", dense([0, 2, 3, 4, 5, 7, 8, 10, 11], g9), {"k_dense_small"}),
        ("dense5_literal", dense([0, 2, 5, 7, 11], g5), {"k_gather_generic"}),
    ]


@pytest.mark.parametrize("dtype", [np.complex128, np.complex64], ids=["f64", "f32"])
def test_3b_power_of_two_homogeneity_of_the_other_kernel_classes(dtype):
    ops = _other_class_ops(12, np.random.default_rng(12))
    for ik in ("normal", "range"):
        for name, build, labels in ops:
            n = 13 if name == "sparse7_ell" else 12
            x = nr.make_state(ik, n, dtype)

            def run(op, xx, check_label):
                with q.HipState(n, dtype) as st:
                    st.set_option("profile", 1)
                    if name == "dense5_literal":
                        st.set_option("force_generic", 1)
                    st.upload(xx)
                    st.apply_op(op)
                    y = st.download()
                    if check_label:
                        assert set(st.profile()) == labels, (name, st.profile())
                    return y

            base = run(build(1.0, dtype), x, True)
            for s in ((-200, 200) if dtype == np.complex128 else (-40, 40)):
                f = np.ldexp(1.0, s)
                want = (base * f).astype(dtype)
                assert nr.same_bits(run(build(1.0, dtype), (x * f).astype(dtype), True), want), (name, ik, s, "x")
                # (2^s G may be another class — a diagonal of ones and one phase is a diagonal of four entries — which must agree too)
                assert nr.same_bits(run(build(f, dtype), x, False), want), (name, ik, s, "G")


@pytest.mark.parametrize("kc", CASES, ids=IDS)
def test_3c_integer_inputs_are_exact(kc):
    """Gaussian-integer matrices with entries in [-3, 3]^2 (real integers for the two-product cases; the all-ones matrix once for every case) on
    integer states in [-256, 256]: every partial sum of every form is an integer below 2^24 (worst case 2^10 * 6 * 512), so both
    precisions must give the int64 result — an accumulating matrix-core path held to equality"""
    pl = nr.placements(kc)
    pl = [pl[2], pl[-1]] + ([pl[0]] if kc.n < 20 else [])  # a mixed placement, the last one (controlled / on the split position), the lowest positions
    x = nr.make_int_state(kc.n, kc.dtype)
    runs = [("gint" if kc.matrix == "U" else "rint", p) for p in pl] + [("ones", pl[0])]
    with nr.HipRunner(q, kc) as dev:
        for mk, (name, targets, controls) in runs:
            G = nr.make_matrix(mk, kc.k, kc.dtype)
            wr, wi = nr.int_reference(kc.n, targets, controls, G, x)
            y = dev.run(targets, controls, G, x)
            bad = np.flatnonzero((y.real != wr) | (y.imag != wi))
            assert bad.size == 0, (kc, mk, name, bad.size, bad[:4], y[bad[:4]], wr[bad[:4]], wi[bad[:4]])
