"""Pauli-string rotations exp(-i theta P) on a device state (include/qip_hipx.h: qipx_state_apply_pauli_rotations,
HipState.apply_pauli_rotations / evolve): k_pauli_rotate's single-amplitude (x = 0) and pair passes, plain and packed
Complex<f32> elements, every slot capacity, the grouping of consecutive terms into passes (rustqip_amd/csrc/qip_pauli.hip).

The reference and the two bars are those of tests/pauli_rotation_ref.py, with u = 2^-53 (Complex<f64>) or 2^-24 (Complex<f32>):

    one rotation, element by element:   |got_j - ref_j| <= 12 u (|psi_j| + |psi_{j^x}|)
    R rotations in sequence:            ||got - ref||_2 <= 12 R u ||psi||_2

k_pauli_rotate walks k_expect_pauli's geometry, so the sizes are those of the expect tests: n = 9 is the row loop of one block
(half a block's lanes for pairs of packed Complex<f32> elements), n = 13 one whole span per block or two blocks, n = 22 hundreds
of blocks.  Every test prints its worst figure before it asserts."""
import ctypes as C
import subprocess

from gpu_common import *  # noqa: F401,F403

import pauli_rotation_ref as P
from rustqip_amd import _ffi
from test_gpu_f1_expect_pauli import MANY_BLOCK_MASKS

pytestmark = pytest.mark.gpu

_IDS = ("c128", "c64")
_STATES = {}
GROUP_DEFAULT = 16  # the default of option "rotate_group"


def _state(n, dtype, norm=1.0):
    """the case state of (n, dtype, norm): shared, never written to"""
    key = (n, np.dtype(dtype), norm)
    if key not in _STATES:
        x = P.make_state(n, P.seed_of(n, dtype), dtype, norm=norm)
        x.setflags(write=False)
        _STATES[key] = x
    return _STATES[key]


def _rotated(st, x, terms, angles):
    st.upload(x)
    st.apply_pauli_rotations(terms, angles)
    return st.download()


def _hold_element(n, term, theta, got, x, what):
    ok, worst = P.within_element_bar(n, term, got, P.rotate_ref(n, term, theta, x), x)
    print(f"{what}: worst |got - ref| = {worst:.2f} u (|psi_j| + |psi_jx|), bar {P.BAR}")
    assert ok, what
    return worst


def _hold_sequence(count, got, ref, x, what):
    ok, worst = P.within_sequence_bar(count, got, ref, x)
    print(f"{what}: |got - ref|_2 = {worst:.3f} R u |psi|_2 (R = {count}), bar {P.BAR}")
    assert ok, what


# ---- 1, 2: single rotations, element by element -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", P.DTYPES, ids=_IDS)
def test_tiny_vectors(dtype):
    """fewer amplitudes than one wave: every Pauli string on n = 1, 2 and 3, one call each on a fresh upload"""
    for n in (1, 2, 3):
        x = _state(n, dtype, 0.8)
        worst = 0.0
        with q.HipState(n, dtype) as st:
            for s in P.all_strings(n):
                for theta in (0.3, -2.5):
                    got = _rotated(st, x, [s], [theta])  # (the string form of a term)
                    ok, w = P.within_element_bar(n, P.term_of_string(s), got, P.rotate_ref(n, P.term_of_string(s), theta, x), x)
                    assert ok, (n, s, theta, w)
                    worst = max(worst, w)
        print(f"n={n}: worst {worst:.2f} u (|psi_j| + |psi_jx|), bar {P.BAR}")


@pytest.mark.parametrize("norm", (1.0, 0.5))
@pytest.mark.parametrize("n", (9, 13))
@pytest.mark.parametrize("dtype", P.DTYPES, ids=_IDS)
def test_one_block_and_several_blocks(dtype, n, norm):
    """every case of mask_cases(n) as a single rotation on a fresh upload: x = 0, x = bit 0 alone (inside a packed Complex<f32>
    element: the unpacked pair pass), the top bit, all bits, n_Y = 1 .. 5 with bit 0 set and clear; the angles 0, 0.7, -1.9, 4.0"""
    x = _state(n, dtype, norm)
    cases = P.single_cases(n)
    assert sorted({P.masks(n, t)[2] for _, t, _ in cases}) == [0, 1, 2, 3, 4, 5]
    assert {theta for _, _, theta in cases} == set(P.ANGLES)
    with q.HipState(n, dtype) as st:
        for name, term, theta in cases:
            got = _rotated(st, x, [term], [theta])
            _hold_element(n, term, theta, got, x, f"n={n} norm={norm} {name} theta={theta}")
            if theta == 0.0:
                assert np.array_equal(got, x), name  # c = 1, s = 0: fl(u + 0) = u (no amplitude of the case state is -0)


# ---- 3: many blocks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(MANY_BLOCK_MASKS))
@pytest.mark.parametrize("dtype", P.DTYPES, ids=_IDS)
def test_many_blocks(dtype, which):
    """n = 22: hundreds of blocks, whole spans of four (x = 0) or two (pairs) elements per lane and row in each.  The four terms
    of a family as one call at the sequence bar, the first alone at the element bar."""
    n = 22
    x = _state(n, dtype)
    terms = [P.term_of_masks(n, cx, cz) for cx, cz in MANY_BLOCK_MASKS[which]]
    angles = [0.7, -1.9, 4.0, 0.3]
    with q.HipState(n, dtype) as st:
        first = _rotated(st, x, terms[:1], angles[:1])
        got = _rotated(st, x, terms, angles)
    _hold_element(n, terms[0], angles[0], first, x, f"n={n} {which} first term")
    _hold_sequence(len(terms), got, P.rotate_many_ref(n, terms, angles, x), x, f"n={n} {which}")


# ---- 4: a batch is its single-term calls, bit for bit ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", (9, 13))
@pytest.mark.parametrize("dtype", P.DTYPES, ids=_IDS)
def test_a_batch_leaves_the_bits_of_the_single_term_calls(dtype, n):
    """67 terms in runs over three x masks (bit 0 set, bit 0 clear, zero): a run longer than 32, anticommuting neighbours of one
    mask, an empty term, a repeated mask after a different one; one call under rotate_group = 1, 4, the default and 32 (every
    kernel capacity: runs of 33, 20, 8, 5 and 1 terms) and the single-term calls in sequence"""
    x = _state(n, dtype)
    terms, angles = P.batch_case(n)
    assert q.pauli_rotation_passes(n, terms) == P.batch_passes(GROUP_DEFAULT)
    downloads = {}
    with q.HipState(n, dtype) as st:
        st.upload(x)
        for t, theta in zip(terms, angles):
            st.apply_pauli_rotations([t], [theta])
        downloads["singles"] = st.download()
        downloads["default"] = _rotated(st, x, terms, angles)
        for group in (1, 4, 16, 32):
            st.set_option("rotate_group", group)
            downloads[group] = _rotated(st, x, terms, angles)
    raw = {k: v.view(np.uint8) for k, v in downloads.items()}
    for k, v in raw.items():
        assert np.array_equal(v, raw["singles"]), k
    _hold_sequence(len(terms), downloads["singles"], P.rotate_many_ref(n, terms, angles, x), x, f"n={n} batch")


# ---- 5: the order is kept ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", P.DTYPES, ids=_IDS)
def test_order_is_kept(dtype):
    n = 9
    x = _state(n, dtype)
    tx, tz = {0: "X"}, {0: "Z"}
    with q.HipState(n, dtype) as st:
        xz = _rotated(st, x, [tx, tz], [0.6, 0.6])
        zx = _rotated(st, x, [tz, tx], [0.6, 0.6])
    _hold_sequence(2, xz, P.rotate_many_ref(n, [tx, tz], [0.6, 0.6], x), x, "X then Z")
    _hold_sequence(2, zx, P.rotate_many_ref(n, [tz, tx], [0.6, 0.6], x), x, "Z then X")
    apart = float(np.linalg.norm(xz.astype(np.complex128) - zx.astype(np.complex128)))
    print(f"the two orders are {apart / P.sequence_bar(2, x):.3e} bars apart")
    assert apart > 100 * P.sequence_bar(2, x)


# ---- 6: invariants through the existing calls -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (9, 13))
@pytest.mark.parametrize("dtype", P.DTYPES, ids=_IDS)
def test_norm_and_own_expectation_are_kept(dtype, n):
    """exp(-i theta P) is unitary and commutes with P: norm_sqr and <psi|P|psi> agree before and after, within 2 * 12 u norm^2
    (the rotation's error, in the square) plus expect_pauli's documented 1e-12 norm^2"""
    x = _state(n, dtype, 0.5)
    u = P.unit_roundoff(dtype)
    with q.HipState(n, dtype) as st:
        for name, term, _ in P.single_cases(n)[::3]:
            st.upload(x)
            norm0, e0 = st.norm_sqr(), st.expect_pauli([term])[0]
            st.apply_pauli_rotations([term], [0.7])
            norm1, e1 = st.norm_sqr(), st.expect_pauli([term])[0]
            print(f"n={n} {name}: norm {abs(norm1 - norm0):.3e}, expectation {abs(e1 - e0):.3e}, bar {2 * P.BAR * u * norm0:.3e}")
            assert abs(norm1 - norm0) <= 2 * P.BAR * u * norm0, name
            assert abs(e1 - e0) <= (2 * P.BAR * u + 1e-12) * norm0, name


# ---- 7: against the existing gate path -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", P.DTYPES, ids=_IDS)
def test_against_apply_op(dtype):
    """exp(-i theta Z_q) is diag(e^{-i theta}, e^{i theta}) on q; exp(-i theta X_a Y_b) is a dense 4 x 4 op on (a, b).  The
    difference stays within the sequence bar (R = 1; the 2-norm bounds every element) plus gpu_common's bar of a dense op"""
    n, theta = 13, 0.7
    x = _state(n, dtype)
    tol = TOL64 if dtype == np.complex128 else TOL32
    X, Y = np.array([[0, 1], [1, 0]]), np.array([[0, -1j], [1j, 0]])
    xy = np.cos(theta) * np.eye(4) - 1j * np.sin(theta) * np.kron(X, Y)  # (a is the op's first index: the more significant)
    cases = [({qb: "Z"}, q.make_matrix_op([qb], [cmath.rect(1, -theta), 0, 0, cmath.rect(1, theta)])) for qb in (n - 1, 0, 5)]
    cases += [({a: "X", b: "Y"}, q.make_matrix_op([a, b], xy.ravel())) for a, b in ((n - 1, 0), (0, n - 1), (3, n - 1), (0, 6))]
    with q.HipState(n, dtype) as st:
        for term, op in cases:
            got = _rotated(st, x, [term], [theta])
            st.upload(x)
            st.apply_op(op)
            want = st.download()
            d = float(np.max(np.abs(got.astype(np.complex128) - want.astype(np.complex128))))
            print(f"{term}: max |rotation - apply_op| = {d:.3e}, bar {P.sequence_bar(1, x) + tol:.3e}")
            assert d <= P.sequence_bar(1, x) + tol, term


# ---- 8: a relabelled state -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", P.DTYPES, ids=_IDS)
def test_relabelled_state(dtype):
    """tile = 1 with tile_relabel = 3 at n = 15 (the setting of the expect tests' test_relabelled_state): the batch leaves the
    qubits relabelled and the call restores the caller's order first — seen as one permutation sweep in the profile"""
    n = 15
    ops = circuits.c2_random_circuit(n, 80, seed=41)
    x = _state(n, dtype)
    terms = [P.term_of_masks(n, cx, cz) for cx, cz in ((0, 0x4001), (1, 0x11), (1, 0x7000), (1 << (n - 1), 0x7001), (0x4102, 0x4106), (0, 0))]
    angles = [0.7, -1.9, 0.3, 4.0, -2.5, 1.1]
    with q.HipState(n, dtype) as st, q.HipState(n, dtype) as twin:
        st.set_option("tile", 1)
        st.set_option("tile_relabel", 3)
        st.set_option("profile", 1)
        st.upload(x)
        st.apply_ops(ops)
        twin.copy_from(st)  # (settles: a copy in the caller's order)
        y = twin.download()
        st.upload(x)
        st.apply_ops(ops)
        st.profile_reset()
        st.apply_pauli_rotations(terms, angles)
        assert st.profile().get("k_permute_bits", {}).get("launches", 0) >= 1, "the batch left no layout to restore"
        got = st.download()
        twin.apply_pauli_rotations(terms, angles)
        assert st.max_abs_diff(twin) == (0.0, 0)
    _hold_sequence(len(terms), got, P.rotate_many_ref(n, terms, angles, y), y, f"n={n} relabelled")


# ---- 9: stream order --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", P.DTYPES, ids=_IDS)
def test_queued_between_batches_without_a_synchronise(dtype):
    n = 12
    layer = circuits.h_layer(n)
    terms = ["ZIIIIIIIIIIZ", "XIIIIIIIIIIX", "IYIIIIZIIIXI", "IIIIIIIIIIII", "IIXIIIIIYIIZ"]
    angles = [0.7, -1.9, 4.0, 0.3, -2.5]
    with q.HipState(n, dtype) as st, q.HipState(n, dtype) as twin:
        st.init_basis(5)
        st.apply_ops(layer)
        st.apply_pauli_rotations(terms, angles)  # no synchronise in between
        st.apply_ops(layer)
        got = st.download()
        twin.init_basis(5)
        twin.apply_ops(layer)
        y = twin.download()  # (a download waits for the stream)
        twin.apply_pauli_rotations(terms, angles)
        mid = twin.download()
        twin.apply_ops(layer)
        want = twin.download()
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    _hold_sequence(len(terms), mid, P.rotate_many_ref(n, [P.term_of_string(s) for s in terms], angles, y), y, "after one layer")


# ---- 10: refusals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", P.DTYPES, ids=_IDS)
def test_refusals(dtype):
    n = 5
    x = _state(n, dtype)
    call = _ffi.lib.qipx_state_apply_pauli_rotations
    u64, u8, dbl = lambda v: (C.c_uint64 * len(v))(*v), lambda v: (C.c_uint8 * len(v))(*v), lambda v: (C.c_double * len(v))(*v)
    good = (u64([0, 2, 3]), u64([0, 3, 1]), u8([1, 3, 2]), dbl([0.4, -1.2]))
    with q.HipState(n, dtype) as st:
        st.upload(x)

        def refused(rc):
            assert rc == _ffi.QIP_ERR_INVALID and _ffi.last_error()
            assert np.array_equal(st.download().view(np.uint8), x.view(np.uint8))

        for null in range(4):
            args = list(good)
            args[null] = None
            refused(call(st._h, *args, 2))
        for bad in (float("nan"), float("inf"), -float("inf")):
            refused(call(st._h, good[0], good[1], good[2], dbl([0.4, bad]), 2))  # in the last term of the batch
            assert "term 1" in _ffi.last_error()
        refused(call(st._h, good[0], u64([3, 3, 1]), good[2], good[3], 2))            # repeated inside a term
        refused(call(st._h, good[0], good[1], u8([1, 4, 2]), good[3], 2))             # code 4
        refused(call(st._h, good[0], u64([0, n, 1]), good[2], good[3], 2))            # qubit = n
        refused(call(st._h, u64([0, 2, 1]), good[1], good[2], good[3], 2))            # decreasing
        refused(call(st._h, u64([1, 2, 3]), good[1], good[2], good[3], 2))            # term_start[0] != 0
        for bad in ([{n: "X"}], ["XX"], [{0: "W"}]):
            with pytest.raises(q.CircuitError):
                st.apply_pauli_rotations(bad, [0.1])
        with pytest.raises(q.CircuitError):
            st.apply_pauli_rotations(["ZIIII", "XIIII"], [1.0])
        for value in (0, -1, 33):
            with pytest.raises(q.CircuitError):
                st.set_option("rotate_group", value)
        assert call(st._h, None, None, None, None, 0) == _ffi.QIP_OK  # no terms: nothing to do, null arrays allowed
        st.apply_pauli_rotations([], [])
        assert np.array_equal(st.download().view(np.uint8), x.view(np.uint8))
        # and it still rotates
        assert call(st._h, *good, 2) == _ffi.QIP_OK
        got = st.download()
    terms = [{0: "X", 3: "Z"}, {1: "Y"}]
    _hold_sequence(2, got, P.rotate_many_ref(n, terms, [0.4, -1.2], x), x, "after the refusals")


# ---- 11, 12: the mirrors ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", P.DTYPES, ids=_IDS)
def test_evolve_is_repeated_rotations(dtype):
    n = 10
    x = _state(n, dtype)
    rng = np.random.default_rng(12)
    strings = ["".join(rng.choice(list("IXYZ"), n)) for _ in range(12)] + ["I" * n]
    coeffs = rng.standard_normal(len(strings))
    dt = 0.05
    with q.HipState(n, dtype) as st:
        st.upload(x)
        st.evolve(strings, coeffs, dt, steps=3)
        got = st.download()
        st.upload(x)
        for _ in range(3):
            st.apply_pauli_rotations(strings, coeffs * dt)
        want = st.download()
        with pytest.raises(q.CircuitError):
            st.evolve(strings, coeffs[:-1], dt)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    terms = [P.term_of_string(s) for s in strings] * 3
    _hold_sequence(len(terms), got, P.rotate_many_ref(n, terms, list(coeffs * dt) * 3, x), x, "evolve")


def test_cpp_mirror(tmp_path):
    n = 10
    x = _state(n, np.complex128)
    rng = np.random.default_rng(13)
    strings = ["".join(rng.choice(list("IXYZ"), n)) for _ in range(10)] + ["I" * n, "Z" * n, "Y" * n]
    angles = rng.uniform(-3.0, 3.0, len(strings))
    exe = str(tmp_path / "test_rotate_mirror")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "rustqip_amd", "host"), os.path.join(ROOT, "tests", "cpp", "test_rotate_mirror.cpp"),
                    "-o", exe, "-L" + os.path.join(ROOT, "rustqip_amd", "lib"), "-lqip_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "rustqip_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib",
                    "-Wl,-rpath-link,/opt/rocm/lib"], check=True, capture_output=True)
    x.tofile(tmp_path / "state.bin")
    args = [a for s, theta in zip(strings, angles) for a in (s, float(theta).hex())]
    res = subprocess.run([exe, str(n), str(tmp_path / "state.bin"), str(tmp_path / "out.bin")] + args, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    with q.HipState(n) as st:
        want = _rotated(st, x, strings, angles)
    got = np.fromfile(tmp_path / "out.bin", dtype=np.complex128)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
