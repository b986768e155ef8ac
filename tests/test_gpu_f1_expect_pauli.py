"""Expectation values of Pauli strings on a device state (include/qip_hipx.h: qipx_state_expect_pauli, HipState.expect_pauli):
k_expect_pauli's single-amplitude (x = 0) and pair passes, plain and packed Complex<f32> elements, the grouping into passes and
the scatter back into input order (rustqip_amd/csrc/qip_pauli.hip).

The bar of every comparison with the reference (tests/expect_pauli_ref.py: double products, math.fsum) is

    1e-12 * sum |psi_j|^2.

With unit roundoff 2^-53 any summation order over N pairs errs by at most (N + 4) * 2^-53 * sum |psi_j| |psi_{j^x}|, and
sum |psi_j| |psi_{j^x}| <= sum |psi_j|^2.  N <= 2^13 gives 9.1e-13: for n <= 13 the bar holds for EVERY correct implementation.
At n = 22 it holds whenever no serial accumulation chain is longer than 2^13 addends, which is so for any grid of >= 512 lanes
plus <= 4096 partial sums (here: a lane adds <= 32 products per block of >= 4096 work items, a block's 256 lanes fold in 8 steps,
the host adds <= 4096 partial sums).

The cross-checks against measure_probs and norm_sqr compare two sums of the same |psi_j|^2 only where both sides form the same
products: this call widens Complex<f32> amplitudes to double first (its contract), the measurement calls form |psi_j|^2 in the
state's own precision.  So the Complex<f32> cross-checks run on a state whose components are multiples of 2^-10 below 1:
re^2 + im^2 is then exact in f32 (an integer below 2^21 over 2^20) and both sides add the same numbers."""
import ctypes as C
import subprocess

from gpu_common import *  # noqa: F401,F403

import expect_pauli_ref as E
from rustqip_amd import _ffi

pytestmark = pytest.mark.gpu

_IDS = ("c128", "c64")
_STATES = {}
G = 16  # the default of option "expect_group"
REL = 1e-12


def _state(n, dtype, norm=1.0):
    """the case state of (n, dtype, norm) and its exact sum |psi_j|^2: shared, never written to"""
    key = (n, np.dtype(dtype), norm)
    if key not in _STATES:
        x = E.make_state(n, E.seed_of(n, dtype), dtype, norm=norm)
        x.setflags(write=False)
        _STATES[key] = (x, E.norm_sqr_ref(x))
    return _STATES[key]


def _close(got, want, scale, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    err = np.abs(got - want)
    print(f"{what}: max |got - want| = {err.max() if err.size else 0.0:.3e}, bar {REL * scale:.3e}")
    bad = np.nonzero(~(err <= REL * scale))[0]
    assert len(bad) == 0, (what, [(int(i), float(got[i]), float(want[i])) for i in bad[:5]])


# ---- against the reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", E.DTYPES, ids=_IDS)
def test_tiny_vectors(dtype):
    """fewer amplitudes than one wave: every Pauli string on n = 1 and 2, one call each, and all 64 strings on n = 3 in one call"""
    for n in (1, 2, 3):
        x, scale = _state(n, dtype, 0.8)
        terms = [E.term_of_string(s) for s in E.all_strings(n)]
        with q.HipState(n, dtype) as st:
            st.upload(x)
            if n < 3:
                got = np.array([st.expect_pauli([t])[0] for t in terms])
            else:
                got = st.expect_pauli(E.all_strings(n))  # (the string form of a term)
        _close(got, E.expect_ref_many(n, terms, x), scale, f"n={n}")


@pytest.mark.parametrize("norm", (1.0, 0.5))
@pytest.mark.parametrize("n", (9, 13))
@pytest.mark.parametrize("dtype", E.DTYPES, ids=_IDS)
def test_one_block_and_several_blocks(dtype, n, norm):
    """n = 9: the row loop of one block (Complex<f32> pairs of packed elements: half a block's lanes); n = 13: Complex<f64>
    one whole span per block — two blocks for x = 0 —, Complex<f32> rows only.  The raw quadratic form on a state of norm^2 0.5."""
    x, scale = _state(n, dtype, norm)
    assert abs(scale - norm) <= 1e-6
    cases = E.mask_cases(n)
    terms = [E.term_of_masks(n, cx, cz) for _, cx, cz in cases]
    for (name, cx, cz), t in zip(cases, terms):
        assert E.masks(n, t)[:2] == (cx, cz), name
    assert sorted({E.masks(n, t)[2] for t in terms}) == [0, 1, 2, 3, 4, 5]
    with q.HipState(n, dtype) as st:
        st.upload(x)
        got = st.expect_pauli(terms)
    _close(got, E.expect_ref_many(n, terms, x), scale, f"n={n} norm={norm}")


_N22 = 22
_TOP22 = 1 << (_N22 - 1)
MANY_BLOCK_MASKS = {  # twelve terms, four per case (the reference takes most of a case's time)
    "x_top": [(_TOP22, 0), (_TOP22, _TOP22 | 1), (_TOP22, 0x155555), (_TOP22, (1 << _N22) - 1)],
    "x_bit0": [(1, 0), (1, 1), (1, 0x2AAAAB), (1, _TOP22 | 0x801)],
    "mixed": [(0x240812, 0x041803), (0x240812, 0x240812), (0, 0x300C03), (0, 0)],  # n_Y = 2 and 5, a Z string, the empty term
}


@pytest.mark.parametrize("which", sorted(MANY_BLOCK_MASKS))
@pytest.mark.parametrize("dtype", E.DTYPES, ids=_IDS)
def test_many_blocks(dtype, which):
    """n = 22: hundreds of blocks, a whole span of four (x = 0) or two (pairs) loads per lane and row in each"""
    n = _N22
    x, scale = _state(n, dtype)
    terms = [E.term_of_masks(n, cx, cz) for cx, cz in MANY_BLOCK_MASKS[which]]
    with q.HipState(n, dtype) as st:
        st.upload(x)
        got = st.expect_pauli(terms)
    _close(got, E.expect_ref_many(n, terms, x), scale, f"n={n} {which}")


# ---- reproducibility: exact ------------------------------------------------------------------------------------------------------
def _three_mask_terms(n):
    """2 G + 3 terms over three x masks — bit 0 set (G + 1 terms: two passes), bit 0 clear (G - 2), zero (4) — shuffled"""
    rng = np.random.default_rng(77)
    xa, xb = (1 << (n - 1)) | 0x21, 0x1C2
    terms = []
    for cx, count in ((xa, G + 1), (xb, G - 2), (0, 4)):
        seen = set()
        while len(seen) < count:
            seen.add(int(rng.integers(0, 1 << n)))
        terms += [E.term_of_masks(n, cx, cz) for cz in sorted(seen)]
    assert len(terms) == 2 * G + 3
    return [terms[i] for i in rng.permutation(len(terms))]


@pytest.mark.parametrize("n", (9, 13))
@pytest.mark.parametrize("dtype", E.DTYPES, ids=_IDS)
def test_a_value_depends_on_the_state_and_its_term_only(dtype, n):
    x, scale = _state(n, dtype)
    terms = _three_mask_terms(n)
    assert q.expect_pauli_passes(n, terms) == 2 + 1 + 1 and q.expect_pauli_passes(n, terms, 1) == len(terms)
    with q.HipState(n, dtype) as st:
        st.upload(x)
        batch = st.expect_pauli(terms)
        singles = np.array([st.expect_pauli([t])[0] for t in terms])
        backwards = st.expect_pauli(terms[::-1])[::-1]
        assert np.array_equal(batch, st.expect_pauli(terms))
        by_group = {}
        for group in (1, 3, 4, 5, 32):  # (1: a pass per term; the others: every kernel capacity, and cuts inside a mask's run)
            st.set_option("expect_group", group)
            by_group[group] = st.expect_pauli(terms)
    assert np.array_equal(batch, singles)
    assert np.array_equal(batch, backwards)
    for group, got in by_group.items():
        assert np.array_equal(batch, got), group
    _close(batch, E.expect_ref_many(n, terms, x), scale, f"n={n}")
    assert len(set(batch.tolist())) == len(terms)  # (no two terms alike: a misplaced result would show)


# ---- against the measurement calls -------------------------------------------------------------------------------------------------
def _cross_state(n, dtype):
    x, _ = _state(n, dtype, 0.9)
    if dtype == np.complex64:  # components on the grid of 2^-10: |psi_j|^2 exact in f32 (see the module's docstring)
        x = (np.round(x.astype(np.complex128) * 1024.0) / 1024.0).astype(np.complex64)
        assert np.count_nonzero(x) > (1 << n) // 2
    return x, E.norm_sqr_ref(x)


@pytest.mark.parametrize("n", (9, 13))
@pytest.mark.parametrize("dtype", E.DTYPES, ids=_IDS)
def test_z_strings_are_signed_measurement_probabilities(dtype, n):
    x, scale = _cross_state(n, dtype)
    index_sets = ([0], [n - 1], [n - 1, 0], [3, n - 2, 1], [n - 1, n - 2, n - 3, 0], [1, 7, 0, 5, n - 1, 2], list(range(n - 1, -1, -1))[:8])
    with q.HipState(n, dtype) as st:
        st.upload(x)
        got = st.expect_pauli([{qb: "Z" for qb in idx} for idx in index_sets] + [{}])
        want = []
        for idx in index_sets:
            p = st.measure_probs(idx)
            m = np.arange(len(p), dtype=np.uint64)
            want.append(float(np.sum((1.0 - 2.0 * E.parity(m)) * p)))  # outcome bit i is the bit of qubit idx[i]
        want.append(st.norm_sqr())
    _close(got, want, scale, f"n={n}")


# ---- a relabelled state; the state is not changed ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", E.DTYPES, ids=_IDS)
def test_relabelled_state(dtype):
    """tile = 1 with tile_relabel = 3: n = 15 is the smallest size at which the scheduler keeps a relabelled plan for this circuit
    (a tile covers 11 index bits; tests/test_tile_plan_cpu.py); the batch leaves the qubits relabelled and the call restores the
    caller's order first — seen as one permutation sweep in the profile"""
    n = 15
    ops = circuits.c2_random_circuit(n, 80, seed=41)
    x, _ = _state(n, dtype)
    terms = [E.term_of_masks(n, cx, cz) for cx, cz in ((0, 0x4001), (1, 0x11), (1 << (n - 1), 0x7001), (0x4102, 0x4106), (0, 0))]
    with q.HipState(n, dtype) as st, q.HipState(n, dtype) as twin:
        st.set_option("tile", 1)
        st.set_option("tile_relabel", 3)
        st.set_option("profile", 1)
        st.upload(x)
        st.apply_ops(ops)
        twin.copy_from(st)  # (settles: a copy in the caller's order)
        st.upload(x)
        st.apply_ops(ops)
        st.profile_reset()
        got = st.expect_pauli(terms)
        assert st.profile().get("k_permute_bits", {}).get("launches", 0) >= 1, "the batch left no layout to restore"
        assert st.max_abs_diff(twin) == (0.0, 0)
        y = twin.download()
        again = twin.expect_pauli(terms)
    assert np.array_equal(got, again)
    _close(got, E.expect_ref_many(n, terms, y), E.norm_sqr_ref(y), f"n={n}")


@pytest.mark.parametrize("dtype", E.DTYPES, ids=_IDS)
def test_ordered_after_queued_work_and_state_unchanged(dtype):
    n = 12
    layer = circuits.h_layer(n)
    terms = ["ZIIIIIIIIIIZ", "XIIIIIIIIIIX", "IYIIIIZIIIXI", "IIIIIIIIIIII"]
    with q.HipState(n, dtype) as st, q.HipState(n, dtype) as twin:
        st.init_basis(5)
        twin.init_basis(5)
        st.apply_ops(layer)
        first = st.expect_pauli(terms)  # no synchronise in between
        st.apply_ops(layer)
        second = st.expect_pauli(terms)
        twin.apply_ops(layer)
        y1 = twin.download()
        twin.apply_ops(layer)
        y2 = twin.download()
        assert st.max_abs_diff(twin) == (0.0, 0)
    _close(first, E.expect_ref_many(n, [E.term_of_string(s) for s in terms], y1), E.norm_sqr_ref(y1), "after one layer")
    _close(second, E.expect_ref_many(n, [E.term_of_string(s) for s in terms], y2), E.norm_sqr_ref(y2), "after two layers")
    # H^n |5> is |+> or |-> per qubit, |-> where 5 has a one (qubits 9 and 11); two layers give |5> back
    assert abs(first[1] + 1.0) <= 1e-5 and abs(second[0] + 1.0) <= 1e-5 and abs(first[0]) <= 1e-5


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", E.DTYPES, ids=_IDS)
def test_refusals(dtype):
    n = 5
    x, _ = _state(n, dtype)
    call = _ffi.lib.qipx_state_expect_pauli
    u64, u8 = lambda v: (C.c_uint64 * len(v))(*v), lambda v: (C.c_uint8 * len(v))(*v)
    out = (C.c_double * 2)()
    good = (u64([0, 2, 3]), u64([0, 3, 1]), u8([1, 3, 2]))
    with q.HipState(n, dtype) as st:
        st.upload(x)

        def refused(rc):
            assert rc == _ffi.QIP_ERR_INVALID and _ffi.last_error()
            assert np.array_equal(st.download(), x)

        assert call(st._h, *good, 2, out) == _ffi.QIP_OK
        for null in range(3):
            args = list(good)
            args[null] = None
            refused(call(st._h, *args, 2, out))
        refused(call(st._h, *good, 2, None))
        refused(call(st._h, u64([1, 2, 3]), good[1], good[2], 2, out))            # term_start[0] != 0
        refused(call(st._h, u64([0, 2, 1]), good[1], good[2], 2, out))            # decreasing
        refused(call(st._h, good[0], u64([0, n, 1]), good[2], 2, out))            # qubit = n
        refused(call(st._h, good[0], u64([3, 3, 1]), good[2], 2, out))            # repeated inside a term
        refused(call(st._h, good[0], good[1], u8([1, 4, 2]), 2, out))             # code 4
        for bad in ([{n: "X"}], ["XX"], [{0: "W"}]):
            with pytest.raises(q.CircuitError):
                st.expect_pauli(bad)
        for value in (0, -1, 33):
            with pytest.raises(q.CircuitError):
                st.set_option("expect_group", value)
        with pytest.raises(q.CircuitError):
            st.expectation(["ZIIII", "XIIII"], [1.0])
        assert call(st._h, None, None, None, 0, None) == _ffi.QIP_OK  # no terms: nothing to do, null arrays allowed
        assert st.expect_pauli([]).shape == (0,)
        assert np.array_equal(st.download(), x)
        # and it still computes
        got = st.expect_pauli([{0: "X", 3: "Z"}, {1: "Y"}])
        assert [out[0], out[1]] == got.tolist()


# ---- the mirrors ------------------------------------------------------------------------------------------------------------------
def test_expectation_is_the_dot_product():
    n = 10
    x, scale = _state(n, np.complex128)
    rng = np.random.default_rng(10)
    strings = ["".join(rng.choice(list("IXYZ"), n)) for _ in range(40)] + ["I" * n]
    coeffs = rng.standard_normal(len(strings))
    with q.HipState(n) as st:
        st.upload(x)
        values = st.expect_pauli(strings)
        h = st.expectation(strings, coeffs)
        assert st.expectation([], []) == 0.0
    assert h == float(np.dot(coeffs, values))
    want = E.expect_ref_many(n, [E.term_of_string(s) for s in strings], x)
    _close(values, want, scale, "expect_pauli of strings")
    assert abs(h - float(np.dot(coeffs, want))) <= REL * scale * float(np.sum(np.abs(coeffs)))
    assert q.ext_abi_version() == 1


def test_cpp_mirror(tmp_path):
    n = 10
    x, _ = _state(n, np.complex128)
    rng = np.random.default_rng(11)
    strings = ["".join(rng.choice(list("IXYZ"), n)) for _ in range(20)] + ["I" * n, "Z" * n, "Y" * n]
    exe = str(tmp_path / "test_expect_mirror")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "rustqip_amd", "host"), os.path.join(ROOT, "tests", "cpp", "test_expect_mirror.cpp"),
                    "-o", exe, "-L" + os.path.join(ROOT, "rustqip_amd", "lib"), "-lqip_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "rustqip_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib",
                    "-Wl,-rpath-link,/opt/rocm/lib"], check=True, capture_output=True)
    x.tofile(tmp_path / "state.bin")
    res = subprocess.run([exe, str(n), str(tmp_path / "state.bin")] + strings, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    with q.HipState(n) as st:
        st.upload(x)
        want = st.expect_pauli(strings)
    assert [float.fromhex(v) for v in res.stdout.split()] == want.tolist()
