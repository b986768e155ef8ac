"""Reduced density matrices of up to six qubits of a device state (qipx_state_reduced_density, include/qip_hipx.h) and the
Python calls built on it: HipState.reduced_density_matrix, purity, entanglement_entropy, mutual_information.

The reference and the bar are those of tests/reduced_density_ref.py: every entry within 1e-12 sqrt(ref[a][a] ref[a'][a']) of
the sum of complex128 products added in longdouble, for Complex<f64> and Complex<f32> states alike.  Every test prints its worst
ratio to the bar before it asserts.

Which size runs which regime of the kernels as built (positions in units of 16-byte elements: a packed Complex<f32> element is
two amplitudes, so its positions are one less and amplitude position 0 is the half of the element):

  k = 1 .. 3, k_density_small.  Positions < 6 are lane bits (the wave transposes rows by shuffles), positions >= 6 are walked
  by the lane.  A wave takes rows of 64 elements, 2^(lane bits) (at least four loads) at a time.
    n = 1, 2, 3      fewer elements than one row: idle lanes hold zeros; k = n is one column
    n = k .. k + 3   the same, up to 64 elements
    n = 9            8 rows (f32: 4): one block, waves with one round or none
    n = 13           128 rows: one to eight blocks, every mix of lane bits and walked bits (position 8 is walked; 5 / 6 is the
                     boundary for f64, 6 / 7 for packed f32)
    n = 20           2^14 rows: 512 to 4096 blocks, several rounds per wave, the block fold (k_sum_partials)

  k = 4 .. 6, k_density_mfma.  A tile is (the values of the positions >= L) x (a run of 2^L elements) with the largest L that
  keeps it within 2^11 elements; a block fetches its next tile while it works on this one; at k = 6 two pairs of waves own half
  of the 16 x 16 block pairs each.
    n = k .. k + 3   one tile of 1 .. 8 columns: fewer than the four of one matrix step (zero padding), one or two steps
    n = 9            one tile: the whole state (f32: half a tile's capacity); bit 0 a row bit or a column bit of packed f32
    n = 13           f64: four tiles = four blocks, f32: two; L = 5 .. 11 by position set, every LDS swizzle from none (the low
                     bits) to four folded row bits (the top bits)
    n = 20           512 tiles (f32: 256), one per block, and the block fold
    n = 23, k = 4    top bits: 4096 tiles (f32: 2048) on 1024 blocks: the only case here with several tiles per block (the tile
                     fetched ahead is used) and with 32 steps per wave, after which a wave adds its accumulators to the second
                     set and clears them inside the loop"""
import ctypes as C
import subprocess

from gpu_common import *  # noqa: F401,F403

import reduced_density_ref as D
from rustqip_amd import _ffi

pytestmark = pytest.mark.gpu

_IDS = ("c128", "c64")
_STATES = {}


def _state(n, dtype, norm=1.0):
    """the case state of (n, dtype, norm): shared, never written to"""
    key = (n, np.dtype(dtype), norm)
    if key not in _STATES:
        x = D.make_state(n, D.seed_of(n, dtype), dtype, norm=norm)
        x.setflags(write=False)
        _STATES[key] = x
    return _STATES[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _hold(n, indices, got, x, what):
    ref = D.density_ref(n, indices, x)
    worst = D.worst_ratio(got, ref)
    print(f"{what}: qubits {list(indices)}: worst |got - ref| / bar = {worst:.3e}")
    assert got.dtype == np.complex128 and got.shape == ref.shape
    assert worst <= 1.0, (what, indices)
    assert D.exact_structure(got), (what, indices)
    return ref


def _run_sets(n, dtype, sets, what):
    """every index set of `sets` (qubits) on the case state of (n, dtype), in one handle; the state stays bit-equal"""
    x = _state(n, dtype)
    with q.HipState(n, dtype) as st:
        st.upload(x)
        for indices in sets:
            _hold(n, indices, st.reduced_density_matrix(indices), x, f"{what} n={n}")
        assert np.array_equal(_bits(st.download()), _bits(x))


# ---- 1: tiny states ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", D.DTYPES, ids=_IDS)
def test_tiny_states_every_ordered_subset(dtype):
    for n in (1, 2, 3):
        _run_sets(n, dtype, list(D.ordered_subsets(n)), "tiny")


# ---- 2: few columns ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", D.DTYPES, ids=_IDS)
@pytest.mark.parametrize("k", range(1, 7))
def test_few_columns(k, dtype):
    """n = k .. k + 3: 1, 2, 4 and 8 columns; the low bits, the top bits, and a scrambled scattered set"""
    for n in range(k, k + 4):
        _run_sets(n, dtype, [D.qubits(n, s) for s in D.few_column_sets(n, k)], "few columns")


# ---- 3: one block ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", D.DTYPES, ids=_IDS)
@pytest.mark.parametrize("k", range(1, 7))
@pytest.mark.parametrize("n", (9, 13))
def test_one_block(n, k, dtype):
    sets = []
    for s in D.position_sets(n, k):
        sets.append(D.qubits(n, s))
        if k >= 2:
            sets.append(D.qubits(n, D.scrambled(s, 100 * n + k)))
    _run_sets(n, dtype, sets, "one block")


# ---- 4: many blocks and the partial fold --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", D.DTYPES, ids=_IDS)
@pytest.mark.parametrize("k", (1, 3, 4, 6))
def test_many_blocks(k, dtype):
    """n = 20: every call runs hundreds of blocks and k_sum_partials folds them"""
    n = 20
    sets = [list(range(k)), list(range(n - k, n)), D.scrambled(sorted([0, n - 1, 4, 9, 13, 6][:k]), k)]
    _run_sets(n, dtype, [D.qubits(n, s) for s in sets], "many blocks")


@pytest.mark.parametrize("dtype", D.DTYPES, ids=_IDS)
def test_accumulators_cleared_inside_the_loop(dtype):
    """n = 23, k = 4, the top bits: several tiles per block, and a wave passes 32 steps and adds its accumulators to the second
    set inside the loop"""
    n = 23
    _run_sets(n, dtype, [D.qubits(n, list(range(n - 4, n)))], "second accumulator set")


# ---- 5: an unnormalised state ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", D.DTYPES, ids=_IDS)
def test_unnormalised_state_is_raw(dtype):
    n, norm = 13, 0.37
    x = _state(n, dtype, norm)
    with q.HipState(n, dtype) as st:
        st.upload(x)
        for indices in ([0], [12, 3], [4, 0, 9], [1, 12, 6, 3], [11, 12, 0, 5, 7, 2]):
            ref = _hold(n, indices, st.reduced_density_matrix(indices), x, f"norm^2 = {norm}")
            assert abs(np.trace(ref).real - norm) <= 1e-6 * norm  # (f32 rounding of the state itself)


# ---- 6: exact properties ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", D.DTYPES, ids=_IDS)
def test_exact_properties(dtype):
    """conjugate lower triangle and +0.0 diagonal (held by every _hold above too); two calls give equal bits; a permuted index list
    gives the bit-exact permutation; the state is bit-equal afterwards"""
    n = 13
    x = _state(n, dtype)
    rng = np.random.default_rng(6)
    with q.HipState(n, dtype) as st:
        st.upload(x)
        for k in range(1, 7):
            for s in D.position_sets(n, k):
                indices = D.qubits(n, s)  # ascending positions
                first, again = st.reduced_density_matrix(indices), st.reduced_density_matrix(indices)
                assert D.exact_structure(first)
                assert np.array_equal(_bits(first), _bits(again)), indices
                perm = [int(v) for v in rng.permutation(k)]
                other = st.reduced_density_matrix([indices[p] for p in perm])
                assert np.array_equal(_bits(other), _bits(D.permuted(first, perm))), (indices, perm)
        assert np.array_equal(_bits(st.download()), _bits(x))


# ---- 7: cross-checks against the other device calls ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", D.DTYPES, ids=_IDS)
def test_cross_checks(dtype):
    """diag rho against measure_probs (Complex<f64>: within the bar; Complex<f32>: measure_probs forms its products in f32, so
    the bar there is the f32 rounding of the products, 2^-22 of the entry), tr rho against norm_sqr, tr(rho P) for the 16
    two-qubit strings against expect_pauli within 1e-12 ||psi||^2"""
    n = 13
    x = _state(n, dtype, 0.81)
    paulis = {"I": np.eye(2), "X": np.array([[0, 1], [1, 0]]), "Y": np.array([[0, -1j], [1j, 0]]), "Z": np.diag([1.0, -1.0])}
    with q.HipState(n, dtype) as st:
        st.upload(x)
        norm2 = st.norm_sqr()
        for indices in ([12], [0, 12], [5, 3, 9], [2, 11, 12, 7], [0, 1, 2, 3, 4], [12, 10, 8, 6, 4, 2]):
            rho = st.reduced_density_matrix(indices)
            probs = st.measure_probs(indices)
            diag = np.diag(rho).real
            bar = 1e-12 * diag if dtype == np.complex128 else 2.0 ** -22 * diag
            worst = float(np.max(np.abs(diag - probs) / np.where(bar > 0, bar, 1.0)))
            print(f"qubits {indices}: diag against measure_probs, worst / bar = {worst:.3e}; trace - norm_sqr = {np.trace(rho).real - norm2:.3e}")
            assert np.all(np.abs(diag - probs) <= bar)
            assert abs(np.trace(rho).real - norm2) <= (1e-12 if dtype == np.complex128 else 2.0 ** -22) * norm2
        for pair in ([3, 8], [12, 0], [11, 12]):
            rho = st.reduced_density_matrix(pair)
            terms = [{pair[0]: a, pair[1]: b} for a in "IXYZ" for b in "IXYZ"]
            want = st.expect_pauli(terms)
            # bit 0 of the row index is qubit pair[0]: rho acts on (qubit pair[1]) (x) (qubit pair[0])
            got = np.array([np.trace(rho @ np.kron(paulis[t[pair[1]]], paulis[t[pair[0]]])) for t in terms])
            worst = float(np.max(np.abs(got - want)))
            print(f"qubits {pair}: tr(rho P) against expect_pauli, worst {worst:.3e}, bar {1e-12 * norm2:.3e}")
            assert worst <= 1e-12 * norm2


# ---- 8: known entanglement ---------------------------------------------------------------------------------------------------------
def _h(qb):
    return q.make_matrix_op([qb], circuits.H)


def _cnot(c, t):
    return q.make_control_op([c], q.make_matrix_op([t], circuits.X))


@pytest.mark.parametrize("dtype", D.DTYPES, ids=_IDS)
def test_bell_pair_and_mutual_information(dtype):
    """a Bell pair on qubits 1 and 4 of n = 6, the rest |0>: either qubit has 1 bit, the pair 0, their mutual information 2 bits;
    entries that are exactly zero in the reference are exactly zero"""
    n = 6
    tol = 1e-12  # (both amplitudes are the same rounding of 2^-1/2 in either precision: rho / tr rho is exact)
    with q.HipState(n, dtype) as st:
        st.init_basis(0)
        st.apply_ops([_h(1), _cnot(1, 4)])
        x = st.download()
        for indices in ([1], [4], [1, 4], [4, 1, 0], [0, 2], [5, 3, 2, 0], [0, 1, 2, 3, 4, 5], [1, 0, 2, 3, 5]):
            got = st.reduced_density_matrix(indices)
            ref = _hold(n, indices, got, x, "Bell")
            assert not np.any(got[ref == 0]), indices
        s1, s4, s14 = st.entanglement_entropy([1]), st.entanglement_entropy([4]), st.entanglement_entropy([1, 4])
        mi = st.mutual_information([1], [4])
        print(f"Bell: S(1) = {s1!r}, S(4) = {s4!r}, S(1,4) = {s14!r}, I = {mi!r}, purity {st.purity([1])!r}")
        assert abs(s1 - 1) <= tol and abs(s4 - 1) <= tol and abs(s14) <= tol and abs(mi - 2) <= 2 * tol
        assert abs(st.purity([1]) - 0.5) <= tol and abs(st.purity([1, 4]) - 1) <= tol
        assert abs(st.entanglement_entropy([1], base=np.e) - np.log(2)) <= tol
        assert abs(st.entanglement_entropy([0, 2, 3])) <= tol and abs(st.purity([0, 2, 3, 5]) - 1) <= tol  # a product state
        with pytest.raises(ValueError):
            st.mutual_information([1, 2], [2, 4])


@pytest.mark.parametrize("dtype", D.DTYPES, ids=_IDS)
def test_ghz(dtype):
    """GHZ at n = 10: every proper subset has entropy 1 bit and purity 1/2"""
    n = 10
    tol = 1e-12
    with q.HipState(n, dtype) as st:
        st.init_basis(0)
        st.apply_ops([_h(0)] + [_cnot(t - 1, t) for t in range(1, n)])
        x = st.download()
        for indices in ([0], [9], [3, 7], [9, 0, 4], [1, 2, 3, 4], [9, 8, 7, 6, 5], [0, 9, 2, 7, 4, 5]):
            got = st.reduced_density_matrix(indices)
            ref = _hold(n, indices, got, x, "GHZ")
            assert not np.any(got[ref == 0]), indices
            s, p = st.entanglement_entropy(indices), st.purity(indices)
            print(f"GHZ qubits {indices}: S = {s!r}, purity = {p!r}")
            assert abs(s - 1) <= tol and abs(p - 0.5) <= tol


@pytest.mark.parametrize("dtype", D.DTYPES, ids=_IDS)
def test_complement_route(dtype):
    """n = 8: seven qubits have the entropy of the one left out; more than six on both sides is the library's refusal"""
    n = 8
    x = _state(n, dtype)
    with q.HipState(n, dtype) as st:
        st.upload(x)
        for out in (0, 3, 7):
            seven = [qb for qb in range(n) if qb != out]
            a, b = st.entanglement_entropy(seven[::-1]), st.entanglement_entropy([out])
            print(f"n = 8 without qubit {out}: {a!r} against {b!r}")
            assert a == b
        assert st.entanglement_entropy(list(range(n))) == 0.0
    with q.HipState(14, dtype) as st:
        st.init_basis(0)
        with pytest.raises(q.QipHipError, match="k = 7"):
            st.entanglement_entropy(list(range(7)))


# ---- 9: a relabelled state -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", D.DTYPES, ids=_IDS)
def test_relabelled_state(dtype):
    """tile_relabel = 3 leaves a layout after apply_ops; the call puts the caller's order back first.  The reference state is the
    download of the same handle (a download restores the caller's order too, and a restored layout moves amplitudes exactly)"""
    n = 15
    ops = circuits.c2_random_circuit(n, 80, seed=41)
    x = _state(n, dtype)
    with q.HipState(n, dtype) as st:
        st.set_option("tile", 1)
        st.set_option("tile_relabel", 3)
        st.set_option("profile", 1)
        for indices in ([14, 0, 7], [0, 14, 5, 9, 2]):
            st.upload(x)
            st.apply_ops(ops)
            st.profile_reset()
            got = st.reduced_density_matrix(indices)
            assert st.profile().get("k_permute_bits", {}).get("launches", 0) >= 1, "the batch left no layout to restore"
            _hold(n, indices, got, st.download(), "relabelled")


# ---- 10: refusals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", D.DTYPES, ids=_IDS)
def test_refusals(dtype):
    n = 8
    x = _state(n, dtype)
    call = _ffi.lib.qipx_state_reduced_density
    u64 = lambda v: (C.c_uint64 * len(v))(*v)  # noqa: E731
    out = (C.c_double * (2 * 64 * 64))(*([7.0] * (2 * 64 * 64)))
    with q.HipState(n, dtype) as st:
        st.upload(x)

        def refused(rc, code=_ffi.QIP_ERR_INVALID):
            message = _ffi.last_error()
            assert rc == code and message
            assert np.array_equal(_bits(st.download()), _bits(x))
            assert all(v == 7.0 for v in out)
            return message

        assert "k = 7" in refused(call(st._h, u64(range(7)), 7, out), _ffi.QIP_ERR_UNSUPPORTED)
        refused(call(st._h, u64([1, 3, 1]), 3, out))        # repeated
        refused(call(st._h, u64([1, n]), 2, out))           # out of range
        refused(call(st._h, u64([1]), 0, out))              # k = 0
        refused(call(st._h, None, 2, out))                  # no index list
        refused(call(st._h, u64([1, 2]), 2, None))          # no output
        refused(call(None, u64([1, 2]), 2, out))            # no handle
        with pytest.raises(q.QipHipError, match="k = 7"):
            st.reduced_density_matrix(list(range(7)))
        for bad in ([1, 1], [n], []):
            with pytest.raises(q.CircuitError):
                st.reduced_density_matrix(bad)
        # and it still works
        _hold(n, [2, 6, 0, 7], st.reduced_density_matrix([2, 6, 0, 7]), x, "after the refusals")


# ---- 11: the C++ mirror ------------------------------------------------------------------------------------------------------------
def test_cpp_mirror(tmp_path):
    n = 10
    x = _state(n, np.complex128)
    exe = str(tmp_path / "test_density_mirror")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "rustqip_amd", "host"), os.path.join(ROOT, "tests", "cpp", "test_density_mirror.cpp"),
                    "-o", exe, "-L" + os.path.join(ROOT, "rustqip_amd", "lib"), "-lqip_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "rustqip_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib",
                    "-Wl,-rpath-link,/opt/rocm/lib"], check=True, capture_output=True)
    x.tofile(tmp_path / "x.bin")
    two, five = [7, 2], [9, 0, 4, 5, 1]
    res = subprocess.run([exe, str(n), str(tmp_path / "x.bin"), str(tmp_path / "out.bin"), ",".join(map(str, two)), ",".join(map(str, five))],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    with q.HipState(n) as st:
        st.upload(x)
        want = np.concatenate([st.reduced_density_matrix(two).ravel(), st.reduced_density_matrix(five).ravel()])
    got = np.fromfile(tmp_path / "out.bin", dtype=np.complex128)
    assert np.array_equal(_bits(got), _bits(want))
