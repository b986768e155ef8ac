"""Reduced transition matrices of up to three qubits of two device states (qipx_state_transition_matrix, include/qip_hipx.h)
and HipState.transition_matrix.

The reference and the bar are those of tests/transition_ref.py: every entry within 1e-12 sqrt(rho_ket[a][a] rho_bra[a'][a']) of
the sum of complex128 products added in longdouble, for both precisions, on two different seeded states.  Every test prints
its worst ratio to the bar before it asserts.

The regimes of k_transition_small are those of k_density_small (tests/test_gpu_f2_reduced_density.py: positions < 6, in 16-byte
elements, are lane bits transposed by shuffles, positions >= 6 are walked; a packed Complex<f32> element is two amplitudes and
amplitude position 0 is its half), one row set of 2^(lane bits) rows per round:
    n = 1, 2, 3      fewer elements than one row: idle lanes hold zeros; k = n is one column
    n = k .. k + 3   the same, up to 64 elements
    n = 9            8 rows (f32: 4): one block
    n = 13           128 rows: every mix of lane bits and walked bits (position 8 is walked; 5 / 6 is the boundary for f64,
                     6 / 7 for packed f32)
    n = 20           2^14 rows: thousands of blocks, several rounds per wave, the block fold (k_sum_partials)
The k = 3 form (the entries split over pairs of lanes) has no size regime of its own: the pairing bit is the lowest lane bit
that is no position, whatever n is, so every k = 3 case above runs it — with the lowest three lane bits taken (the low set),
with none taken (the top set), and on tiny states where the partner lane is an idle one."""
import ctypes as C
import subprocess

from gpu_common import *  # noqa: F401,F403

import transition_ref as T
from rustqip_amd import _ffi

pytestmark = pytest.mark.gpu

_IDS = ("c128", "c64")
_STATES = {}


def _pair(n, dtype, norms=(1.0, 1.0)):
    """(bra, ket) of the case: two different seeded states, shared, never written to"""
    key = (n, np.dtype(dtype), norms)
    if key not in _STATES:
        bra = T.make_state(n, T.seed_of(n, dtype) + 500, dtype, zero_every=7, norm=norms[0])
        ket = T.make_state(n, T.seed_of(n, dtype), dtype, norm=norms[1])
        bra.setflags(write=False)
        ket.setflags(write=False)
        _STATES[key] = (bra, ket)
    return _STATES[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _hold(n, indices, got, bra, ket, what):
    ref = T.transition_ref(n, indices, bra, ket)
    bar = T.bars(T.row_weights(n, indices, ket), T.row_weights(n, indices, bra))
    worst = T.worst_ratio(got, ref, bar)
    print(f"{what}: qubits {list(indices)}: worst |got - ref| / bar = {worst:.3e}")
    assert got.dtype == np.complex128 and got.shape == ref.shape
    assert worst <= 1.0, (what, indices)
    return ref


def _run_sets(n, dtype, sets, what):
    """every index set of `sets` (qubits) on the case pair of (n, dtype), in one pair of handles; the states stay bit-equal"""
    bra, ket = _pair(n, dtype)
    with q.HipState(n, dtype) as hb, q.HipState(n, dtype) as hk:
        hb.upload(bra)
        hk.upload(ket)
        for indices in sets:
            _hold(n, indices, hb.transition_matrix(hk, indices), bra, ket, f"{what} n={n}")
        assert np.array_equal(_bits(hb.download()), _bits(bra)) and np.array_equal(_bits(hk.download()), _bits(ket))


@pytest.mark.parametrize("dtype", T.DTYPES, ids=_IDS)
def test_tiny_states_every_ordered_subset(dtype):
    for n in (1, 2, 3):
        _run_sets(n, dtype, list(T.ordered_subsets(n)), "tiny")


@pytest.mark.parametrize("dtype", T.DTYPES, ids=_IDS)
@pytest.mark.parametrize("k", (1, 2, 3))
def test_few_columns(k, dtype):
    for n in range(k, k + 4):
        _run_sets(n, dtype, [T.qubits(n, s) for s in T.few_column_sets(n, k)], "few columns")


@pytest.mark.parametrize("dtype", T.DTYPES, ids=_IDS)
@pytest.mark.parametrize("k", (1, 2, 3))
@pytest.mark.parametrize("n", (9, 13))
def test_one_block(n, k, dtype):
    sets = []
    for s in T.position_sets(n, k):
        sets.append(T.qubits(n, s))
        if k >= 2:
            sets.append(T.qubits(n, T.scrambled(s, 100 * n + k)))
    _run_sets(n, dtype, sets, "one block")


@pytest.mark.parametrize("dtype", T.DTYPES, ids=_IDS)
@pytest.mark.parametrize("k", (1, 2, 3))
def test_many_blocks(k, dtype):
    """n = 20: thousands of blocks, and k_sum_partials folds them"""
    n = 20
    sets = [list(range(k)), list(range(n - k, n)), T.scrambled(sorted([0, n - 1, 9][:k]), k)]
    _run_sets(n, dtype, [T.qubits(n, s) for s in sets], "many blocks")


@pytest.mark.parametrize("dtype", T.DTYPES, ids=_IDS)
def test_exact_properties(dtype):
    """two calls give equal bits; a permuted index list gives the bit-exact permutation; a zero bra gives an all-zero matrix;
    both states are bit-equal afterwards"""
    n = 13
    bra, ket = _pair(n, dtype)
    rng = np.random.default_rng(6)
    with q.HipState(n, dtype) as hb, q.HipState(n, dtype) as hk, q.HipState(n, dtype) as hz:
        hb.upload(bra)
        hk.upload(ket)
        hz.upload(np.zeros(1 << n, dtype=dtype))
        for k in (1, 2, 3):
            for s in T.position_sets(n, k):
                indices = T.qubits(n, s)
                first, again = hb.transition_matrix(hk, indices), hb.transition_matrix(hk, indices)
                assert np.array_equal(_bits(first), _bits(again)), indices
                perm = [int(v) for v in rng.permutation(k)]
                other = hb.transition_matrix(hk, [indices[p] for p in perm])
                assert np.array_equal(_bits(other), _bits(T.permuted(first, perm))), (indices, perm)
                assert not np.any(hz.transition_matrix(hk, indices)), indices
        assert np.array_equal(_bits(hb.download()), _bits(bra)) and np.array_equal(_bits(hk.download()), _bits(ket))


def _h(qb):
    return q.make_matrix_op([qb], circuits.H)


def _cnot(c, t):
    return q.make_control_op([c], q.make_matrix_op([t], circuits.X))


@pytest.mark.parametrize("dtype", T.DTYPES, ids=_IDS)
def test_exact_zeros_of_bell_and_ghz(dtype):
    """bra: GHZ on all qubits, ket: a Bell pair on qubits 1 and 4 with the rest |0>: entries that are exactly zero in the
    reference are exactly zero"""
    n = 13
    with q.HipState(n, dtype) as hb, q.HipState(n, dtype) as hk:
        hb.init_basis(0)
        hb.apply_ops([_h(0)] + [_cnot(t - 1, t) for t in range(1, n)])
        hk.init_basis(0)
        hk.apply_ops([_h(1), _cnot(1, 4)])
        bra, ket = hb.download(), hk.download()
        for indices in ([1], [4, 1], [1, 4, 0], [12, 0, 6], [12], [5, 7], [10, 11, 12]):
            got = hb.transition_matrix(hk, indices)
            ref = _hold(n, indices, got, bra, ket, "Bell / GHZ")
            assert np.any(ref == 0) and not np.any(got[ref == 0]), indices


@pytest.mark.parametrize("dtype", T.DTYPES, ids=_IDS)
def test_cross_checks(dtype):
    """an unnormalised pair: bra is ket against reduced_density_matrix within two bars, tr M against inner, trace(P M) for the 16
    two-qubit strings against pauli_matrix_elements within 1e-12 ||bra|| ||ket||"""
    n = 13
    bra, ket = _pair(n, dtype, (0.81, 2.3))
    paulis = {"I": np.eye(2), "X": np.array([[0, 1], [1, 0]]), "Y": np.array([[0, -1j], [1j, 0]]), "Z": np.diag([1.0, -1.0])}
    scale = 1e-12 * np.sqrt(0.81 * 2.3) * (1 + 1e-6)  # (the f32 rounding of the states themselves)
    with q.HipState(n, dtype) as hb, q.HipState(n, dtype) as hk:
        hb.upload(bra)
        hk.upload(ket)
        for indices in ([12], [0, 12], [5, 3, 9], [0, 1, 2]):
            same, rho = hk.transition_matrix(hk, indices), hk.reduced_density_matrix(indices)
            w = T.row_weights(n, indices, ket)
            worst = T.worst_ratio(same, rho, 2 * T.bars(w, w))
            print(f"qubits {indices}: bra is ket against reduced_density_matrix, worst / (2 bars) = {worst:.3e}")
            assert worst <= 1.0
            m = hb.transition_matrix(hk, indices)
            inner = hb.inner(hk)
            print(f"qubits {indices}: |tr M - inner| = {abs(np.trace(m) - inner):.3e}, bar {2 * scale:.3e}")
            assert abs(np.trace(m) - inner) <= 2 * scale
        for pair in ([3, 8], [12, 0], [11, 12]):
            m = hb.transition_matrix(hk, pair)
            terms = [{pair[0]: a, pair[1]: b} for a in "IXYZ" for b in "IXYZ"]
            want = hb.pauli_matrix_elements(hk, terms)
            # bit 0 of the row index is qubit pair[0]: M acts on (qubit pair[1]) (x) (qubit pair[0])
            got = np.array([np.trace(np.kron(paulis[t[pair[1]]], paulis[t[pair[0]]]) @ m) for t in terms])
            worst = float(np.max(np.abs(got - want)))
            print(f"qubits {pair}: trace(P M) against pauli_matrix_elements, worst {worst:.3e}, bar {scale:.3e}")
            assert worst <= scale


@pytest.mark.parametrize("dtype", T.DTYPES, ids=_IDS)
def test_relabelled_states(dtype):
    """tile_relabel = 3 leaves a layout after apply_ops on BOTH handles; the call puts the caller's order back first.  The
    reference states are the downloads of the same handles"""
    n = 15
    bra, ket = _pair(n, dtype)
    with q.HipState(n, dtype) as hb, q.HipState(n, dtype) as hk:
        for st, x, seed in ((hb, bra, 43), (hk, ket, 41)):
            st.set_option("tile", 1)
            st.set_option("tile_relabel", 3)
            st.set_option("profile", 1)
        for indices in ([14, 0, 7], [9, 2], [0]):
            for st, x, seed in ((hb, bra, 43), (hk, ket, 41)):
                st.upload(x)
                st.apply_ops(circuits.c2_random_circuit(n, 80, seed=seed))
                st.profile_reset()
            got = hb.transition_matrix(hk, indices)
            for st in (hb, hk):
                assert st.profile().get("k_permute_bits", {}).get("launches", 0) >= 1, "the batch left no layout to restore"
            _hold(n, indices, got, hb.download(), hk.download(), "relabelled")


@pytest.mark.parametrize("dtype", T.DTYPES, ids=_IDS)
def test_ordering_after_queued_work(dtype):
    """work queued on either handle (apply_ops returns without waiting) is seen by the call"""
    n = 20
    bra, ket = _pair(n, dtype)
    ops = [_h(qb) for qb in range(n)] + [_cnot(qb, (qb + 7) % n) for qb in range(n)]
    with q.HipState(n, dtype) as hb, q.HipState(n, dtype) as hk:
        hb.upload(bra)
        hk.upload(ket)
        hb.apply_ops(ops)
        hk.apply_ops(ops[::-1])
        got = hb.transition_matrix(hk, [3, 19, 11])
        _hold(n, [3, 19, 11], got, hb.download(), hk.download(), "queued work")


@pytest.mark.parametrize("dtype", T.DTYPES, ids=_IDS)
def test_refusals(dtype):
    n = 8
    bra, ket = _pair(n, dtype)
    other = np.complex64 if dtype == np.complex128 else np.complex128
    call = _ffi.lib.qipx_state_transition_matrix
    u64 = lambda v: (C.c_uint64 * len(v))(*v)  # noqa: E731
    out = (C.c_double * (2 * 16 * 16))(*([7.0] * (2 * 16 * 16)))
    with q.HipState(n, dtype) as hb, q.HipState(n, dtype) as hk, q.HipState(n + 1, dtype) as wide, q.HipState(n, other) as prec:
        hb.upload(bra)
        hk.upload(ket)

        def refused(rc, code=_ffi.QIP_ERR_INVALID):
            message = _ffi.last_error()
            assert rc == code and message
            assert np.array_equal(_bits(hb.download()), _bits(bra)) and np.array_equal(_bits(hk.download()), _bits(ket))
            assert all(v == 7.0 for v in out)
            return message

        assert "k = 4" in refused(call(hb._h, hk._h, u64(range(4)), 4, out), _ffi.QIP_ERR_UNSUPPORTED)
        refused(call(hb._h, hk._h, u64([1, 3, 1]), 3, out))     # repeated
        refused(call(hb._h, hk._h, u64([1, n]), 2, out))        # out of range
        refused(call(hb._h, hk._h, u64([1]), 0, out))           # k = 0
        refused(call(hb._h, hk._h, None, 2, out))               # no index list
        refused(call(hb._h, hk._h, u64([1, 2]), 2, None))       # no output
        refused(call(None, hk._h, u64([1, 2]), 2, out))         # no bra
        refused(call(hb._h, None, u64([1, 2]), 2, out))         # no ket
        refused(call(wide._h, hk._h, u64([1, 2]), 2, out))      # another n
        refused(call(hb._h, prec._h, u64([1, 2]), 2, out))      # another precision
        with pytest.raises(q.QipHipError, match="k = 4"):
            hb.transition_matrix(hk, [0, 1, 2, 3])
        for bad in ([1, 1], [n], [], [-1]):
            with pytest.raises(q.CircuitError):
                hb.transition_matrix(hk, bad)
        for partner in (wide, prec, None):
            with pytest.raises(q.CircuitError):
                hb.transition_matrix(partner, [0])
        _hold(n, [2, 6, 0], hb.transition_matrix(hk, [2, 6, 0]), bra, ket, "after the refusals")


def test_cpp_mirror(tmp_path):
    n = 10
    bra, ket = _pair(n, np.complex128)
    exe = str(tmp_path / "test_transition_mirror")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "rustqip_amd", "host"), os.path.join(ROOT, "tests", "cpp", "test_transition_mirror.cpp"),
                    "-o", exe, "-L" + os.path.join(ROOT, "rustqip_amd", "lib"), "-lqip_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "rustqip_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib",
                    "-Wl,-rpath-link,/opt/rocm/lib"], check=True, capture_output=True)
    bra.tofile(tmp_path / "bra.bin")
    ket.tofile(tmp_path / "ket.bin")
    two, three = [7, 2], [9, 0, 4]
    res = subprocess.run([exe, str(n), str(tmp_path / "bra.bin"), str(tmp_path / "ket.bin"), str(tmp_path / "out.bin"),
                          ",".join(map(str, two)), ",".join(map(str, three))], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    with q.HipState(n) as hb, q.HipState(n) as hk:
        hb.upload(bra)
        hk.upload(ket)
        want = np.concatenate([hb.transition_matrix(hk, two).ravel(), hb.transition_matrix(hk, three).ravel()])
    got = np.fromfile(tmp_path / "out.bin", dtype=np.complex128)
    assert np.array_equal(_bits(got), _bits(want))
