"""Many samples of a device state in one call (include/qip_hipx.h: qipx_state_soft_measure_many, HipState.soft_measure_many):
k_walk_chunks, the grouping by candidate chunk, k_resolve_many and the rounds (rustqip_amd/csrc/qip_measure.hip).

  (A) identity   element j of the batch is what the single call returns for sample j — exact, nothing left out, both precisions
  (B) reference  the batch against the exact crossing of tests/sample_many_ref.py, independent of the code under test
  (C) refusals   QIP_ERR_INVALID, the state unchanged
  (D) mirrors    HipState.sample, the C++ mirror"""
import ctypes as C
import subprocess

from gpu_common import *  # noqa: F401,F403

import measure_ref as R
import sample_many_ref as S
from rustqip_amd import _ffi

pytestmark = pytest.mark.gpu

_IDS = ("c128", "c64")
_STATES = {}
EDGES = (0.0, 1e-300, 1.5)


def _state(n, dtype, norm=1.0):
    """the case state of (n, dtype), shared, never written to"""
    key = (n, np.dtype(dtype), norm)
    if key not in _STATES:
        x = R.make_state(n, R.seed_of(n, dtype), dtype, norm=norm)
        x.setflags(write=False)
        _STATES[key] = x
    return _STATES[key]


def _samples(st, n, count):
    """uniform draws plus the edges: crossing at once, a denormal-sized sample, never crossing, the state's own norm"""
    return np.concatenate([S.samples(n, count), EDGES, [st.norm_sqr()]])


def _singles(st, idx, rs):
    return np.array([st.soft_measure(idx, float(r)) for r in rs], dtype=np.uint64)


def _same(got, want, rs, what):
    assert got.dtype == np.uint64 and got.shape == want.shape, what
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (what, len(bad), [(float(rs[j]), int(got[j]), int(want[j])) for j in bad[:5]])


# ---- (A) identity with the single call --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 3, 6, 10))
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_identity_one_chunk(O, dtype, n):
    """one chunk, shorter than a block's 256 lanes and then 1024 long"""
    x, idx = _state(n, dtype), R.soft_index_set(n)
    with q.HipState(n, dtype) as st:
        st.upload(x)
        rs = _samples(st, n, 67)
        _same(st.soft_measure_many(idx, rs), _singles(st, idx, rs), rs, n)


@pytest.mark.parametrize("n", (12, 14))
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_identity_several_chunks_unnormalised(O, dtype, n):
    """4 and 16 chunks of 1024, several samples per chunk; norm^2 = 0.5, so half the samples never cross"""
    x, idx = _state(n, dtype, norm=0.5), R.soft_index_set(n)
    with q.HipState(n, dtype) as st:
        st.upload(x)
        rs = _samples(st, n, 300)
        got, want = st.soft_measure_many(idx, rs), _singles(st, idx, rs)
        _same(got, want, rs, n)
        assert abs(st.norm_sqr() - 0.5) <= 1e-6 and 100 <= int(np.sum(rs[:300] > 0.5)) <= 200  # (the never-crossing half)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_identity_empty_chunks_before_the_crossing(O, dtype):
    """a basis state at the last index: every chunk before the crossing is empty — small samples come within the margin of
    each of them (the rounds, or the walk's pass over a chunk whose sum is exactly 0)"""
    n, idx = 14, R.soft_index_set(14)
    rs = np.array([1e-12, 1e-10, 0.3, 1.0, 0.0])
    with q.HipState(n, dtype) as st:
        st.init_basis((1 << n) - 1)
        got, want = st.soft_measure_many(idx, rs), _singles(st, idx, rs)
        _same(got, want, rs, "basis")
        last = R.outcome_of(n, idx, (1 << n) - 1)
        assert [int(v) for v in got] == [last, last, last, last, 0]


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_identity_slabs_and_sample_order(O, dtype):
    """many slabs and a ragged last one; the same samples sorted, reversed and repeated"""
    n, count = 16, 4096
    x, idx = _state(n, dtype), R.soft_index_set(n)
    with q.HipState(n, dtype) as st:
        st.upload(x)
        rs = _samples(st, n, count)
        want = _singles(st, idx, rs)
        for slab in (64, 1000):
            st.set_option("sample_slab", slab)
            _same(st.soft_measure_many(idx, rs), want, rs, slab)
            order = np.argsort(rs, kind="stable")
            _same(st.soft_measure_many(idx, rs[order]), want[order], rs[order], (slab, "sorted"))
            _same(st.soft_measure_many(idx, rs[::-1]), want[::-1], rs[::-1], (slab, "reversed"))
            _same(st.soft_measure_many(idx, np.repeat(rs, 4)), np.repeat(want, 4), np.repeat(rs, 4), (slab, "repeated"))


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_identity_one_crowded_chunk(O, dtype):
    """a state with support only inside chunk 5 of 16: every sample lands there, several blocks for one chunk"""
    n, count = 14, 4096
    x = np.zeros(1 << n, dtype=dtype)
    x[5 * 1024:6 * 1024] = _state(10, dtype)
    idx = R.soft_index_set(n)
    with q.HipState(n, dtype) as st:
        st.upload(x)
        rs = _samples(st, n, count)
        got, want = st.soft_measure_many(idx, rs), _singles(st, idx, rs)
        _same(got, want, rs, "crowded")
        assert len(set(int(v) for v in got)) > 1  # (qubit 0 is the top index bit: fixed inside chunk 5)


@pytest.mark.parametrize("n,dtype", R.BIG, ids=_IDS)
def test_identity_large_state(O, n, dtype):
    """512 MiB: the first size whose chunks are longer than 1024 (2048 / 4096 amplitudes, segments of 8 / 16)"""
    x, idx = _state(n, dtype), R.soft_index_set(n)
    with q.HipState(n, dtype) as st:
        st.upload(x)
        rs = _samples(st, n, 2048 - 4)
        assert len(rs) == 2048
        got = st.soft_measure_many(idx, rs)
        _same(got[:32], _singles(st, idx, rs[:32]), rs[:32], n)
        _same(got[-4:], _singles(st, idx, rs[-4:]), rs[-4:], (n, "edges"))
        assert got.shape == (2048,) and len(set(int(v) for v in got)) == 8


@pytest.mark.parametrize("n", (10, 14))
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_identity_index_sets(O, dtype, n):
    x = _state(n, dtype)
    scrambled = [int(v) for v in np.random.default_rng(n).permutation(n)]
    with q.HipState(n, dtype) as st:
        st.upload(x)
        rs = _samples(st, n, 67)
        for idx in (R.soft_index_set(n), [n - 1], scrambled):
            _same(st.soft_measure_many(idx, rs), _singles(st, idx, rs), rs, (n, idx))


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_state_is_not_changed(O, dtype):
    n = 12
    x = _state(n, dtype)
    with q.HipState(n, dtype) as st:
        st.upload(x)
        st.soft_measure_many(R.soft_index_set(n), _samples(st, n, 300))
        assert np.array_equal(st.download(), x)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_ordered_after_queued_work(O, dtype):
    """apply_ops, the batch, apply_ops, the batch — no synchronise in between: each batch sees the state of that point"""
    n, idx = 14, R.soft_index_set(14)
    layer = circuits.h_layer(n)
    rs = np.concatenate([S.samples(n, 60), EDGES])
    with q.HipState(n, dtype) as st, q.HipState(n, dtype) as twin:
        st.init_basis(5)
        twin.init_basis(5)
        st.apply_ops(layer)
        first = st.soft_measure_many(idx, rs)
        st.apply_ops(layer)
        second = st.soft_measure_many(idx, rs)
        twin.apply_ops(layer)
        _same(first, _singles(twin, idx, rs), rs, "after one layer")
        twin.apply_ops(layer)
        _same(second, _singles(twin, idx, rs), rs, "after two layers")
        assert len(set(int(v) for v in first)) > 1


# ---- (B) independent of the code under test ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,n,count,margin", S.MARGIN_CASES, ids=lambda v: getattr(v, "__name__", str(v)))
def test_against_the_exact_crossing(O, dtype, n, count, margin):
    x, idx = _state(n, dtype), R.soft_index_set(n)
    rs = S.margin_samples(dtype, n, count)
    at, dist = S.crossing_many(x, rs)
    for j in (0, 1, count // 2, count - 1):  # the vectorised reference is measure_ref.crossing_ref
        assert (int(at[j]), float(dist[j])) == R.crossing_ref(x, float(rs[j]))
    keep = np.nonzero(dist >= margin)[0]
    print(f"{np.dtype(dtype).name} n={n}: {count - len(keep)} of {count} left out")
    assert count - len(keep) <= count // 100
    want = np.array([R.outcome_of(n, idx, i) for i in at], dtype=np.uint64)
    with q.HipState(n, dtype) as st:
        st.upload(x)
        got = st.soft_measure_many(idx, rs)
    _same(got[keep], want[keep], rs[keep], n)


# ---- (C) refusals -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_refusals(O, dtype):
    n = 5
    x = _state(n, dtype)
    many = _ffi.lib.qipx_state_soft_measure_many
    rs = (C.c_double * 3)(0.1, 0.5, 0.9)
    out = (C.c_uint64 * 3)()
    idx = (C.c_uint64 * 2)(0, 3)
    with q.HipState(n, dtype) as st:
        st.upload(x)

        def refused(call, *args):
            with pytest.raises(q.CircuitError):
                call(*args)
            assert np.array_equal(st.download(), x)

        for bad in ([1, 3, 1], [0, n], [], list(range(n + 1))):  # repeated, index = n, k = 0, k = n + 1
            refused(st.soft_measure_many, bad, [0.1, 0.5, 0.9])
        for args in ((None, 3, out), (rs, 3, None), (None, 3, None)):
            assert many(st._h, idx, 2, *args) == _ffi.QIP_ERR_INVALID
            assert np.array_equal(st.download(), x)
        refused(st.set_option, "sample_slab", 0)
        refused(st.set_option, "sample_slab", -5)
        assert many(st._h, idx, 2, None, 0, None) == _ffi.QIP_OK  # no samples: nothing to do, null arrays allowed
        assert st.soft_measure_many([0, 3], []).shape == (0,)
        assert np.array_equal(st.download(), x)
        # and it still samples
        got = st.soft_measure_many([0, 3], [0.1, 0.5, 0.9])
        assert [int(v) for v in got] == [st.soft_measure([0, 3], r) for r in (0.1, 0.5, 0.9)]


# ---- (D) the mirrors ----------------------------------------------------------------------------------------------------------
def test_sample_draws_from_pcg64(O):
    n, idx = 10, R.soft_index_set(10)
    with q.HipState(n) as st:
        st.upload(_state(n, np.complex128))
        draws = np.random.Generator(np.random.PCG64(5)).random(1000)
        got = st.sample(idx, 1000, seed=5)
        assert got.dtype == np.uint64 and np.array_equal(got, st.soft_measure_many(idx, draws))
        assert not np.array_equal(got, st.sample(idx, 1000, seed=6))
    assert q.ext_abi_version() == 1


def test_cpp_mirror(O, tmp_path):
    n, idx = 10, R.soft_index_set(10)
    x = _state(n, np.complex128)
    rs = np.concatenate([S.samples(n, 200), EDGES])
    exe = str(tmp_path / "test_sample_mirror")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "rustqip_amd", "host"), os.path.join(ROOT, "tests", "cpp", "test_sample_mirror.cpp"),
                    "-o", exe, "-L" + os.path.join(ROOT, "rustqip_amd", "lib"), "-lqip_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "rustqip_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib",
                    "-Wl,-rpath-link,/opt/rocm/lib"], check=True, capture_output=True)
    x.tofile(tmp_path / "state.bin")
    rs.tofile(tmp_path / "samples.bin")
    res = subprocess.run([exe, str(n), str(tmp_path / "state.bin"), str(tmp_path / "samples.bin")] + [str(i) for i in idx],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    with q.HipState(n) as st:
        st.upload(x)
        want = st.soft_measure_many(idx, rs)
    assert [int(v) for v in res.stdout.split()] == [int(v) for v in want]
