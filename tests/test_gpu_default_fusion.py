"""Option pair_floor on the default path (tile = 0, n >= 22): an apply_ops batch is planned once as tile sweeps in circuit
order (exact commutations only, no relabelling) and every step of >= 2 gates that the byte rule accepts runs as ONE
interpreter sweep; everything else one launch per gate.  The results are those of one launch per gate (pair_floor = 0) bit
for bit.  Helpers and bars: tests/gpu_common.py."""
from gpu_common import *  # noqa: F401,F403

from oracle import window_parity as W
from rustqip_amd import _ffi
from rustqip_amd.ops import plan_tiles

pytestmark = pytest.mark.gpu

CHUNK = 1 << 24  # amplitudes per download when two whole states are compared


def _headline(n):
    return circuits.c2_random_circuit(n, 256, seed=28, single_only=True)  # bench.py's headline: H / X / Rz


def _prepared(n, dtype, pair_floor, seed):
    st = q.HipState(n, dtype)
    st.set_option("pair_floor", pair_floor)
    st.init_basis(0)
    st.apply_ops(W.product_state_ops(n, seed=seed)[0])
    return st


def _first_difference(a, b, n):
    N = 1 << n
    for off in range(0, N, CHUNK):
        if not np.array_equal(a.download(off, min(CHUNK, N - off)), b.download(off, min(CHUNK, N - off))):
            return off
    return None


def _jit():  # what a foreground call compiles, loads or hands to helpers (not what helpers of an earlier test may still finish)
    c = _ffi.jit_counters()
    return {k: c[k] for k in ("kernels_resident_total", "disk_hits", "background_segments")}


def _launches(prof):
    return sum(v["launches"] for k, v in prof.items() if k != "tile_sweep_parts")


@pytest.mark.parametrize("n,dtype", [(22, np.complex128), (24, np.complex128), (30, np.complex128), (30, np.complex64)])
def test_headline_fused_is_bit_equal_to_gate_by_gate(n, dtype):
    ops = _headline(n)
    jit0 = _jit()
    with _prepared(n, dtype, 1, n) as fused:
        fused.set_option("profile", 1)
        fused.profile_reset()
        fused.apply_ops(ops)
        prof = fused.profile()
        fused.set_option("profile", 0)
        assert _jit() == jit0  # the interpreter only: nothing compiled, looked up or spawned
        plan = plan_tiles(n, ops, 1, _ffi.QIP_C64 if dtype == np.complex128 else _ffi.QIP_C32)
        multi = sum(1 for s in plan if len(s) >= 2)
        assert multi >= 4 and _launches(prof) == len(plan), prof  # H / X / Rz steps of >= 2 gates all pay: one sweep each
        if n == 30 and dtype == np.complex128:
            assert multi == 15 and _launches(prof) == 15, prof  # 256 gates -> 15 sweeps, no single-gate step
        with _prepared(n, dtype, 0, n) as gbg:
            gbg.set_option("profile", 1)
            gbg.profile_reset()
            gbg.apply_ops(ops)
            assert _launches(gbg.profile()) == len(ops)  # pair_floor = 0: one launch per gate
            assert _first_difference(fused, gbg, n) is None


@pytest.mark.parametrize("n,gates", [(24, 256), (30, 96)])
def test_headline_fused_matches_the_oracle_on_closed_sub_cubes(O, n, gates):
    ops = _headline(n)[:gates]
    with _prepared(n, np.complex128, 1, n) as st:
        st.set_option("profile", 1)
        agg = W.check_circuit(st, n, ops, O, gate_by_gate=False, seed=7, bases_per_step=2)
        prof = st.profile()
    assert agg["gates"] == gates and agg["skipped"] == 0, agg
    assert agg["max_abs_delta"] == 0.0, agg  # only a -0 may differ
    assert prof.get("k_tile_passes", {}).get("launches", 0) >= 2, prof  # the default path really fused


def test_qft_prefix_gets_no_more_launches_and_pairs_of_phases_stay_apart():
    n = 24
    ops = circuits.c3_qft(n)[:200]
    res = {}
    for pair in (0, 1):
        with _prepared(n, np.complex128, pair, 3) as st:
            st.set_option("profile", 1)
            st.profile_reset()
            st.apply_ops(ops)
            res[pair] = (st.download(), _launches(st.profile()))
    assert res[1][1] <= res[0][1] == len(ops), (res[0][1], res[1][1])
    assert np.array_equal(res[0][0], res[1][0])
    # two controlled phases move 1/4 + 1/4 (selectors above the rows) or 1/2 + 1/2 (target inside a row) of a sweep: the byte
    # rule keeps them on their own kernels (one fused sweep would move a whole one)
    cp = lambda a, b: q.make_control_op([a], q.make_matrix_op([b], [1, 0, 0, cmath.rect(1, 0.4)]))  # noqa: E731
    for pair_ops in ([cp(1, 2), cp(3, 4)], [cp(1, n - 1), cp(3, n - 2)]):
        with _prepared(n, np.complex128, 1, 4) as st:
            st.set_option("profile", 1)
            st.profile_reset()
            st.apply_ops(pair_ops)
            prof = st.profile()
        assert _launches(prof) == 2, prof  # (one fused sweep would be one launch)


def test_batch_with_ops_the_tile_cannot_take_is_bit_equal():
    n = 22
    rng = np.random.default_rng(11)
    c2 = _headline(n)
    k5 = q.make_matrix_op([0, 3, 7, n - 2, n - 5], rand_unitary(5, rng).ravel())
    rows = [[((r * 5 + 1) % 64, 0.5j), (r, 2.0), ((r * 11 + 3) % 64, -0.25)] for r in range(64)]
    sp6 = q.make_sparse_matrix_op([1, 2, 6, 9, n - 1, n - 3], rows)
    swaps = [q.make_swap_op([2], [n - 4]), q.make_swap_op([5, 8], [n - 1, 1]), q.make_swap_op([0], [11])]
    ops = c2[:60] + [k5] + c2[60:120] + swaps + c2[120:180] + [sp6] + c2[180:] + [k5]
    got = {}
    for pair in (0, 1):
        with _prepared(n, np.complex128, pair, 5) as st:
            st.set_option("profile", 1)
            st.profile_reset()
            st.apply_ops(ops)
            got[pair] = (st.download(), st.profile())
    assert np.array_equal(got[0][0], got[1][0])
    assert got[1][1].get("k_tile_passes", {}).get("launches", 0) >= 4, got[1][1]
    assert _launches(got[1][1]) < _launches(got[0][1])


def test_failing_op_reports_its_caller_index():
    n = 22
    ops = _headline(n)[:40]
    bad = ops[:17] + [q.make_matrix_op([n + 3], circuits.H)] + ops[17:]
    with _prepared(n, np.complex128, 1, 6) as st:
        with pytest.raises(Exception, match=r"op 17\b"):
            st.apply_ops(bad)
        st.apply_ops(ops)  # not poisoned: nothing was relabelled
        assert abs(st.norm_sqr() - 1) < 1e-9


def test_program_on_a_default_state_records_gate_by_gate():
    n = 22
    ops = _headline(n)[:64]
    jit0 = _jit()
    with _prepared(n, np.complex128, 1, 8) as st:
        prog = st.compile_program(ops)
        prog.run()
        assert prog.is_graph
        got = st.download()
        prog.close()
    assert _jit() == jit0
    with _prepared(n, np.complex128, 0, 8) as st:
        st.apply_ops(ops)
        want = st.download()
    assert np.array_equal(got, want)
