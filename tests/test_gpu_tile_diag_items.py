"""Diagonal Matrix ops on two and three qubits inside tile sweeps (tile item kind TILE_KIND_DIAG_K) on the GPU: the default path
(tile = 0, pair_floor = 1, n >= 22) fuses them with their neighbours bit for bit, tile = 1 through the interpreter, compiled narrow
and wide segments and relabelling equals gate by gate, tile = 2 with merged runs and fused multiply-adds keeps the 1e-12 bar, and
a program replays them.  Circuits: tests/diag_items.py; the host side of all this is tests/test_tile_diag_items_cpu.py."""
from gpu_common import *  # noqa: F401,F403

from diag_items import ALL_COMBINATIONS, five_op_cases, five_ops, item_coverage, seeded_default_mix, seeded_mix
from rustqip_amd import _ffi
from rustqip_amd.ops import plan_tiles

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [np.complex128, np.complex64], ids=["c64", "c32"])
CASES = five_op_cases()


def _dt(dtype):
    return _ffi.QIP_C64 if dtype == np.complex128 else _ffi.QIP_C32


def _tol(dtype):
    return TOL64 if dtype == np.complex128 else TOL32


def _launches(prof):
    return sum(v["launches"] for k, v in prof.items() if k != "tile_sweep_parts")


def _run(n, x, ops, times=1, **options):
    """ops applied `times` times to a fresh state holding x, under the given per-handle options: (the vector, the profile, norm)"""
    with q.HipState(n, x.dtype) as st:
        for k, v in options.items():
            st.set_option(k, v)
        st.upload(x)
        st.set_option("profile", 1)
        st.profile_reset()
        for _ in range(times):
            st.apply_ops(ops)
        prof = st.profile()
        return st.download(), prof, st.norm_sqr()


def _why(a, b):
    bad = np.flatnonzero(a != b)
    return f"{bad.size} amplitudes differ, first at index {bad[0]}, max|d| = {np.max(np.abs(a - b)):.3e}" if bad.size else "equal"


@pytest.fixture(scope="module")
def oracle_of():
    """want(n, key, ops, x): the oracle's Complex<f64> result, computed once per key"""
    from oracle import qip_oracle as O

    memo = {}

    def want(n, key, ops, x):
        if key not in memo:
            memo[key] = O.apply_ops_in_place(n, ops, x.astype(np.complex128))
        return memo[key]

    return want


# ---- 1. the default path at n = 22, the smallest size at which it fuses -------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("name", sorted(CASES))
def test_default_path_runs_the_five_ops_as_one_launch(name, dtype, oracle_of):
    n = 22
    ops = five_ops(n, CASES[name])
    x32 = rand_state(n, 40, np.complex64)
    x = x32.astype(dtype)
    fused, pf, _ = _run(n, x, ops, pair_floor=1)
    gbg, pg, _ = _run(n, x, ops, pair_floor=0)
    assert _launches(pf) == 1 and pf["k_tile_passes"]["launches"] == 1, pf
    assert _launches(pg) == 5 and pg["k_phase" if name in ("phase_on_01", "cz_4x4") else "k_diag"]["launches"] == 1, pg  # (an H alone may be a one-op sweep)
    assert np.array_equal(fused, gbg), _why(fused, gbg)
    want = oracle_of(n, name, ops, x32)
    if dtype == np.complex128:  # every op launched alone is the oracle's unfused fold: bit for bit
        assert np.array_equal(fused, want), _why(fused, want)
    else:
        assert float(np.max(np.abs(fused - want))) <= TOL32


# ---- 2. seeded batches: every existing kind with diagonal items on row bits, tile bits and high bits --------------------------------

MIX_SEEDS = (0, 3)  # together they put every (bit class, k, controlled) combination into a multi-gate step, at both sizes


@pytest.mark.parametrize("seed", MIX_SEEDS)
@pytest.mark.parametrize("n", [22, 23])
def test_seeded_default_batches_are_bit_equal_to_gate_by_gate_and_match_the_oracle(n, seed, oracle_of):
    ops, tags = seeded_default_mix(n, seed, gates=60)
    x32 = rand_state(n, 60 + seed, np.complex64)
    want = oracle_of(n, ("mix", n, seed), ops, x32)
    for dtype in (np.complex128, np.complex64):
        x = x32.astype(dtype)
        fused, pf, _ = _run(n, x, ops, pair_floor=1)
        gbg, pg, _ = _run(n, x, ops, pair_floor=0)
        where = f"n={n} seed={seed} {np.dtype(dtype).name}"
        assert np.array_equal(fused, gbg), f"{where}: pair_floor 1 vs 0: {_why(fused, gbg)}"
        assert _launches(pf) < _launches(pg) and pf.get("k_tile_passes", {}).get("launches", 0) >= 1, (where, pf, pg)
        if dtype == np.complex128:  # every op launched alone is the oracle's unfused fold: bit for bit
            assert np.array_equal(fused, want), f"{where}: oracle: {_why(fused, want)}"
        else:
            assert float(np.max(np.abs(fused - want))) <= TOL32, where
        # what the batches of this size hold between them (host arithmetic): every combination inside a multi-gate step, tables with
        # and without unit entries, lone phases at sub-indices with zero bits
        covered, shapes = set(), set()
        for other in MIX_SEEDS:
            ops_o, tags_o = seeded_default_mix(n, other, gates=60)
            covered |= item_coverage(plan_tiles(n, ops_o, 1, _dt(dtype)), tags_o)
            shapes |= {t[3] for t in tags_o if t is not None}
        assert covered == ALL_COMBINATIONS, (where, sorted(ALL_COMBINATIONS - covered))
        assert shapes == {"full", "some", "exact", "phase0"}


# ---- 3. tile = 1 / 2 at n = 16, above the 13 bits of a wide tile --------------------------------------------------------------------

N16 = 16


def _circuit16():
    ops, _, tags = seeded_mix(N16, 5, gates=36, item_share=0.4)
    return ops, tags


VARIANTS = {
    "interpreted": {"tile": 1},
    "tile_jit": {"tile": 1, "tile_jit": 1},
    "tile_jit_wide": {"tile": 1, "tile_jit": 1, "tile_wide": 1},
    "tile_relabel": {"tile": 1, "tile_relabel": 2},
}


@pytest.fixture(scope="module")
def gate_by_gate16():
    memo = {}

    def get(dtype):
        if dtype not in memo:
            ops, _ = _circuit16()
            memo[dtype] = _run(N16, rand_state(N16, 16, dtype), ops, tile=0)
        return memo[dtype]

    return get


@DTYPES
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_tile_1_sweeps_with_diagonal_items_equal_gate_by_gate(variant, dtype, gate_by_gate16):
    ops, tags = _circuit16()
    mode = 1 | (16 if variant == "tile_jit_wide" else 0) | (12 if variant == "tile_relabel" else 0)
    plan = plan_tiles(N16, ops, mode, _dt(dtype))
    multi = [s for s in plan if len(s) >= 2]
    assert 2 <= len(multi) <= 4 and sum(1 for s in multi for i in s if tags[i] is not None) >= 6, plan  # premise
    gbg, pg, _ = gate_by_gate16(dtype)
    before = _ffi.jit_counters()["kernels_resident_total"]
    got, prof, norm = _run(N16, rand_state(N16, 16, dtype), ops, **VARIANTS[variant])
    compiled = _ffi.jit_counters()["kernels_resident_total"] - before
    # (compiled segments are booked under the interpreter's profile class: the segments that became resident tell them apart)
    assert compiled >= 2 if "tile_jit" in VARIANTS[variant] else compiled == 0, (variant, compiled)
    assert _launches(prof) < _launches(pg) and prof["k_tile_passes"]["launches"] >= 2, prof
    assert np.array_equal(got, gbg), _why(got, gbg)
    assert abs(norm - 1) <= (1e-12 if dtype == np.complex128 else 1e-5)


@DTYPES
@pytest.mark.parametrize("wide", [0, 1], ids=["narrow", "wide"])
def test_tile_2_with_merged_runs_and_fma_keeps_the_bar(wide, dtype, oracle_of):
    ops, _ = _circuit16()
    x = rand_state(N16, 16, dtype)
    before = _ffi.jit_counters()["kernels_resident_total"]
    got, prof, norm = _run(N16, x, ops, tile=2, tile_jit=1, tile_wide=wide, tile_fma=1, tile_merge=1)
    assert _ffi.jit_counters()["kernels_resident_total"] > before  # the sweeps ran as compiled segments
    want = oracle_of(N16, ("n16", np.dtype(dtype).name), ops, x)
    assert prof["k_tile_passes"]["launches"] >= 1, prof
    assert float(np.max(np.abs(got - want))) <= _tol(dtype)
    assert abs(norm - 1) <= (1e-12 if dtype == np.complex128 else 1e-5)


# ---- 4. programs --------------------------------------------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("n,options", [(16, {"tile": 1}), (22, {})], ids=["n16_tile1", "n22_default"])
def test_a_program_run_twice_equals_apply_ops_twice(n, options, dtype):
    ops, _, tags = seeded_mix(n, 2, gates=30, item_share=0.4)
    assert sum(t is not None for t in tags) >= 8
    x = rand_state(n, 21, dtype)
    want, _, _ = _run(n, x, ops, times=2, **options)
    with q.HipState(n, dtype) as st:
        for k, v in options.items():
            st.set_option(k, v)
        st.upload(x)
        prog = st.compile_program(ops)
        prog.run()
        prog.run()
        got = st.download()
        prog.close()
    assert np.array_equal(got, want), _why(got, want)
