"""Uncontrolled X gates absorbed on the host for the interpreter's tile sweeps (tile_absorb_x): a multi-gate sweep of
k_tile_passes no longer gets them as items — they go into the next dense gate on their bit, swap the entries of diagonal gates,
come back in front of a control, and what is left at the end of the segment is applied by the sweep's store (TilePassDesc::flip).
The results are what they were, bit for bit: against one launch per gate (pair_floor = 0) over the whole vector, and against the
CPU oracle on closed sub-cubes.  The host half is replayed without a GPU in tests/test_tile_absorb_x_cpu.py."""
from gpu_common import *  # noqa: F401,F403

from oracle import window_parity as W
from rustqip_amd import _ffi
from rustqip_amd.ops import TILE_PLAN_ABSORB_X, debug_tile_plan, plan_tiles

pytestmark = pytest.mark.gpu

CHUNK = 1 << 24
DENSE = [0.3 + 0.1j, -0.7j, 0.2, 0.9 - 0.4j]
ZERO_ENTRY = [0.5 + 0.25j, 0, 0.3j, 0.8 - 0.1j]


def _headline(n, gates=256):
    return circuits.c2_random_circuit(n, 256, seed=28, single_only=True)[:gates]


def _on_flipped_bits(n):
    """X gates followed by what may and may not take them: dense gates (with zero entries too), diagonal gates, X.X, a control
    and a controlled dense gate on the flipped bit (the X must come back), a swap, and X gates left for the store — on a lane
    bit at load / store time (1), on 11 (tile bit 5 of a Complex<f64> state), on high positions"""
    m = lambda b, mat: q.make_matrix_op([n - 1 - b], mat)  # noqa: E731
    c = lambda cb, op: q.make_control_op([n - 1 - b for b in cb], op)  # noqa: E731
    rz = circuits.rz(0.7)
    return [m(1, circuits.X), m(n - 2, circuits.X), m(7, circuits.H), m(n - 2, rz), m(n - 2, circuits.H), m(11, circuits.X),
            m(9, circuits.X), m(9, ZERO_ENTRY), m(3, circuits.X), m(3, circuits.X), m(8, circuits.X), c([8], m(n - 3, DENSE)),
            m(n - 3, circuits.X), c([2], m(n - 3, DENSE)), m(6, circuits.X), c([4], m(6, [1, 0, 0, 1j])), m(10, circuits.X),
            q.make_swap_op([n - 1 - 10], [n - 1 - 0]), m(7, circuits.X), m(n - 2, circuits.X), m(5, circuits.X), m(5, rz),
            m(n - 1, circuits.H), m(n - 1, circuits.X)]


def _prepared(n, dtype, seed, **options):
    st = q.HipState(n, dtype)
    for k, v in options.items():
        st.set_option(k, v)
    st.init_basis(0)
    st.apply_ops(W.product_state_ops(n, seed=seed)[0])
    return st


def _first_difference(a, b, n):
    N = 1 << n
    for off in range(0, N, CHUNK):
        if not np.array_equal(a.download(off, min(CHUNK, N - off)), b.download(off, min(CHUNK, N - off))):
            return off
    return None


def _jit():
    c = _ffi.jit_counters()
    return {k: c[k] for k in ("kernels_resident_total", "disk_hits", "background_segments")}


def _code(dtype):
    return _ffi.QIP_C64 if dtype == np.complex128 else _ffi.QIP_C32


def _absorbed(n, ops, dtype):
    """(multi-gate steps, items that left the interpreter's lists, steps whose store flips) of the mode-1 plan"""
    plan = debug_tile_plan(n, ops, 1 | TILE_PLAN_ABSORB_X, _code(dtype))
    steps = [s["absorb"] for s in plan["steps"] if "absorb" in s]
    return len(steps), sum(a["dropped"] for a in steps), sum(1 for a in steps if a["flip"])


CASES = {
    "headline22": (22, np.complex128, lambda n: _headline(n)),
    "c2_24": (24, np.complex128, lambda n: circuits.c2_random_circuit(n, 256, seed=28)),  # CNOTs: controls on flipped bits
    "headline30": (30, np.complex128, lambda n: _headline(n, 96)),
    "flipped_bits30": (30, np.complex128, _on_flipped_bits),
    "headline24_f32": (24, np.complex64, lambda n: _headline(n)),
    "flipped_bits22_f32": (22, np.complex64, _on_flipped_bits),
    "c2_30_f32": (30, np.complex64, lambda n: circuits.c2_random_circuit(n, 96, seed=28)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_default_path_is_bit_equal_to_gate_by_gate(name):
    n, dtype, make = CASES[name]
    ops = make(n)
    nsteps, dropped, flips = _absorbed(n, ops, dtype)
    assert nsteps >= 1 and dropped >= 3 and flips >= 1, (nsteps, dropped, flips)  # the case really exercises the rewrite
    jit0 = _jit()
    with _prepared(n, dtype, n, pair_floor=1) as fused, _prepared(n, dtype, n, pair_floor=0) as gbg:
        fused.set_option("profile", 1)
        fused.profile_reset()
        fused.apply_ops(ops)
        prof = fused.profile()
        assert _jit() == jit0  # the interpreter only
        launches = sum(v["launches"] for k, v in prof.items() if k != "tile_sweep_parts")
        assert prof.get("k_tile_passes", {}).get("launches", 0) >= 1 and launches <= len(plan_tiles(n, ops, 1, _code(dtype))), prof
        gbg.apply_ops(ops)
        assert _first_difference(fused, gbg, n) is None


@pytest.mark.parametrize("name", ["c2_24", "flipped_bits30", "flipped_bits22_f32"])
def test_tile_1_interpreter_is_bit_equal_to_gate_by_gate(name):
    # (tile_auto = 0: the interpreter whatever the code-object caches hold, and nothing handed to background helpers)
    n, dtype, make = CASES[name]
    ops = make(n)
    jit0 = _jit()
    with _prepared(n, dtype, 3, tile=1, tile_auto=0) as tiled, _prepared(n, dtype, 3, pair_floor=0) as gbg:
        tiled.apply_ops(ops)
        assert _jit() == jit0
        gbg.apply_ops(ops)
        assert _first_difference(tiled, gbg, n) is None


def test_a_segment_of_x_gates_only_is_one_launch():
    n = 24
    ops = [q.make_matrix_op([n - 1 - b], circuits.X) for b in (1, 7, 11, 7, 9, n - 1)]
    with _prepared(n, np.complex128, 5, pair_floor=1) as fused, _prepared(n, np.complex128, 5, pair_floor=0) as gbg:
        fused.set_option("profile", 1)
        fused.profile_reset()
        fused.apply_ops(ops)
        prof = fused.profile()
        assert sum(v["launches"] for v in prof.values()) == len(plan_tiles(n, ops, 1)) == 1, prof  # empty list: still one sweep
        gbg.apply_ops(ops)
        assert _first_difference(fused, gbg, n) is None


@pytest.mark.parametrize("name,gates", [("c2_24", 256), ("flipped_bits30", None), ("headline30", 64)])
def test_oracle_on_closed_sub_cubes(O, name, gates):
    n, dtype, make = CASES[name]
    ops = make(n)[:gates]
    jit0 = _jit()
    with _prepared(n, dtype, n, pair_floor=1) as st:
        st.set_option("profile", 1)
        agg = W.check_circuit(st, n, ops, O, gate_by_gate=False, seed=7, bases_per_step=2)
        prof = st.profile()
    assert agg["gates"] == len(ops) and agg["skipped"] == 0, agg
    assert agg["max_abs_delta"] == 0.0, agg  # only a -0 may differ
    assert prof.get("k_tile_passes", {}).get("launches", 0) >= 1, prof
    assert _jit() == jit0
