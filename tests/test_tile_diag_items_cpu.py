"""Diagonal Matrix ops on two and three qubits as tile items (kind TILE_KIND_DIAG_K; classify_tile_item, qip_tile_sched.hip), without
a GPU: they join multi-gate steps, the scheduler treats them exactly like a controlled 1-qubit diagonal gate of the same footprint,
the lists the interpreter kernel is handed replay to the circuit's dense-matrix product, and segments that hold them are generated
and compile.  Circuits: tests/diag_items.py."""
import cmath

import numpy as np
import pytest

from rustqip_amd import _ffi
from rustqip_amd.ops import TILE_KIND_DIAG_K, TILE_PLAN_ABSORB_X, TILE_PLAN_INTERP, debug_tile_jit, debug_tile_plan, plan_tiles

from diag_items import (ALL_COMBINATIONS, H, X, apply_dense, diag_op, five_op_cases, five_ops, gate1, item_coverage, qaoa, rz, seeded_mix,
                        zz)
from test_tile_plan_cpu import emulate_segment

CASES = five_op_cases()
DTYPES = {"c64": (_ffi.QIP_C64, np.complex128, 1e-13), "c32": (_ffi.QIP_C32, np.complex64, 1e-5)}
RELABEL, WIDE = 4, 16


# ---- 1. fused into one step -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", sorted(CASES))
def test_a_diagonal_gate_between_hadamards_is_one_step_of_five_ops(name, mode):
    for dtype in (_ffi.QIP_C64, _ffi.QIP_C32):
        assert plan_tiles(22, five_ops(22, CASES[name]), mode, dtype) == [[0, 1, 2, 3, 4]]


# ---- 2. the scheduler sees a controlled 1-qubit diagonal of the same footprint ----------------------------------------------------

SCHED_MODES = [1, 2, 1 | RELABEL, 2 | RELABEL, 1 | WIDE, 2 | WIDE, 2 | RELABEL | WIDE]


@pytest.mark.parametrize("mode", SCHED_MODES)
def test_qaoa_layers_plan_like_their_stand_in(mode):
    n = 24
    got = plan_tiles(n, qaoa(n, 2, "diag"), mode)
    assert got == plan_tiles(n, qaoa(n, 2, "stand_in"), mode)
    expected = {1: 8, 2: 5, 1 | RELABEL: 8, 2 | RELABEL: 5, 2 | RELABEL | WIDE: 3}  # (the ring as 4x4 diagonals took 56 steps)
    if mode in expected:
        assert len(got) == expected[mode]
    assert len(got) < len(plan_tiles(n, qaoa(n, 2, "cnot"), mode))  # ... and fewer than CNOT . Rz . CNOT (14 / 8 steps)


@pytest.mark.parametrize("mode", SCHED_MODES)
@pytest.mark.parametrize("n", [16, 22, 24])
def test_seeded_mixes_plan_like_their_stand_in(n, mode):
    covered = set()
    for seed in range(4):
        ops, subs, tags = seeded_mix(n, seed, gates=80)
        for dtype in (_ffi.QIP_C64, _ffi.QIP_C32):
            plan = plan_tiles(n, ops, mode, dtype)
            assert plan == plan_tiles(n, subs, mode, dtype), (n, seed, mode)
        covered |= item_coverage(plan, tags)
    assert covered == ALL_COMBINATIONS, sorted(ALL_COMBINATIONS - covered)


def test_a_lone_phase_where_every_op_bit_reads_one_is_a_controlled_phase():
    """diag(1, 1, 1, f) IS a controlled phase: kind 1 with the other op bit as a control, no table"""
    n = 14
    ops = [gate1(n, 3, H), diag_op(n, [9, 3], [1, 1, 1, cmath.exp(0.4j)]), diag_op(n, [12, 7, 3], [1] * 7 + [1j]), gate1(n, 9, H)]
    plan = debug_tile_plan(n, ops, 1)
    (step,) = plan["steps"]
    assert "diag" not in step and sorted(g["kind"] for g in step["gates"]) == [0, 0, 1, 1]


# ---- 3. what the interpreter kernel is handed, replayed ----------------------------------------------------------------------------

def replay_interp(n, ops, x, dtype, mode):
    """multi-gate steps from their "absorb" export — the X-absorbed list with its diagonal runs, through the numpy model of
    k_tile_passes, then the store's flip — everything else by the dense reference.  Returns (state, plan, diagonal gates replayed)"""
    plan = debug_tile_plan(n, ops, mode | TILE_PLAN_INTERP | TILE_PLAN_ABSORB_X, dtype)
    st = x.copy()
    done, items = [], 0
    for step in plan["steps"]:
        assert "perm" not in step
        if len(step["ops"]) == 1:
            st = apply_dense(n, [ops[step["ops"][0]]], st).astype(x.dtype)
        else:
            a = step["absorb"]
            for seg in (step, a):  # a diagonal item never reaches the kernel as a gate of its own: always steps of a run
                own = [i for i, g in enumerate(seg["gates"]) if g["kind"] == TILE_KIND_DIAG_K]
                assert len(own) == len(seg.get("diag", [])) and sorted(seg["gates"][i]["nz"] for i in own) == list(range(len(own)))
                assert not any(g.get("gate") in own for g in seg["interp"]["gates"])
            items += len(a.get("diag", []))
            emulate_segment(st, n, a, use_interp=True)
            st = st[np.arange(1 << n, dtype=np.int64) ^ sum(1 << p for p in a["flip_pos"])]  # the store: out[t] = tile[t ^ flip]
        done += step["ops"]
    assert sorted(done) == list(range(len(ops)))
    return st, plan, items


def _state(n, seed, cdtype):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    return (v / np.linalg.norm(v)).astype(cdtype)


@pytest.mark.parametrize("dt", ["c64", "c32"])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("n", [12, 13, 14])
def test_interpreter_lists_replay_to_the_dense_matrix_product(n, mode, dt):
    code, cdtype, tol = DTYPES[dt]
    replayed = 0
    for seed in range(2):
        ops, _, tags = seeded_mix(n, seed, gates=50, item_share=0.4)
        x = _state(n, 5 + seed, cdtype)
        got, plan, items = replay_interp(n, ops, x, code, mode)
        want = apply_dense(n, ops, x)
        assert got.dtype == cdtype and float(np.max(np.abs(got - want))) <= tol
        replayed += items
    assert replayed >= 10  # the mixes really put diagonal items into multi-gate steps


@pytest.mark.parametrize("dt", ["c64", "c32"])
def test_replay_with_item_bits_on_lane_bits_pass_bits_outside_and_under_pending_x(dt):
    """one segment each, between H gates on bits 7, 8, 9: an item's bits are pass bits of its pass, lane bits or lie outside the
    tile — every class is met, checked below from the export; an X in front of the item leaves its bit pending when the item arrives"""
    code, cdtype, tol = DTYPES[dt]
    n = 14
    d8 = [cmath.exp(0.2j * (k + 1)) for k in range(8)]
    one = [1, 1, cmath.exp(0.9j), 1]
    cases = {
        "lane": [diag_op(n, [0, 3], zz(0.3))],
        "pass": [diag_op(n, [9, 8], one)],
        "outside": [diag_op(n, [13, 12], zz(0.2)), diag_op(n, [12, 13], one)],
        "mixed3": [diag_op(n, [3, 9, 13], d8), diag_op(n, [13, 0, 8], d8, controls=(12, 4))],
        "controls": [diag_op(n, [0, 8], one, controls=(13,)), diag_op(n, [12, 13], zz(0.1), controls=(3, 9))],
        "x_on_op_bit": [gate1(n, 3, X), diag_op(n, [3, 9], one), gate1(n, 13, X), diag_op(n, [13, 0, 8], d8)],
        "x_on_control": [gate1(n, 4, X), diag_op(n, [0, 8], zz(0.3), controls=(4,)), gate1(n, 0, X)],
    }
    classes = set()
    for name, middle in cases.items():
        ops = [gate1(n, b, H) for b in (7, 8, 9)] + middle + [gate1(n, b, H) for b in (9, 7)] + [gate1(n, 5, rz(0.2))]
        x = _state(n, 11, cdtype)
        got, plan, items = replay_interp(n, ops, x, code, 1)
        assert len(plan["steps"]) == 1 and items == sum(1 for o in middle if o.kind != "Matrix" or len(o.indices) > 1), name
        assert float(np.max(np.abs(got - apply_dense(n, ops, x)))) <= tol, name
        a = plan["steps"][0]["absorb"]
        for gi, g in enumerate(a["gates"]):
            if g["kind"] == TILE_KIND_DIAG_K:
                (pb,) = [ps["pb"] for ps in a["passes"] if ps["first"] <= gi < ps["first"] + ps["count"]]
                classes |= {"outside" if b == 0xFFFFFFFF else "pass" if b in pb else "lane" for b in a["diag"][g["nz"]]["bits"]}
        if name.startswith("x_on"):  # the X came back in front of the item: the table is not permuted
            assert a["dropped"] <= 1 and [d["f"] for d in a["diag"]] == [d["f"] for d in plan["steps"][0]["diag"]]
    assert classes == {"lane", "pass", "outside"}


@pytest.mark.parametrize("mode", [1, 2])
def test_wide_plans_with_diagonal_items_keep_their_tables(mode):
    """the wide export: the gates in the plan's order, every diagonal item applied from its "diag" entry and the gate's masks"""
    n = 16
    ops, _, _ = seeded_mix(n, 3, gates=40, item_share=0.4)
    plan = debug_tile_plan(n, ops, mode | WIDE)
    x = _state(n, 2, np.complex128)
    st = x.copy()
    idx = np.arange(1 << n, dtype=np.int64)
    seen = 0
    for step in plan["steps"]:
        if len(step["ops"]) == 1:
            st = apply_dense(n, [ops[step["ops"][0]]], st)
            continue
        assert step["wide"] == 1
        tile_pos = step["low"] + step["high"]
        assert sorted(step["order"]) == list(range(len(step["ops"])))
        # gate by gate in the plan's order: the existing kinds as the ops they stand for, the new one from its exported table and bits
        for gi, g in enumerate(step["gates"]):
            if g["kind"] != TILE_KIND_DIAG_K:
                st = apply_dense(n, [ops[step["ops"][step["order"][gi]]]], st)
                continue
            d = step["diag"][g["nz"]]
            ctl = g["omask"] | sum(1 << tile_pos[b] for b in range(13) if (g["cmask"] >> b) & 1)
            assert all(p == (tile_pos[b] if b != 0xFFFFFFFF else p) for b, p in zip(d["bits"], d["pos"]))
            sub = np.zeros_like(idx)
            for p in d["pos"]:
                sub = (sub << 1) | ((idx >> p) & 1)
            f = np.array([complex(*e) for e in d["f"]])[sub]
            st = np.where((idx & ctl) == ctl, f * st, st)
            seen += 1
    assert seen >= 5 and float(np.max(np.abs(st - apply_dense(n, ops, x)))) <= 1e-13


# ---- 4. generated segments ----------------------------------------------------------------------------------------------------------

def _jit_circuit(n, gamma):
    top = n - 1
    return [gate1(n, 3, H), gate1(n, 9, H), diag_op(n, [3, 9], zz(gamma)), diag_op(n, [top, 0, 9], [1, 1j, cmath.exp(1j * gamma), 1, -1, 1, 1, 1]),
            diag_op(n, [9, top], [1, cmath.exp(2j * gamma), 1, 1], controls=(4,)), gate1(n, top, rz(0.1)), gate1(n, 3, H), gate1(n, 9, H)]


@pytest.mark.parametrize("dt", ["c64", "c32"])
@pytest.mark.parametrize("wide", [0, WIDE], ids=["narrow", "wide"])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("n", [14, 16])
def test_segments_with_diagonal_items_are_generated_and_compile(n, mode, wide, dt):
    PARAMS, MERGE, FMA = 64, 128, 32
    code = DTYPES[dt][0]
    a = debug_tile_jit(n, _jit_circuit(n, 0.3), mode | wide | PARAMS, code)
    assert a["segments"] >= 1 and a["code_bytes"] > 0
    assert "diagonal on 2 bits" in a["first_source"] and "diagonal on 3 bits" in a["first_source"]
    # a new angle is new kernel data, not a new kernel; a unit entry that stops being one is a new kernel
    assert debug_tile_jit(n, _jit_circuit(n, 0.45), mode | wide | PARAMS, code)["first_source"] == a["first_source"]
    assert debug_tile_jit(n, _jit_circuit(n, 0.0), mode | wide | PARAMS, code)["first_source"] != a["first_source"]
    if mode == 2:  # tile_merge / tile_fma (tile = 2 only): the items join the run of diagonal gates as factors
        m = debug_tile_jit(n, _jit_circuit(n, 0.3), mode | wide | PARAMS | MERGE | FMA, code)
        assert m["segments"] >= 1 and m["code_bytes"] > 0 and "one run of diagonal gates" in m["first_source"]
        assert "diagonal on 2 bits" not in m["first_source"]
