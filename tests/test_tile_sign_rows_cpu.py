"""Dense 1-qubit gates whose second row is the first up to one sign per column (H, H.X after an absorbed X, Ry(pi/2)): the
interpreter's lists mark them in TileGate::b1 (tile_mark_sign_rows, qip_tile_sched.hip) and k_tile_passes forms both rows of a
marked gate of real entries from row 0's products (pass_dense_signs).  Without a GPU: which items carry the bits, that nothing but
the interpreter's lists does, and a numpy model of the new arithmetic — products once, second row by negation — that must EQUAL
the oracle's gate-by-gate result."""
import cmath

import numpy as np
import pytest

import rustqip_amd as q
from oracle import qip_oracle as O
from oracle import window_parity as W
from rustqip_amd import circuits
from rustqip_amd.ops import (TILE_PLAN_ABSORB_X, TILE_SIGN_NEG0, TILE_SIGN_NEG1, TILE_SIGN_ROWS, debug_tile_plan)

from test_tile_absorb_x_cpu import DTYPES, _Vec, _bits, _c, _m, apply_gate_list

N = 13
X, H = circuits.X, circuits.H
SIGN_BITS = TILE_SIGN_ROWS | TILE_SIGN_NEG0 | TILE_SIGN_NEG1
A, B = 0.6, 0.8
CA, CB = 0.3 + 0.4j, 0.5 - 0.2j
RZ = [cmath.rect(1, -0.35), 0, 0, cmath.rect(1, 0.35)]
ROTATION = [0.6, -0.8, 0.8, 0.6]  # the fuzz suite's real rotation: row 1 is no signed copy of row 0
OTHER = 3  # a Hadamard on this bit rides along so that the step has >= 2 gates


def _random_unitary(seed):
    rng = np.random.default_rng(seed)
    z = rng.normal(size=(2, 2)) + 1j * rng.normal(size=(2, 2))
    return np.linalg.qr(z)[0].ravel()


# name -> (ops in front of the rider, target bit, expected b1 & SIGN_BITS of the item on the target bit)
MARKED = {
    "h": ([_m(N, 8, H)], 8, TILE_SIGN_ROWS | TILE_SIGN_NEG1),
    "x_then_h": ([_m(N, 8, X), _m(N, 8, H)], 8, TILE_SIGN_ROWS | TILE_SIGN_NEG0),
    "h_on_a_row": ([_m(N, 2, H)], 2, TILE_SIGN_ROWS | TILE_SIGN_NEG1),
    "real_neg_neg": ([_m(N, 8, [A, B, -A, -B])], 8, TILE_SIGN_ROWS | TILE_SIGN_NEG0 | TILE_SIGN_NEG1),
    "real_pos_pos": ([_m(N, 8, [A, B, A, B])], 8, TILE_SIGN_ROWS),
    "real_neg_pos": ([_m(N, 10, [A, B, -A, B])], 10, TILE_SIGN_ROWS | TILE_SIGN_NEG0),
    "complex_neg_pos": ([_m(N, 8, [CA, CB, -CA, CB])], 8, TILE_SIGN_ROWS | TILE_SIGN_NEG0),
    "controlled_h": ([_c(N, [9], _m(N, 8, H))], 8, TILE_SIGN_ROWS | TILE_SIGN_NEG1),
}
UNMARKED = {
    "real_rotation": [_m(N, 8, ROTATION)],
    "random_unitary": [_m(N, 8, _random_unitary(5))],
    "conjugate_row": [_m(N, 8, [CA, CB, CA.conjugate(), CB])],
    "one_component_flipped": [_m(N, 8, [CA, CB, complex(-CA.real, CA.imag), CB])],
    "zero_entry": [_m(N, 8, [A, 0, -A, B])],
    "rz": [_m(N, 8, RZ)],
}


def _steps(ops, dt, mode=1 | TILE_PLAN_ABSORB_X):
    return [s for s in debug_tile_plan(N, ops, mode, DTYPES[dt][0])["steps"] if len(s["ops"]) > 1]


def _on_bit(seg, bit):
    tile_pos = seg["low"] + seg["high"]
    hit = [g for g in seg["gates"] if g["kind"] in (0, 1) and g["b0"] != 0xFFFFFFFF and tile_pos[g["b0"]] == bit]
    assert len(hit) == 1, seg["gates"]
    return hit[0]


@pytest.mark.parametrize("dt", ["c64", "c32"])
@pytest.mark.parametrize("name", sorted(MARKED))
def test_marked(name, dt):
    ops, bit, want = MARKED[name]
    (step,) = _steps(ops + [_m(N, OTHER, H)], dt)
    g = _on_bit(step["absorb"], bit)
    assert g["kind"] == 0 and g["nz"] == 15 and g["b1"] & SIGN_BITS == want, g
    assert bool(g["b1"] & 1) == (name != "complex_neg_pos")  # the real-entries bit stands beside the new ones
    # the plan itself (what the generated kernels are written from, and the k_tile_gates form) carries none of the bits
    assert all(pg["b1"] & SIGN_BITS == 0 for pg in step["gates"] if pg["kind"] == 0)


@pytest.mark.parametrize("dt", ["c64", "c32"])
@pytest.mark.parametrize("name", sorted(UNMARKED))
def test_unmarked(name, dt):
    (step,) = _steps(UNMARKED[name] + [_m(N, OTHER, H)], dt)
    g = _on_bit(step["absorb"], 8)
    assert g["b1"] & SIGN_BITS == 0, g
    assert _on_bit(step["absorb"], OTHER)["b1"] & TILE_SIGN_ROWS  # (the rider is a Hadamard)


@pytest.mark.parametrize("dt", ["c64", "c32"])
def test_only_the_interpreter_lists_are_marked(dt):
    """plans without the absorbed form, and wide plans (mode bit 16), hold no marked item: those are what the run-time compiler's
    sources are generated from"""
    ops = circuits.c2_random_circuit(N + 1, 120, seed=28)
    for mode in (1, 2, 1 | 16, 2 | 16):
        plan = debug_tile_plan(N + 1, ops, mode, DTYPES[dt][0])
        kind0 = [g for s in plan["steps"] if len(s["ops"]) > 1 for g in s["gates"] if g["kind"] == 0]
        assert kind0 and all(g["b1"] & ~3 == 0 for g in kind0)
    marked = [g for s in debug_tile_plan(N + 1, ops, 1 | TILE_PLAN_ABSORB_X, DTYPES[dt][0])["steps"] if "absorb" in s
              for g in s["absorb"]["gates"] if g["kind"] == 0 and g["b1"] & TILE_SIGN_ROWS]
    assert len(marked) >= 10


def test_headline_lists_mark_every_hadamard():
    ops = circuits.c2_random_circuit(30, 256, seed=28, single_only=True)
    gates = [g for s in debug_tile_plan(30, ops, 1 | TILE_PLAN_ABSORB_X)["steps"] for g in s["absorb"]["gates"]]
    dense = [g for g in gates if g["kind"] == 0]
    assert len(gates) == 177 and len(dense) == 92  # (92 dense + 85 diagonal: the per-sweep rows of profiles/h_shared_products.md)
    assert all(g["b1"] & TILE_SIGN_ROWS and g["b1"] & 1 for g in dense)
    assert all(bool(g["b1"] & TILE_SIGN_NEG0) != bool(g["b1"] & TILE_SIGN_NEG1) for g in dense)  # H or H.X
    assert any(g["b1"] & TILE_SIGN_NEG0 for g in dense) and any(g["b1"] & TILE_SIGN_NEG1 for g in dense)


# ---- the new arithmetic, replayed ----

def apply_gate_list_signs(v, n, seg):
    """apply_gate_list with the marked gates of real entries as pass_dense_signs_body computes them"""
    tile_pos = seg["low"] + seg["high"]
    idx = np.arange(1 << n, dtype=np.int64)
    shared = 0
    for g in seg["gates"]:
        if not (g["kind"] == 0 and g["b1"] & TILE_SIGN_ROWS and g["b1"] & 1 and g["cmask"] == 0):
            apply_gate_list(v, n, dict(seg, gates=[g]))
            continue
        assert g["nz"] == 15 and not g["b1"] & 2
        ctl = g["omask"]
        p = tile_pos[g["b0"]]
        i0 = idx[((idx & ctl) == ctl) & (((idx >> p) & 1) == 0)]
        i1 = i0 | (1 << p)
        m0, m1 = v.F(g["m"][0][0]), v.F(g["m"][1][0])
        for col, neg in ((0, TILE_SIGN_NEG0), (1, TILE_SIGN_NEG1)):  # what the bits promise, on the numbers the kernel reads
            want = -v.F(g["m"][col][0]) if g["b1"] & neg else v.F(g["m"][col][0])
            assert v.F(g["m"][2 + col][0]) == want
        (a0x, a0y), (a1x, a1y) = v.get(i0), v.get(i1)
        p0x, p0y, p1x, p1y = m0 * a0x, m0 * a0y, m1 * a1x, m1 * a1y
        v.put(i0, (p0x + p1x, p0y + p1y))
        n0, n1 = bool(g["b1"] & TILE_SIGN_NEG0), bool(g["b1"] & TILE_SIGN_NEG1)
        second = lambda s, t: (-s) - t if n0 and n1 else t - s if n0 else s - t if n1 else s + t  # noqa: E731
        v.put(i1, (second(p0x, p1x), second(p0y, p1y)))
        shared += 1
    return shared


def _product_state(n, seed, cdtype):
    return W.product_state_window(n, W.product_state_ops(n, seed)[1], 0, 1 << n).astype(cdtype)


REPLAYED = dict({k: v[0] + [_m(N, OTHER, H)] for k, v in MARKED.items()},
                h_three_pass_bits=[_m(N, 7, H), _m(N, 9, H), _m(N, 12, H)],
                h_on_rows=[_m(N, 0, H), _m(N, 3, H), _m(N, 5, H)],
                x_rz_h=[_m(N, 8, X), _m(N, 3, RZ), _m(N, 8, H)],
                headline13=circuits.c2_random_circuit(N, 120, seed=28, single_only=True))


@pytest.mark.parametrize("dt", ["c64", "c32"])
@pytest.mark.parametrize("name", sorted(REPLAYED))
def test_shared_products_replayed_equal_the_oracle(name, dt):
    code, cdtype = DTYPES[dt]
    ops = REPLAYED[name]
    x = _product_state(N, 11, cdtype)
    plan = debug_tile_plan(N, ops, 1 | TILE_PLAN_ABSORB_X, code)
    st, shared, done = x.copy(), 0, []
    for step in plan["steps"]:
        if "absorb" in step:
            a = step["absorb"]
            v = _Vec(st)
            shared += apply_gate_list_signs(v, N, a)
            st = v.array(cdtype)
            st = st[np.arange(1 << N, dtype=np.int64) ^ sum(1 << p for p in a["flip_pos"])]
        else:
            assert len(step["ops"]) == 1 and "perm" not in step
            st = O.apply_ops_in_place(N, [ops[step["ops"][0]]], st)
        done += step["ops"]
    assert sorted(done) == list(range(len(ops)))
    assert shared >= 1  # (every case holds a plain Hadamard at least)
    assert np.array_equal(st, O.apply_ops_in_place(N, ops, x.copy()))
