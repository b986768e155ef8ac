"""The interpreter kernel reads its lists in a wire format of 64-byte blocks (csrc/qip_tile_wire.h): one block per list entry with
everything up to m[0], m[1], a second block for m[2], m[3], one block per run item whose element mask is resolved into a form
(all eight, a half by a pass bit, both halves with a factor each, or per-element tests).  These lists are chosen for what that
code can get wrong: fields at their largest values, the second block, merged and lone halves, irregular masks, runs that whole
blocks skip, a run that starts beyond item 255, dense items behind a run.  Every list must give, bit for bit, what one launch per
gate gives from the same seeded product state; which path each list reaches is checked on the host from the lists the kernel is
really handed."""
import cmath
import math

import numpy as np
import pytest

import rustqip_amd as q
from oracle import window_parity as W
from rustqip_amd import _ffi, circuits
from rustqip_amd.ops import TILE_PLAN_ABSORB_X, TILE_PLAN_INTERP, debug_tile_plan

# TileOp (csrc/qip_kernels.h), as exported in the "op" of a gate
DIAG_UNIFORM, DIAG_LANE, DIAG_LANE_CTL, DIAG_REG, DENSE, DENSE_LANE, DENSE2Q, SWAP, DENSE3Q = 0, 1, 2, (3, 4, 5), (6, 7, 8), (9, 10, 11), range(12, 18), (18, 19, 20), range(21, 27)
MAX_GATES = 256  # kTileMaxGates

RY = [math.cos(0.15), -math.sin(0.15), math.sin(0.15), math.cos(0.15)]
RX = [math.cos(0.2), -1j * math.sin(0.2), -1j * math.sin(0.2), math.cos(0.2)]   # complex entries: all four products of both rows
CPLX = [0.3 + 0.1j, -0.7j, 0.2 - 0.6j, 0.9 - 0.4j]                              # four different complex entries (m[2], m[3] are their own)
UPPER, LOWER = [1, 0.5, 0, 1], [1, 0, 0.5 - 0.25j, 1]                           # a zero entry in the second / first row
LO = (0x55, 0x33, 0x0F)  # element masks of the half with pass bit J = 0


def _dt(dtype):
    return _ffi.QIP_C64 if dtype == np.complex128 else _ffi.QIP_C32


def _pos(n, dtype):
    """A, B, C: the dense targets of the first pass (pass bits J = 0, 1, 2); L0, L1: lane bits; C, D, E, F, G: dense targets on five
    positions above the rows, so the tile's five free bits are exactly these and G is the highest tile bit (a lane bit of the first
    pass); OUT: outside the tile, the top index bit unless the rows' sixth position is there"""
    two = [q.make_matrix_op([0], circuits.H), q.make_matrix_op([1], circuits.H)]
    p5 = debug_tile_plan(n, two, 1 | TILE_PLAN_ABSORB_X, _dt(dtype))["steps"][0]["absorb"]["low"][5]
    return dict(A=1, B=3, C=7, L0=0, L1=2, D=6, E=8, F=9, G=10, OUT=n - 1 if p5 != n - 1 else 5)


def _lists(n, dtype):
    p = _pos(n, dtype)
    A, B, C, L0, L1, D, E, F, G, OUT = (p[k] for k in ("A", "B", "C", "L0", "L1", "D", "E", "F", "G", "OUT"))

    def m(pp, mat):
        return q.make_matrix_op([n - 1 - pp], mat)

    def ctl(cs, op):
        return q.make_control_op([n - 1 - c for c in cs], op)

    def ph(t):
        return [1, 0, 0, cmath.rect(1, t)]

    def hp(t):  # the unit entry second: only the half with the target bit 0 is multiplied
        return [cmath.rect(1, t), 0, 0, 1]

    def diag3(ps, k):
        return q.make_matrix_op([n - 1 - x for x in ps], np.diag([cmath.rect(1, 0.01 * k + 0.1 * (e + 1)) for e in range(8)]).ravel())

    rng = np.random.default_rng(11)
    u2 = np.linalg.qr(rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4)))[0]
    u3 = np.linalg.qr(rng.standard_normal((8, 8)) + 1j * rng.standard_normal((8, 8)))[0]
    H, X, rz = circuits.H, circuits.X, circuits.rz
    blocks = [  # the second block, and the header fields at their largest
        m(A, RX), m(L0, rz(0.11)), m(B, UPPER), m(C, LOWER), m(L1, ph(0.3)), m(A, CPLX),
        ctl([OUT], m(B, CPLX)), m(C, H), m(OUT, rz(0.31)), m(A, H),      # control / diagonal target outside, on the top bit
        ctl([G], m(L0, ph(0.45))), m(B, H),                                # lane control on the highest lane bit, folded into a factor
        ctl([G], m(B, RY)), ctl([G], m(C, CPLX)),                          # ... selecting a dense update
        ctl([G], m(A, rz(0.2))), m(C, RX), ctl([G, OUT], m(L1, rz(0.6))), m(B, RX),
        m(G, H), m(A, CPLX), m(D, RX), m(E, H), m(F, UPPER),
    ]
    runs = [  # every element form of a run item
        m(A, H), m(B, H), m(C, H),
        m(A, rz(0.1)), m(B, rz(0.2)), m(C, rz(0.3)),                       # both entries non-unit: one item, two factors
        m(A, ph(0.4)), m(B, ph(0.5)), m(C, ph(0.6)),                       # one unit entry: a lone high half
        m(A, hp(0.7)), m(B, hp(0.8)), m(C, hp(0.9)),                       # ... a lone low half
        ctl([A], m(B, ph(0.8))), ctl([A, B], m(C, ph(0.9))),               # 2 and 1 of the eight elements
        ctl([A], m(L0, ph(0.25))), m(L0, rz(0.3)), m(L1, ph(0.35)),        # half by a control | all eight, selected / conditional per lane
        ctl([OUT], m(A, rz(0.35))), m(OUT, ph(0.2)), ctl([OUT], m(L0, rz(0.5))),   # blocks whose base fails the outside condition skip
        ctl([G], m(B, rz(0.15))), ctl([G, OUT], m(C, rz(0.45))),           # both halves under a lane condition on the highest lane bit
        m(B, RY), m(C, rz(0.55)), m(A, rz(0.65)),
        m(G, H), m(G, rz(0.75)), m(A, rz(0.85)), m(D, H), m(E, H), m(E, rz(0.95)), m(F, H), m(D, ph(0.05)),
    ]
    trip = [(A, L0, OUT), (B, C, G), (L1, OUT, C), (C, A, B), (L0, L1, G)]
    long_run = ([m(A, H)] + [diag3(trip[k % 5], k) for k in range(126)] + [m(B, CPLX)] +
                [diag3(trip[(k + 2) % 5], 200 + k) for k in range(MAX_GATES - 128)])
    after_run = [  # dense 2- and 3-qubit items behind a run, and an X left to the store
        m(A, H), m(L0, rz(0.3)), m(OUT, ph(0.4)), m(B, rz(0.3)), q.make_matrix_op([n - 1 - A, n - 1 - C], u2.ravel()),
        m(L1, rz(0.2)), m(C, ph(0.7)), m(A, rz(0.9)), q.make_matrix_op([n - 1 - C, n - 1 - A, n - 1 - B], u3.ravel()),
        m(A, rz(0.25)), m(L0, ph(0.15)), m(C, CPLX), m(B, X),
    ]
    return {"blocks": blocks, "runs": runs, "long_run": long_run, "after_run": after_run}


def _handed(n, ops, dtype):
    """what the interpreter is handed for `ops` (host only): per multi-gate step its gate list, the rewritten list with its runs, the
    run items, the tile's high positions and the store's flip"""
    plan = debug_tile_plan(n, ops, 1 | TILE_PLAN_ABSORB_X | TILE_PLAN_INTERP, _dt(dtype))
    return [st["absorb"] for st in plan["steps"] if "absorb" in st]


@pytest.mark.parametrize("dtype", [np.complex128, np.complex64], ids=["c64", "c32"])
@pytest.mark.parametrize("n", [12, 14, 22])
def test_premise_the_lists_reach_the_paths_they_are_meant_for(n, dtype):
    lists, p = _lists(n, dtype), _pos(n, dtype)
    segs = _handed(n, lists["blocks"], dtype)
    gates = [g for s in segs for g in s["gates"]]
    dense = [g for g in gates if g["kind"] == 0 and g["op"] in DENSE and not g["b1"] & 2]
    assert any(not g["b1"] & 1 and g["nz"] == 15 for g in dense), "complex dense gate: all of m[0..3]"
    assert {g["nz"] for g in dense} >= {15, 11, 13}, sorted({g["nz"] for g in dense})  # m[2] == 0 (UPPER) / m[1] == 0 (LOWER)
    top = 1 << p["OUT"]
    assert any(g["omask"] & top and g["kind"] == 0 for g in gates), "dense gate with a control outside the tile"
    assert any(g["op"] in (DIAG_UNIFORM, DIAG_LANE_CTL) and g["tpos_out"] == p["OUT"] for g in gates), "diagonal target outside the tile"
    if n >= 14 or dtype == np.complex64:
        assert p["OUT"] == n - 1  # the top index bit: omask and tpos_out at their largest
    hi_lane = 1 << 10
    assert all(s["high"][-1] == p["G"] for s in segs if len(s["high"]) == 5), [s["high"] for s in segs]
    assert any(g["cm_lane"] & hi_lane and g["op"] in DENSE_LANE for g in gates), "dense gate selected by the highest lane bit"
    assert any(g["cm_lane"] & hi_lane and g["kind"] == 1 for g in gates), "diagonal gate with the highest lane bit as a control"

    segs = _handed(n, lists["runs"], dtype)
    items = [it for s in segs for it in s["interp"]["items"]]
    cond = lambda it: (it["lane"], it["out"], it["sel"])  # noqa: E731
    pairs = [(a, b) for a, b in zip(items, items[1:]) if a["emask"] ^ b["emask"] == 0xFF and cond(a) == cond(b) and not a["sel"]]
    for j in range(3):
        assert any(a["emask"] == LO[j] for a, _ in pairs), f"both halves by pass bit {j}: one wire item"
        lone = [b for a, b, c in zip(items, items[1:], items[2:]) if a["emask"] ^ b["emask"] != 0xFF and b["emask"] ^ c["emask"] != 0xFF]
        assert any(b["emask"] == LO[j] for b in lone) and any(b["emask"] == LO[j] ^ 0xFF for b in lone), f"lone halves by pass bit {j}"
    assert any(a["lane"][0] & hi_lane for a, _ in pairs), "both halves under a condition on the highest lane bit"
    assert any(a["out"][0] for a, _ in pairs), "both halves under an outside condition"
    assert {bin(it["emask"]).count("1") for it in items} >= {8, 4, 2, 1}, "irregular masks: 2 and 1 of eight elements"
    assert any(it["sel"] for it in items) and any(it["emask"] == 0xFF and not it["sel"] and it["lane"][0] for it in items)
    assert any(it["out"][0] & (1 << p["OUT"]) for it in items), "a run item that blocks skip"

    segs = _handed(n, lists["long_run"], dtype)
    starts = [g["run"] for s in segs for g in s["interp"]["gates"] if "run" in g]
    assert any(first > 255 and count >= 8 for first, count in starts), starts  # a run that starts beyond item 255
    assert max(len(s["gates"]) for s in segs) >= 128, [len(s["gates"]) for s in segs]

    segs = _handed(n, lists["after_run"], dtype)
    assert any(s["flip"] for s in segs), "an X left to the store"
    seen = set()
    for s in segs:
        run_before = False
        for g in s["interp"]["gates"]:
            if "run" in g:
                run_before = True
            elif run_before and s["gates"][g["gate"]]["op"] in DENSE2Q:
                seen.add(2)
            elif run_before and s["gates"][g["gate"]]["op"] in DENSE3Q:
                seen.add(3)
    assert seen == {2, 3}, seen


def _start(n, dtype):
    with q.HipState(n, dtype) as st:
        st.init_basis(0)
        st.apply_ops(W.product_state_ops(n, seed=n)[0])
        return st.download()


_START = {}


def _run(n, dtype, ops, **options):
    key = (n, np.dtype(dtype).name)
    if key not in _START:
        _START[key] = _start(n, dtype)
    with q.HipState(n, dtype) as st:
        for k, v in options.items():
            st.set_option(k, v)
        st.upload(_START[key])
        st.set_option("profile", 1)
        st.profile_reset()
        st.apply_ops(ops)
        prof = st.profile()
        return st.download(), prof


def _why(a, b):
    bad = np.flatnonzero(a != b)
    return f"{bad.size} amplitudes differ, first at index {bad[0]}, max|d| = {np.max(np.abs(a - b)):.3e}" if bad.size else "equal"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["blocks", "runs", "long_run", "after_run"])
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64], ids=["c64", "c32"])
@pytest.mark.parametrize("n", [12, 14])
def test_wire_lists_are_bit_equal_to_one_launch_per_gate(n, dtype, name):
    ops = _lists(n, dtype)[name]
    got, prof = _run(n, dtype, ops, tile=1, tile_jit=0, tile_auto=0)
    # (one launch per gate; mfma = 0: a dense 3-qubit gate launched alone is then the unfused fold that a sweep performs)
    want, _ = _run(n, dtype, ops, tile=0, pair_floor=0, mfma=0)
    assert prof.get("k_tile_passes", {}).get("launches", 0) >= 1, prof  # the interpreter really ran
    assert np.array_equal(got, want), f"n={n} {np.dtype(dtype).name} {name}: {_why(got, want)}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["blocks", "runs", "after_run"])
def test_default_path_wire_lists_are_bit_equal_to_one_launch_per_gate(name):
    n = 22
    ops = _lists(n, np.complex128)[name]
    got, prof = _run(n, np.complex128, ops, pair_floor=1)
    want, _ = _run(n, np.complex128, ops, tile=0, pair_floor=0, mfma=0)
    assert prof.get("k_tile_passes", {}).get("launches", 0) >= 1, prof
    assert np.array_equal(got, want), f"n={n} {name}: {_why(got, want)}"
