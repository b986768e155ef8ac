"""Uncontrolled X gates absorbed on the host for the interpreter's tile sweeps (tile_absorb_x, qip_tile_sched.hip), without a GPU.

qip_hip_debug_tile_plan mode bit 4096 exports, per multi-gate step, what k_tile_passes is really handed: the rewritten gate list,
its passes and the flip its store applies.  A numpy model replays that form — the gates in list order with the kernel's own
arithmetic (every product and sum rounded by itself, in the state's precision), then the flip — and the result must EQUAL the
oracle's gate-by-gate result: the rewrite moves amplitudes and reorders the two terms of a sum, it rounds nothing differently.
The model multiplies by zero entries and by unit factors where the kernel skips them; for finite amplitudes that changes at most
the sign of a zero, which == ignores (as everywhere else in the bit-equality tests)."""
import cmath
import hashlib
import math

import numpy as np
import pytest

import rustqip_amd as q
from oracle import qip_oracle as O
from rustqip_amd import _ffi, circuits
from rustqip_amd.ops import TILE_BITS, TILE_PLAN_ABSORB_X, TILE_PLAN_INTERP, debug_tile_plan

from fuzz_ops import fuzz_circuit, seeded_default_batch
from test_tile_plan_cpu import emulate_segment

OUTSIDE = 0xFFFFFFFF
DTYPES = {"c64": (_ffi.QIP_C64, np.complex128), "c32": (_ffi.QIP_C32, np.complex64)}
X, H = circuits.X, circuits.H
S2 = math.sqrt(0.5)


def _bits(mask):
    return [b for b in range(64) if (mask >> b) & 1]


class _Vec:
    """a state as two real arrays, so that every product and every sum is one rounding (numpy's complex multiply may fuse)"""

    def __init__(self, st):
        self.re, self.im = st.real.copy(), st.imag.copy()
        self.F = self.re.dtype.type

    def get(self, i):
        return self.re[i], self.im[i]

    def put(self, i, v):
        self.re[i], self.im[i] = v

    def number(self, pair):
        return self.F(pair[0]), self.F(pair[1])

    def array(self, cdtype):
        out = np.empty(self.re.shape, dtype=cdtype)
        out.real, out.imag = self.re, self.im
        return out


def _cmul(m, x):  # qip_kernels.h cmul
    return m[0] * x[0] - m[1] * x[1], m[0] * x[1] + m[1] * x[0]


def _cadd(a, b):
    return a[0] + b[0], a[1] + b[1]


def apply_gate_list(v, n, seg):
    """the gates of one exported segment, in list order, on the whole vector: tile-index bits -> amplitude-index positions"""
    tile_pos = seg["low"] + seg["high"]
    assert len(tile_pos) == TILE_BITS and len(set(tile_pos)) == TILE_BITS
    idx = np.arange(1 << n, dtype=np.int64)
    mats = seg["mats"]
    for g in seg["gates"]:
        ctl = g["omask"] | sum(1 << tile_pos[b] for b in _bits(g["cmask"]))
        on = (idx & ctl) == ctl
        kind = g["kind"]
        if kind == 0:
            p = tile_pos[g["b0"]]
            i0 = idx[on & (((idx >> p) & 1) == 0)]
            i1 = i0 | (1 << p)
            m = [v.number(e) for e in g["m"]]
            a0, a1 = v.get(i0), v.get(i1)
            v.put(i0, _cadd(_cmul(m[0], a0), _cmul(m[1], a1)))
            v.put(i1, _cadd(_cmul(m[2], a0), _cmul(m[3], a1)))
        elif kind == 1:
            p = g["tpos_out"] if g["b0"] == OUTSIDE else tile_pos[g["b0"]]
            for h in range(2):
                i = idx[on & (((idx >> p) & 1) == h)]
                v.put(i, _cmul(v.number(g["m"][h]), v.get(i)))
        elif kind == 2:
            pa, pb = tile_pos[g["b0"]], tile_pos[g["b1"]]
            i10 = idx[on & (((idx >> pa) & 1) == 1) & (((idx >> pb) & 1) == 0)]
            i01 = (i10 & ~(1 << pa)) | (1 << pb)
            a, b = v.get(i10), v.get(i01)
            v.put(i10, b)
            v.put(i01, a)
        else:  # dense 2- / 3-qubit: all products, columns ascending (pass_dense2 / pass_dense3w)
            bits = [g["b0"], g["b1"]] + ([g["tpos_out"]] if kind == 4 else [])  # sub-index MSB first
            k = len(bits)
            pos = [tile_pos[b] for b in bits]
            sel = on.copy()
            for p in pos:
                sel &= ((idx >> p) & 1) == 0
            i0 = idx[sel]
            ids = [i0 | sum(((c >> (k - 1 - j)) & 1) << pos[j] for j in range(k)) for c in range(1 << k)]
            x = [v.get(i) for i in ids]
            mat = mats[16 * g["nz"]: 16 * g["nz"] + (1 << (2 * k))]
            for r in range(1 << k):
                acc = _cmul(v.number(mat[r << k]), x[0])
                for c in range(1, 1 << k):
                    acc = _cadd(acc, _cmul(v.number(mat[(r << k) + c]), x[c]))
                v.put(ids[r], acc)


def replay_absorbed(n, ops, x, dtype, mode=1):
    """the whole circuit: multi-gate steps from their "absorb" export (gates, then the flip), everything else by the oracle"""
    plan = debug_tile_plan(n, ops, mode | TILE_PLAN_ABSORB_X, dtype)
    st = x.copy()
    done = []
    for step in plan["steps"]:
        if "perm" in step:
            j = np.arange(1 << n, dtype=np.uint64)
            src = np.zeros_like(j)
            for dbit, sbit in enumerate(step["perm"]):
                src |= ((j >> np.uint64(dbit)) & np.uint64(1)) << np.uint64(sbit)
            st = st[src.astype(np.int64)]
        elif len(step["ops"]) == 1:
            st = O.apply_ops_in_place(n, [ops[step["ops"][0]]], st)
        else:
            a = step["absorb"]
            assert a["high"] == step["high"] and a["low"] == step["low"]  # the schedule's choice of positions stands
            tile_pos = a["low"] + a["high"]
            assert sorted(a["flip_pos"]) == sorted(tile_pos[b] for b in _bits(a["flip"]))
            assert len(a["passes"]) <= len(step["passes"]) and len(a["gates"]) + a["dropped"] == len(step["gates"])
            assert sum(ps["count"] for ps in a["passes"]) == len(a["gates"])
            v = _Vec(st)
            apply_gate_list(v, n, a)
            st = v.array(x.dtype)
            st = st[np.arange(1 << n, dtype=np.int64) ^ sum(1 << p for p in a["flip_pos"])]  # the store: out[t] = tile[t ^ flip]
        done += step["ops"]
    assert sorted(done) == list(range(len(ops)))
    return st, plan


def check(n, ops, dt, mode=1, seed=3):
    code, cdtype = DTYPES[dt]
    x = circuits.random_state(n, seed=seed).astype(cdtype)
    got, plan = replay_absorbed(n, ops, x, code, mode)
    want = O.apply_ops_in_place(n, ops, x.copy())
    assert got.dtype == want.dtype == cdtype
    assert np.array_equal(got, want)
    return plan


def multi(plan):
    return [s for s in plan["steps"] if "absorb" in s]


def is_x(g):
    return g["kind"] == 0 and g["b1"] & 2 and g["cmask"] == 0 and g["omask"] == 0


@pytest.mark.parametrize("dt", ["c64", "c32"])
@pytest.mark.parametrize("name", ["headline12", "headline16", "c2n13", "c2n15", "fuzz14", "batch15s0", "batch13s1", "batch14s2"])
def test_absorbed_form_replayed_equals_the_oracle(name, dt):
    n = int(name[5:7] if name.startswith("batch") else name[-2:])
    ops = {
        "headline12": lambda: circuits.c2_random_circuit(n, 256, seed=28, single_only=True),
        "headline16": lambda: circuits.c2_random_circuit(n, 256, seed=28, single_only=True),
        "c2n13": lambda: circuits.c2_random_circuit(n, 256, seed=28),
        "c2n15": lambda: circuits.h_layer(n) + circuits.c2_random_circuit(n, 200, seed=5),
        "fuzz14": lambda: fuzz_circuit(n, np.random.default_rng(14), 140),
        "batch15s0": lambda: seeded_default_batch(n, 0, 160)[0],
        "batch13s1": lambda: seeded_default_batch(n, 1, 160)[0],
        "batch14s2": lambda: seeded_default_batch(n, 2, 120)[0],
    }[name]()
    plan = check(n, ops, dt)
    steps = multi(plan)
    assert steps and sum(s["absorb"]["dropped"] for s in steps) > 0  # the rewrite really happened


def _m(n, bit, mat):
    return q.make_matrix_op([n - 1 - bit], mat)


def _c(n, cbits, op):
    return q.make_control_op([n - 1 - b for b in cbits], op)


RZ = [cmath.rect(1, -0.35), 0, 0, cmath.rect(1, 0.35)]
ZERO_ENTRY = [0.5 + 0.25j, 0, 0.3j, 0.8 - 0.1j]  # complex, with a zero entry (nz = 13 -> 14 after the column swap)
DENSE = [0.3 + 0.1j, -0.7j, 0.2, 0.9 - 0.4j]


def hand_cases(n):
    """name -> (ops, check of the one multi-gate step's absorbed form); every case is one segment (a Hadamard on another bit rides
    along where needed so that the step has >= 2 gates and something rounds)"""
    t = 8
    other = _m(n, 3, H)
    return {
        "x_x": ([_m(n, t, X), other, _m(n, t, X)],
                lambda a: a["flip"] == 0 and len(a["gates"]) == 1 and a["dropped"] == 2),
        "x_then_zero_entry_gate": ([_m(n, t, X), other, _m(n, t, ZERO_ENTRY)],
                                   lambda a: a["flip"] == 0 and len(a["gates"]) == 2 and sorted(g["nz"] for g in a["gates"]) == [14, 15]),
        "x_rz_h": ([_m(n, t, X), _m(n, t, RZ), _m(n, t, H), other],
                   lambda a: a["flip"] == 0 and a["dropped"] == 1 and not any(is_x(g) for g in a["gates"])),
        "x_then_control_on_it": ([_m(n, t, X), _c(n, [t], _m(n, 9, DENSE)), other],
                                 lambda a: a["flip"] == 0 and a["dropped"] == 0 and sum(1 for g in a["gates"] if is_x(g)) == 1),
        "x_then_controlled_dense_on_it": ([_m(n, t, X), _c(n, [2], _m(n, t, DENSE)), other],
                                          lambda a: a["flip"] == 0 and a["dropped"] == 0 and sum(1 for g in a["gates"] if is_x(g)) == 1),
        "x_then_controlled_phase_on_it": ([_m(n, t, X), _c(n, [2], _m(n, t, [1, 0, 0, 1j])), _m(n, 9, X), other],
                                          lambda a: a["dropped"] == 2 and sorted(a["flip_pos"]) == [t, 9]),
        "x_only": ([_m(n, 1, X), _m(n, 7, X), _m(n, 11, X), _m(n, 7, X), _m(n, 9, X)],
                   lambda a: a["gates"] == [] and a["passes"] == [] and sorted(a["flip_pos"]) == [1, 9, 11]),
        # a lane bit at load / store time (1), positions that are pass bits of the H gates' pass, and position 11 (tile bit 5 of a
        # Complex<f64> state, an ordinary high position of a Complex<f32> one below n = 13)
        "x_on_lane_pass_and_11": ([_m(n, 1, X), _m(n, 7, H), _m(n, 7, X), _m(n, 11, X), _m(n, 9, H),
                                   _m(n, 9, X), _m(n, 10, DENSE)],
                                  lambda a: sorted(a["flip_pos"]) == [1, 7, 9, 11] and len(a["gates"]) == 3),
        "x_then_swap_and_dense2": ([_m(n, t, X), _m(n, 6, X), q.make_swap_op([n - 1 - t], [n - 1 - 2]),
                                    q.make_matrix_op([n - 1 - 6, n - 1 - 7], np.kron(np.array(DENSE).reshape(2, 2), np.array(H).reshape(2, 2)).ravel()),
                                    other],
                                   lambda a: a["flip"] == 0 and a["dropped"] == 0),
    }


@pytest.mark.parametrize("dt", ["c64", "c32"])
@pytest.mark.parametrize("name", sorted(hand_cases(12)))
def test_hand_cases(name, dt):
    n = 12
    ops, ok = hand_cases(n)[name]
    plan = check(n, ops, dt)
    steps = multi(plan)
    assert len(plan["steps"]) == 1 and len(steps) == 1, [s["ops"] for s in plan["steps"]]
    assert ok(steps[0]["absorb"]), steps[0]["absorb"]


@pytest.mark.parametrize("dt", ["c64", "c32"])
def test_absorbed_passes_resolve_like_any_plan(dt):
    """the rewritten list goes through build_tile_segment like any other: the lane-level numpy model of k_tile_passes (dispatch
    codes, pass bits, lane assignment, diagonal runs; tests/test_tile_plan_cpu.py) accepts every absorbed segment and agrees with
    the plain replay of the gate list to rounding (that model multiplies in double precision)"""
    n = 13
    code, cdtype = DTYPES[dt]
    ops = circuits.c2_random_circuit(n, 200, seed=28)
    plan = debug_tile_plan(n, ops, 1 | TILE_PLAN_ABSORB_X, code)
    x = circuits.random_state(n, seed=9)
    for step in multi(plan):
        a = step["absorb"]
        lanes = x.copy()
        emulate_segment(lanes, n, a, use_interp=True)
        v = _Vec(x)
        apply_gate_list(v, n, a)
        assert np.max(np.abs(lanes - v.array(np.complex128))) <= 1e-13


def test_headline_sweeps_hold_no_x_and_177_gates():
    """the benchmark's circuit (30 qubits, 256 H / X / Rz gates, seed 28): 15 sweeps before and after, every X gone from the
    interpreter's lists, 79 of 256 gates with them, and no sweep with more passes than before"""
    ops = circuits.c2_random_circuit(30, 256, seed=28, single_only=True)
    plan = debug_tile_plan(30, ops, 1 | TILE_PLAN_ABSORB_X)
    steps = multi(plan)
    assert len(plan["steps"]) == len(steps) == 15
    assert sum(len(s["gates"]) for s in steps) == 256
    assert not any(is_x(g) for s in steps for g in s["absorb"]["gates"])
    assert sum(len(s["absorb"]["gates"]) for s in steps) == 177
    assert all(len(s["absorb"]["passes"]) <= len(s["passes"]) for s in steps)
    assert sum(len(s["absorb"]["passes"]) for s in steps) < sum(len(s["passes"]) for s in steps)


@pytest.mark.parametrize("dt", ["c64", "c32"])
def test_pass_count_never_rises(dt):
    code = DTYPES[dt][0]
    for n, ops in ((24, circuits.c2_random_circuit(24, 256, seed=28)), (30, circuits.c2_random_circuit(30, 256, seed=28)),
                   (26, circuits.c4_clifford_t(26, 256, seed=32)), (24, circuits.h_layer(24) + circuits.c5_grover_iteration(24)),
                   (22, seeded_default_batch(22, 0, 200)[0]), (14, fuzz_circuit(14, np.random.default_rng(14), 140))):
        for mode in (1, 2):
            for s in multi(debug_tile_plan(n, ops, mode | TILE_PLAN_ABSORB_X, code)):
                assert len(s["absorb"]["passes"]) <= len(s["passes"]), (n, mode, s["ops"])


# sha256 of the export's text for modes WITHOUT bit 4096, recorded from the build before the bit existed
EXPORT_CASES = {
    "headline30_m1": (30, lambda: circuits.c2_random_circuit(30, 256, seed=28, single_only=True), 1, "c64"),
    "c2n14_m1": (14, lambda: circuits.c2_random_circuit(14, 200, seed=28), 1, "c64"),
    "c2n14_m2": (14, lambda: circuits.c2_random_circuit(14, 200, seed=28), 2, "c64"),
    "c2n14_m1_interp": (14, lambda: circuits.c2_random_circuit(14, 200, seed=28), 1 | TILE_PLAN_INTERP, "c64"),
    "c2n14_m7": (14, lambda: circuits.c2_random_circuit(14, 200, seed=28), 7, "c64"),
    "qft13_m1_interp_c32": (13, lambda: circuits.c3_qft(13), 1 | TILE_PLAN_INTERP, "c32"),
    "batch13_m1_c32": (13, lambda: seeded_default_batch(13, 2, 120)[0], 1, "c32"),
    "c2n20_wide": (20, lambda: circuits.c2_random_circuit(20, 200, seed=28), 2 | 16, "c64"),
}
EXPORT_SHA256 = {
    "batch13_m1_c32": "f87b58385dad8cecacc6d917fc1f5ac6353d9eb91c24eaef49ae4b1c664e38e0",
    "c2n14_m1": "8d972ad8aa9f441cd3a96b7ac09ab7c37834eec374e112e65a44f41822b9cf47",
    "c2n14_m1_interp": "55e49d686deb108eac8fafee4cd15abd00edc1786d0f1d21af67dc8b496a3a24",
    "c2n14_m2": "2ae2425bd39dd0b780a9dd604b8729807045884f2f7811d792011678504abf88",
    "c2n14_m7": "2ae2425bd39dd0b780a9dd604b8729807045884f2f7811d792011678504abf88",
    "c2n20_wide": "b16c802c06e6d2dbd7869d24b81f5454b4ca4807a1f6ac2bc0cf7c84f52a5843",
    "headline30_m1": "8a8e6c7f06dff05b3a3e7616d0b457e8be9e81fc903551777321d268a3d77443",
    "qft13_m1_interp_c32": "603e8c3221e13eef187b03326a4b4be777626e5f9d2937ed8babf904087c8738",
}


def export_text(name, extra_mode=0):
    n, make, mode, dt = EXPORT_CASES[name]
    code = DTYPES[dt][0]
    cops = [op.to_c(code) for op in make()]
    arr = (_ffi.QipOp * len(cops))(*cops)
    txt = _ffi.lib.qip_hip_debug_tile_plan(code, n, arr, len(cops), mode | extra_mode)
    assert txt
    return txt if isinstance(txt, bytes) else txt.encode()


@pytest.mark.parametrize("name", sorted(EXPORT_CASES))
def test_modes_without_the_bit_export_what_they_did(name):
    assert hashlib.sha256(export_text(name)).hexdigest() == EXPORT_SHA256[name]
    if name != "c2n20_wide":  # (and with the bit something is really added)
        assert b'"absorb"' in export_text(name, TILE_PLAN_ABSORB_X) and b'"absorb"' not in export_text(name)
