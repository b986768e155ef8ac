"""The interpreter's gate loop (k_tile_passes) keeps a lane's eight amplitudes in registers from gate to gate.  What can go wrong
there is an amplitude that a gate did NOT touch arriving wrong at the next gate or at the pass's write-back, so these lists switch
kind at every entry and are full of partial updates: gates that rewrite half, a quarter or one of the eight elements, gates whole
lanes or whole blocks skip, exchanges, and second and third passes (write-back and reload between kinds).  Every list must give,
bit for bit, what one launch per gate gives from the same seeded product state.  The premise - which code path of the kernel each
list reaches - is checked on the host (no GPU) from the lists the kernel is really handed."""
import cmath
import math

import numpy as np
import pytest

import rustqip_amd as q
from oracle import window_parity as W
from rustqip_amd import _ffi, circuits
from rustqip_amd.ops import TILE_PLAN_ABSORB_X, TILE_PLAN_INTERP, TILE_SIGN_ROWS, debug_tile_plan

# TileOp (csrc/qip_kernels.h), as exported in the "op" of a gate
DIAG_UNIFORM, DIAG_LANE, DIAG_LANE_CTL, DIAG_REG, DENSE, DENSE_LANE, DENSE2Q, SWAP, DENSE3Q = 0, 1, 2, (3, 4, 5), (6, 7, 8), (9, 10, 11), range(12, 18), (18, 19, 20), range(21, 27)

RY = [math.cos(0.15), -math.sin(0.15), math.sin(0.15), math.cos(0.15)]   # generic real entries
RX = [math.cos(0.2), -1j * math.sin(0.2), -1j * math.sin(0.2), math.cos(0.2)]  # complex entries
UPPER = [1, 0.5, 0, 1]                                                    # a zero entry (the zero-skipping rows)


def _dt(dtype):
    return _ffi.QIP_C64 if dtype == np.complex128 else _ffi.QIP_C32


def _lists(n):
    """{name: ops}.  Positions are amplitude-index bits (qubit n - 1 - p).  A, B, C: the dense targets of the first pass (its three
    pass bits, indices J = 0, 1, 2); L0, L1: tile bits that no gate exchanges across (lane bits); D, E, F, G: targets that open the
    second and third pass; OUT: a position that is not among the tile's eleven."""
    A, B, C, L0, L1, D, E, F, G, OUT = 1, 3, 7, 0, 2, 4, 8, 9, 10, 6 if n <= 14 else n - 1

    def m(p, mat):
        return q.make_matrix_op([n - 1 - p], mat)

    def ctl(cs, op):
        return q.make_control_op([n - 1 - c for c in cs], op)

    def ph(t):
        return [1, 0, 0, cmath.rect(1, t)]

    rng = np.random.default_rng(5)
    u2 = np.linalg.qr(rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4)))[0]
    u3 = np.linalg.qr(rng.standard_normal((8, 8)) + 1j * rng.standard_normal((8, 8)))[0]
    H, X, rz = circuits.H, circuits.X, circuits.rz
    run9 = [m(p, rz(0.1 + 0.07 * i)) if i % 2 else m(p, ph(0.3 + 0.05 * i)) for i, p in enumerate([OUT, L0, A, L1, B, OUT, C, L0, A])]
    one_pass = [
        m(A, H), m(OUT, rz(0.31)),                      # sign rows J = 0 | one wave-uniform factor
        m(B, X), m(B, H), m(L0, rz(0.52)),              # H.X on J = 1 | per-lane factor
        m(C, H), m(A, rz(0.23)),                        # J = 2 | factor by pass bit
        m(B, RY), m(L1, ph(0.4)), m(OUT, ph(0.9)),      # generic real | run of 2
        m(C, RX), ctl([A], m(L0, ph(0.7))),             # complex | controlled phase: 4 of 8 elements
        m(A, UPPER), ctl([A], m(B, ph(0.6))),           # zero entry | 2 of 8
        m(A, X), m(A, H), ctl([A, B], m(C, ph(1.1))),   # H.X on J = 0 | 1 of 8
        ctl([A], m(B, X)), m(L0, rz(0.2)), m(A, rz(0.3)), m(OUT, rz(0.4)),   # CNOT, control on a pass bit: half the pairs | run of 3
        ctl([B], m(C, H)), m(L1, rz(0.11)),             # controlled H, control on a pass bit
        ctl([L0], m(A, X)), m(OUT, rz(0.21)),           # control on a lane bit
        ctl([L1], m(B, H)), ctl([L1], m(L0, ph(0.45))),   # | lane-bit control folded into the factor
        m(C, X), m(C, H), m(C, rz(0.12)),               # H.X on J = 2
        ctl([OUT], m(C, X)), m(L0, ph(0.33)),           # control outside the tile: whole blocks skip
        ctl([OUT], m(A, H)), *run9,                     # | run of 9
        m(B, H), q.make_swap_op([n - 1 - A], [n - 1 - C]), m(L1, rz(0.6)),   # swap of two pass bits
        m(C, H), m(L0, X),                              # a trailing X: the store flips the bit
    ]
    passes = [  # dense targets on seven positions: three passes, a diagonal or partial update next to every boundary
        m(A, H), m(OUT, rz(0.3)), m(B, RY), ctl([A], m(C, ph(0.5))), m(C, H), m(L0, rz(0.7)),
        m(D, H), ctl([C], m(D, X)), m(E, RX), m(A, rz(0.2)), m(L1, ph(0.3)), m(F, H), m(F, X), ctl([D, E], m(F, ph(0.8))),
        m(G, H), m(OUT, rz(0.9)), m(A, UPPER), ctl([G], m(A, H)), m(B, H), m(D, rz(0.4)), m(G, X),
    ]
    dense23 = [  # dense 2- and 3-qubit items between one-element updates
        m(A, H), ctl([A, B], m(C, ph(0.4))), q.make_matrix_op([n - 1 - A, n - 1 - C], u2.ravel()), m(L0, rz(0.3)),
        m(B, H), m(B, X), q.make_matrix_op([n - 1 - C, n - 1 - A, n - 1 - B], u3.ravel()), ctl([B], m(A, ph(0.2))), m(C, RY), m(OUT, rz(0.8)),
        q.make_swap_op([n - 1 - A], [n - 1 - B]), m(C, H), m(A, X),
    ]
    return {"one_pass": one_pass, "passes": passes, "dense23": dense23}


def _paths(n, ops, dtype):
    """what the interpreter is handed for `ops` (host only): the gates of its lists in order, the passes and the store's flip"""
    plan = debug_tile_plan(n, ops, 1 | TILE_PLAN_ABSORB_X | TILE_PLAN_INTERP, _dt(dtype))
    gates, npasses, flip = [], 0, 0
    for st in plan["steps"]:
        if "absorb" in st:
            gates += st["absorb"]["gates"]
            npasses += len(st["absorb"]["passes"])
            flip |= st["absorb"]["flip"]
    return gates, npasses, flip


def _diag_run_lengths(gates):
    runs, k = [], 0
    for g in gates + [{"kind": 0}]:
        if g["kind"] in (1, 5):
            k += 1
        else:
            runs.append(k)
            k = 0
    return {r for r in runs if r}


@pytest.mark.parametrize("dtype", [np.complex128, np.complex64], ids=["c64", "c32"])
@pytest.mark.parametrize("n", [12, 14, 22])
def test_premise_the_lists_reach_every_path_of_the_gate_loop(n, dtype):
    lists = _lists(n)
    gates, npasses, flip = _paths(n, lists["one_pass"], dtype)
    codes = {g["op"] for g in gates}
    assert npasses == 1 and flip != 0, (npasses, flip)  # one pass: no write-back between the kinds; a trailing X in the store
    assert {DIAG_UNIFORM, DIAG_LANE, DIAG_LANE_CTL, *DIAG_REG, *DENSE, *DENSE_LANE[:2]} <= codes and codes & set(SWAP), sorted(codes)
    signs = {(g["op"] - DENSE[0], g["b1"] >> 3) for g in gates if g["op"] in DENSE and g["kind"] == 0 and g["b1"] & TILE_SIGN_ROWS}
    assert {j for j, _ in signs} == {0, 1, 2} and {s for _, s in signs} == {1, 2}, signs  # H and H.X, each pass-bit index
    assert any(g["op"] in DENSE and g["b1"] & 2 and g["cm_reg"] for g in gates), "CNOT with its control on a pass bit"
    assert any(g["op"] in DENSE and g["nz"] != 15 and not g["b1"] & 2 for g in gates), "zero entry"
    assert any(g["op"] in DENSE and g["omask"] for g in gates), "control outside the tile"
    assert {1, 2, 3, 9} <= _diag_run_lengths(gates), _diag_run_lengths(gates)  # single gates and runs of 2, 3 and 9
    # controlled phases, alone between dense gates, over 4, 2 and 1 of the lane's eight elements
    alone = [g for a, g, b in zip(gates, gates[1:], gates[2:]) if g["kind"] == 1 and a["kind"] != 1 and b["kind"] != 1]
    assert {4, 2, 1} <= {8 >> (bin(g["cm_reg"]).count("1") + (g["op"] in DIAG_REG)) for g in alone}
    gates, npasses, flip = _paths(n, lists["passes"], dtype)
    assert npasses >= 3 and flip != 0, (npasses, flip)
    gates, npasses, flip = _paths(n, lists["dense23"], dtype)
    codes = {g["op"] for g in gates}
    assert codes & set(DENSE2Q) and codes & set(DENSE3Q) and codes & set(SWAP) and flip != 0, (sorted(codes), flip)


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
@pytest.mark.parametrize("name", ["one_pass", "passes", "dense23"])
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64], ids=["c64", "c32"])
@pytest.mark.parametrize("n", [12, 14])
def test_interpreter_sweeps_are_bit_equal_to_one_launch_per_gate(n, dtype, name):
    ops = _lists(n)[name]
    got, prof = _run(n, dtype, ops, tile=1, tile_jit=0, tile_auto=0)
    # (one launch per gate; below n = 17 a dense 3-qubit gate launched alone would run on matrix cores, an fma chain: mfma = 0
    # makes it the unfused fold that a sweep, the VALU kernel and the oracle share)
    want, _ = _run(n, dtype, ops, tile=0, pair_floor=0, mfma=0)
    assert prof.get("k_tile_passes", {}).get("launches", 0) >= 1, prof  # the interpreter really ran
    assert np.array_equal(got, want), f"n={n} {np.dtype(dtype).name} {name}: {_why(got, want)}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one_pass", "passes"])
def test_default_path_sweeps_are_bit_equal_to_one_launch_per_gate(name):
    n = 22
    ops = _lists(n)[name]
    got, prof = _run(n, np.complex128, ops, pair_floor=1)
    want, _ = _run(n, np.complex128, ops, tile=0, pair_floor=0)
    assert prof.get("k_tile_passes", {}).get("launches", 0) >= 1, prof
    assert np.array_equal(got, want), f"n={n} {name}: {_why(got, want)}"
