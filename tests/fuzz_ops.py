"""Seeded random circuits shared by the tile scheduler's CPU replay (tests/test_tile_plan_cpu.py) and the default path's fused
sweeps on the GPU (tests/test_gpu_default_fusion_kinds.py).  A plain helper module, no fixtures.

Positions below are amplitude-index BITS; qubit q of make_matrix_op / make_control_op is bit n - 1 - q (`_q`)."""
import cmath
import math

import numpy as np

import rustqip_amd as q


def rand_unitary(k, rng):
    a = rng.standard_normal((1 << k, 1 << k)) + 1j * rng.standard_normal((1 << k, 1 << k))
    u, _ = np.linalg.qr(a)
    return u


def fuzz_circuit(n, rng, gates):
    s2 = 0.5 ** 0.5
    g1 = [[0, 1, 1, 0], [0, -1j, 1j, 0], [1, 0, 0, -1], [s2, s2, s2, -s2], [1, 0, 0, 1j], [1, 0, 0, cmath.rect(1, 0.785)],
          [cmath.rect(1, -0.35), 0, 0, cmath.rect(1, 0.35)], [1, 1, 0, 1], [0.3 + 0.1j, -0.7j, 0.2, 0.9 - 0.4j]]
    ops = []
    for _ in range(gates):
        perm = [int(v) for v in rng.permutation(n)]
        shape = int(rng.integers(0, 9))
        nc = int(rng.integers(0, 5))
        if shape <= 3:
            g = q.make_matrix_op([perm[0]], g1[int(rng.integers(0, len(g1)))])
            ops.append(q.make_control_op(perm[1:1 + nc], g) if nc and rng.integers(0, 2) else g)
        elif shape == 4:
            g = q.make_matrix_op([perm[0]], [1, 0, 0, cmath.rect(1, float(rng.uniform(0, 6.28)))])
            ops.append(q.make_control_op(perm[1:2 + nc], g))
        elif shape == 5:
            g = q.make_swap_op([perm[0]], [perm[1]])
            ops.append(q.make_control_op(perm[2:2 + nc], g) if nc else g)
        elif shape == 6:
            g = q.make_matrix_op(perm[:2], rand_unitary(2, rng).ravel())
            ops.append(q.make_control_op(perm[2:2 + min(nc, 3)], g) if nc else g)
        elif shape == 7:
            g = q.make_matrix_op(perm[:3], rand_unitary(3, rng).ravel())  # a pass of its own three bits
            ops.append(q.make_control_op(perm[3:3 + min(nc, 3)], g) if nc and rng.integers(0, 2) else g)
        else:
            ops.append(q.make_swap_op(perm[:2], perm[2:4]))  # not tileable
    return ops


# ---- the default path's palette: every tile item kind of classify_tile_item (qip_tile_sched.hip), with and without controls,
# biased toward the bits where tile addressing changes ----------------------------------------------------------------------

S2 = math.sqrt(0.5)
EXACT_1Q = {"X": [0, 1, 1, 0], "Y": [0, -1j, 1j, 0]}  # kind 0, rounding-free: mode 1 moves them past other gates
EXACT_DIAG = {"Z": [1, 0, 0, -1], "S": [1, 0, 0, 1j]}  # kind 1, rounding-free
ROUNDED_1Q = {
    "H": [S2, S2, S2, -S2],
    "upper": [1, 1, 0, 1],           # a zero entry (the interpreter's zero-skipping shapes)
    "rank1": [0.5, 0.25j, 0, 0],     # a zero row
    "real": [0.6, -0.8, 0.8, 0.6],   # a real matrix (the interpreter's `real` shortcut)
    "dense": [0.3 + 0.1j, -0.7j, 0.2, 0.9 - 0.4j],
}
ROUNDED_DIAG = {"T": [1, 0, 0, cmath.rect(1, math.pi / 4)], "Rz": [cmath.rect(1, -0.35), 0, 0, cmath.rect(1, 0.35)]}
IDENT = [1, 0, 0, 1]


def edge_bits(n):
    """where tile addressing changes: the row's low bits 0 / 4 / 5 / 6, tile_p5's 11 (Complex<f64>) and its neighbours, the top"""
    return sorted({0, 4, 5, 6, 10, 11, 12} | set(range(n - 6, n)))


def _q(n, bits):
    return [n - 1 - b for b in bits]


class _Picker:
    def __init__(self, n, rng):
        self.n, self.rng, self.edges = n, rng, edge_bits(n)

    def bits(self, k, taken=(), below6=None):
        """k distinct bits not in `taken`, each an edge bit with probability 0.6; below6 = at most this many below bit 6"""
        out = []
        low = sum(1 for b in taken if b < 6)
        while len(out) < k:
            b = int(self.rng.choice(self.edges)) if self.rng.random() < 0.6 else int(self.rng.integers(0, self.n))
            if b in out or b in taken or (below6 is not None and b < 6 and low >= below6):
                continue
            low += b < 6
            out.append(b)
        return out

    def n_controls(self, room):
        r = self.rng.random()
        nc = 0 if r < 0.4 else 1 if r < 0.7 else 2 if r < 0.85 else 3
        if self.rng.random() < 0.06:  # now and then more than n - 17: past a dense gate's one-op sweep threshold
            nc = self.n - 17 + int(self.rng.integers(1, 4))
        return max(0, min(nc, room))


def fuzz_default_batch(n, rng, gates, dense3_low=False, dense4=False):
    """`gates` ops for the default apply_ops path and, per op, its tag (kind, controls, bits touched): the tile item kind 0-4,
    "noop" for an identity (launches nothing), None for an op the tile cannot take.

    dense3_low = False: a dense 3-qubit gate has at most one target below bit 6, so launched alone it never takes launch_kq's
    matrix-core form — every op of the batch then runs alone as the unfused fold the oracle computes (bit-equal to it).
    dense3_low = True lets two or three targets sit below bit 6; dense4 adds dense 4-qubit gates (matrix cores, a 1e-12 bar).
    About 4 % of the ops are untileable breakers: Swap(2), a sparse op, dense 4-qubit (dense4)."""
    pk = _Picker(n, rng)
    ops, tags = [], []

    def add(op, kind, ctl, bits):
        ops.append(op)
        tags.append((kind, len(ctl), frozenset(bits)))

    def ctrl(op, tb, cb):
        return q.make_control_op(_q(n, cb), op) if cb else op

    for _ in range(gates):
        r = rng.random()
        if r < 0.30:  # exact single-qubit: X / Y (kind 0) or Z / S (kind 1), CNOT, Toffoli, CZ, CS
            name, m = list({**EXACT_1Q, **EXACT_DIAG}.items())[int(rng.integers(0, 4))]
            tb = pk.bits(1)
            cb = pk.bits(pk.n_controls(n - 1), tb)
            add(ctrl(q.make_matrix_op(_q(n, tb), m), tb, cb), 0 if name in EXACT_1Q else 1, cb, tb + cb)
        elif r < 0.52:  # rounded single-qubit: H, zero-entry, real, dense (kind 0) or T / Rz (kind 1), plain or controlled
            pool = {**ROUNDED_1Q, **ROUNDED_DIAG}
            name = list(pool)[int(rng.integers(0, len(pool)))]
            tb = pk.bits(1)
            cb = pk.bits(pk.n_controls(n - 1), tb)
            add(ctrl(q.make_matrix_op(_q(n, tb), pool[name]), tb, cb), 1 if name in ROUNDED_DIAG else 0, cb, tb + cb)
        elif r < 0.60:  # controlled phase of a random angle (kind 1)
            tb = pk.bits(1)
            cb = pk.bits(max(1, pk.n_controls(n - 1)), tb)
            add(ctrl(q.make_matrix_op(_q(n, tb), [1, 0, 0, cmath.rect(1, float(rng.uniform(0, 6.28)))]), tb, cb), 1, cb, tb + cb)
        elif r < 0.63:  # identity, plain or controlled: launches nothing
            tb = pk.bits(1)
            cb = pk.bits(pk.n_controls(n - 1), tb)
            add(ctrl(q.make_matrix_op(_q(n, tb), IDENT), tb, cb), "noop", cb, tb + cb)
        elif r < 0.71:  # Swap(1), plain or controlled (kind 2, exact)
            tb = pk.bits(2)
            cb = pk.bits(pk.n_controls(n - 2), tb)
            add(ctrl(q.make_swap_op(_q(n, tb[:1]), _q(n, tb[1:])), tb, cb), 2, cb, tb + cb)
        elif r < 0.82:  # dense 2-qubit (kind 3): complex unitary, real orthogonal, or with zero entries
            tb = pk.bits(2)
            cb = pk.bits(pk.n_controls(n - 2), tb)
            shape = int(rng.integers(0, 3))
            if shape == 0:
                m = rand_unitary(2, rng)
            elif shape == 1:
                m = np.linalg.qr(rng.standard_normal((4, 4)))[0].astype(complex)
            else:
                m = np.kron(np.array(ROUNDED_1Q["upper"], dtype=complex).reshape(2, 2), np.array(ROUNDED_1Q["H"], dtype=complex).reshape(2, 2))
            add(ctrl(q.make_matrix_op(_q(n, tb), m.ravel()), tb, cb), 3, cb, tb + cb)
        elif r < 0.96:  # dense 3-qubit (kind 4)
            tb = pk.bits(3, below6=None if dense3_low else 1)
            cb = pk.bits(pk.n_controls(n - 3), tb)
            m = rand_unitary(3, rng) if rng.random() < 0.7 else np.linalg.qr(rng.standard_normal((8, 8)))[0].astype(complex)
            add(ctrl(q.make_matrix_op(_q(n, tb), m.ravel()), tb, cb), 4, cb, tb + cb)
        else:  # breakers the tile cannot take
            shape = int(rng.integers(0, 3 if dense4 else 2))
            if shape == 0:
                tb = pk.bits(4)
                add(q.make_swap_op(_q(n, tb[:2]), _q(n, tb[2:])), None, (), tb)
            elif shape == 1:
                tb = pk.bits(3)
                rows = [[((r_ * 3 + 1) % 8, 0.6j), (r_, 0.8)] for r_ in range(8)]
                add(q.make_sparse_matrix_op(_q(n, tb), rows), None, (), tb)
            else:
                tb = pk.bits(4)
                add(q.make_matrix_op(_q(n, tb), rand_unitary(4, rng).ravel()), None, (), tb)
    return ops, tags


def fused_coverage(plan, tags):
    """what the multi-gate steps of a plan (plan_tiles' list of steps) held: {(kind, controlled)} and {(kind, bit)}"""
    kinds, at = set(), set()
    for step in plan:
        if len(step) < 2:
            continue
        for i in step:
            kind, ctl, bits = tags[i]
            if not isinstance(kind, int):
                continue
            kinds.add((kind, ctl > 0))
            at |= {(kind, b) for b in bits}
    return kinds, at


FUZZ_SEEDS = (0, 1, 2)  # seed 2 is the mixed palette: dense 3-qubit gates with targets below bit 6, dense 4-qubit breakers


def seeded_default_batch(n, seed, gates=200):
    mixed = seed == 2
    return fuzz_default_batch(n, np.random.default_rng(1000 * n + seed), gates, dense3_low=mixed, dense4=mixed)


def dense3_in_a_multi_gate_step(plan, index):
    return any(index in step and len(step) >= 2 for step in plan)


SINGLE_VIA_TILE_DEFAULT = 3  # the library's default of global option single_via_tile


def dense3_case(name, n, rng):
    """A dense 3-qubit gate on bits 0, 1, 2 between H gates, which mode 1 plans as ONE multi-gate step.  Launched alone it
    takes launch_kq's matrix-core form unless it takes the one-op tile sweep, which needs single_via_tile > 0 and
    n >= 17 + controls.  Returns (ops, index of the dense gate, single_via_tile to set, runs on matrix cores alone)."""
    u3 = q.make_matrix_op(_q(n, [0, 1, 2]), rand_unitary(3, rng).ravel())
    h = lambda b: q.make_matrix_op(_q(n, [b]), ROUNDED_1Q["H"])  # noqa: E731
    if name == "single_via_tile_0":
        return [h(7), u3, h(8)], 1, 0, True
    nc = {"five_controls": 5, "six_controls": 6, "seven_controls": 7}[name]
    cu = q.make_control_op(_q(n, range(12, 12 + nc)), u3)
    return [h(7), h(8), cu, h(9)], 2, SINGLE_VIA_TILE_DEFAULT, n < 17 + nc


DENSE3_CASES = [("six_controls", 22), ("seven_controls", 23), ("single_via_tile_0", 22), ("five_controls", 22)]


def unit_phase_case(n, rng):
    """S and Y gates (exact: a unit phase) after a dense 4-qubit gate on other bits: mode 1 moves them past it into the step of
    the H gates in front.  Launched alone the dense gate runs on matrix cores, whose three-product form does not commute
    exactly with a factor i.  Returns (ops, index of the dense gate)."""
    h = lambda b: q.make_matrix_op(_q(n, [b]), ROUNDED_1Q["H"])  # noqa: E731
    u4 = q.make_matrix_op(_q(n, [6, 8, 10, 12]), rand_unitary(4, rng).ravel())
    return [h(4), h(13), u4, q.make_matrix_op(_q(n, [4]), EXACT_DIAG["S"]), q.make_matrix_op(_q(n, [13]), EXACT_1Q["Y"])], 2
