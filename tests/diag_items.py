"""Circuits with diagonal Matrix ops on two and three qubits — the tile item kind TILE_KIND_DIAG_K — shared by
tests/test_tile_diag_items_cpu.py and tests/test_gpu_tile_diag_items.py.  A plain helper module, no fixtures.

Positions are amplitude-index BITS; qubit q of make_matrix_op / make_control_op is bit n - 1 - q.  An op's FIRST index is the
most significant bit of its sub-index, so diag_op(n, [a, b], d) multiplies the amplitudes whose bits (a, b) read (1, 0) by d[2]."""
import cmath
import math

import numpy as np

import rustqip_amd as q
from rustqip_amd import circuits

S2 = math.sqrt(0.5)
H = [S2, S2, S2, -S2]
X = [0, 1, 1, 0]
T = [1, 0, 0, cmath.rect(1, math.pi / 4)]


def _q(n, bits):
    return [n - 1 - b for b in bits]


def gate1(n, bit, m):
    return q.make_matrix_op(_q(n, [bit]), m)


def rz(gamma):
    return [cmath.exp(-1j * gamma), 0, 0, cmath.exp(1j * gamma)]


def rx(theta):
    c, s = math.cos(theta / 2), math.sin(theta / 2)
    return [c, -1j * s, -1j * s, c]


def zz(gamma):
    """the ZZ phase of QAOA / Ising circuits"""
    return [cmath.exp(-1j * gamma), cmath.exp(1j * gamma), cmath.exp(1j * gamma), cmath.exp(-1j * gamma)]


def diag_op(n, bits, entries, controls=()):
    op = q.make_matrix_op(_q(n, bits), np.diag(np.asarray(entries, dtype=complex)).ravel())
    return q.make_control_op(_q(n, controls), op) if controls else op


def stand_in(n, bits, entries, controls=()):
    """a 1-qubit diagonal on the item's LAST op bit, controlled by its other op bits and its own controls: the same footprint,
    and the same exactness class (Z where every entry is one of +-1, +-i, a rounded Rz otherwise)"""
    exact = all(e in (1, -1, 1j, -1j) for e in (complex(v) for v in entries))
    g = gate1(n, bits[-1], [1, 0, 0, -1] if exact else rz(0.3))
    return q.make_control_op(_q(n, list(controls) + list(bits[:-1])), g)


def five_op_cases(n=22, phi=0.7, gamma=0.3):
    """name -> (bits, entries, controls) of D in [H(3), H(9), D, H(3), H(9)]"""
    return {
        "zz": ([3, 9], zz(gamma), ()),
        "cz_4x4": ([3, 9], [1, 1, 1, -1], ()),
        "phase_on_01": ([3, 9], [1, cmath.exp(1j * phi), 1, 1], ()),
        "diag8": ([3, 9, 15], [cmath.exp(0.1j * (k + 1)) for k in range(8)], ()),
        "controlled_zz": ([3, 9], zz(gamma), (12,)),
    }


def five_ops(n, case, as_stand_in=False):
    bits, entries, controls = case
    d = (stand_in if as_stand_in else diag_op)(n, bits, entries, controls)
    return [gate1(n, 3, H), gate1(n, 9, H), d, gate1(n, 3, H), gate1(n, 9, H)]


def qaoa(n, layers=2, spelling="diag"):
    """rustqip_amd.circuits.qaoa_ring: `layers` of (a ring of n ZZ phases, n Rx gates); spelling "diag", "cnot" or "stand_in" (see there)"""
    return circuits.qaoa_ring(n, layers, spelling)


# ---- seeded mixes: H / Rz / T / CNOT / X with diagonal items on lane bits, pass bits and outside the tile -------------------------

BIT_CLASSES = {"row": (0, 3, 5), "tile": (6, 8, 10), "high": (14, -1)}  # (-1 = n - 1)


def _entries(k, shape, rng):
    """a 2^k table.  shape: "full" = no unit entry, "some" = unit and non-unit entries, "exact" = entries of +-1, +-i with a unit
    among them, "phase0" = ONE non-unit entry at a sub-index with a zero bit (KC_PHASE, not the all-ones pattern)"""
    side = 1 << k
    if shape == "full":
        return [cmath.exp(1j * float(rng.uniform(0.1, 3.0))) for _ in range(side)]
    if shape == "some":
        d = [cmath.exp(1j * float(rng.uniform(0.1, 3.0))) if rng.random() < 0.5 else 1 for _ in range(side)]
        d[0], d[-1] = cmath.exp(0.37j), 1  # at least one of each, and never the all-ones phase pattern
        return d
    if shape == "exact":
        d = [[1, -1, 1j, -1j][int(rng.integers(0, 4))] for _ in range(side)]
        d[0], d[1] = -1, 1
        return d
    d = [1] * side
    d[int(rng.integers(0, side - 1))] = cmath.exp(1j * float(rng.uniform(0.1, 3.0)))
    return d


def _pools(n):
    return {name: [b % n for b in bits] for name, bits in BIT_CLASSES.items()}


def random_item(n, rng):
    """(op, its stand-in, tag): a diagonal item with k = 2 / 3 op bits and 0 - 2 controls, every bit drawn from BIT_CLASSES.
    tag = (k, controlled, frozenset of the bit classes its op bits and controls sit on, shape of the table)"""
    pools = _pools(n)
    every = sorted({b for bits in pools.values() for b in bits})
    k = 2 + int(rng.integers(0, 2))
    nc = int(rng.integers(0, 2)) * (1 + int(rng.integers(0, 2)))  # 0, 1 or 2 controls
    cls = list(pools)[int(rng.integers(0, 3))]  # the class the item visits for sure; the rest is drawn from all the positions
    first = int(rng.choice(pools[cls]))
    rest = [int(b) for b in rng.permutation([b for b in every if b != first])][: k + nc - 1]
    bits = [int(b) for b in rng.permutation([first] + rest[: k - 1])]
    controls = rest[k - 1:]
    shape = ["full", "some", "exact", "phase0"][int(rng.integers(0, 4))]
    entries = _entries(k, shape, rng)
    where = frozenset(name for name, p in pools.items() if set(p) & set(bits + controls))
    return diag_op(n, bits, entries, controls), stand_in(n, bits, entries, controls), (k, nc > 0, where, shape)


def seeded_mix(n, seed, gates=60, item_share=0.3):
    """(ops, the same circuit with every diagonal item replaced by its stand-in, tags): H / Rz / T / CNOT / X with diagonal items.
    tags[i] = None for the existing kinds, random_item's tag for a diagonal item."""
    rng = np.random.default_rng(9000 + 100 * n + seed)
    every = sorted({b for bits in _pools(n).values() for b in bits})
    ops, subs, tags = [], [], []

    def both(op, tag=None, sub=None):
        ops.append(op)
        subs.append(op if sub is None else sub)
        tags.append(tag)

    for _ in range(gates):
        r = rng.random()
        if r < item_share:
            op, sub, tag = random_item(n, rng)
            both(op, tag, sub)
        elif r < item_share + 0.25:
            both(gate1(n, int(rng.integers(0, n)), H))
        elif r < item_share + 0.40:
            both(gate1(n, int(rng.choice(every)), rz(float(rng.uniform(0.1, 1.0)))))
        elif r < item_share + 0.48:
            both(gate1(n, int(rng.choice(every)), T))
        elif r < item_share + 0.60:
            both(gate1(n, int(rng.choice(every)), X))
        else:
            c, t = (int(b) for b in rng.permutation(n)[:2])
            both(q.make_control_op(_q(n, [c]), gate1(n, t, X)))
    return ops, subs, tags


def seeded_default_mix(n, seed, gates=60, item_share=0.35):
    """(ops, tags) for the default apply_ops path: the palette of every existing tile item kind (fuzz_ops.fuzz_default_batch, dense
    3-qubit gates with at most one target below bit 6: launched alone every op is the oracle's fold) with diagonal items between"""
    from fuzz_ops import fuzz_default_batch

    rng = np.random.default_rng(7000 + 100 * n + seed)
    n_items = int(round(gates * item_share))
    old, _ = fuzz_default_batch(n, rng, gates - n_items)
    slots = set(int(v) for v in rng.choice(gates, size=n_items, replace=False))
    ops, tags = [], []
    old = iter(old)
    for i in range(gates):
        if i in slots:
            op, _, tag = random_item(n, rng)
            ops.append(op)
            tags.append(tag)
        else:
            ops.append(next(old))
            tags.append(None)
    return ops, tags


def item_coverage(plan, tags):
    """{(bit class, k, controlled)} of the diagonal items that sit in multi-gate steps of a plan (plan_tiles' list of steps)"""
    seen = set()
    for step in plan:
        if len(step) < 2:
            continue
        for i in step:
            if tags[i] is not None:
                k, ctl, where, _ = tags[i]
                seen |= {(cls, k, ctl) for cls in where}
    return seen


ALL_COMBINATIONS = {(cls, k, ctl) for cls in BIT_CLASSES for k in (2, 3) for ctl in (False, True)}


def apply_dense(n, ops, x):
    """the circuit as a product of dense matrices applied to x, in numpy and Complex<f64>: every op (a Matrix, or Controls around
    one) is written out as the 2^m x 2^m matrix on all its qubits and contracted with the state tensor (axis i = qubit i)"""
    psi = np.asarray(x, dtype=np.complex128).reshape((2,) * n)
    for op in ops:
        controls, inner = [], op
        while inner.kind == "Control":
            controls += list(inner.indices[: inner.n_controls])
            inner = inner.inner
        assert inner.kind == "Matrix"
        k = len(inner.indices)
        qubits = controls + list(inner.indices)
        m = len(qubits)
        full = np.eye(1 << m, dtype=np.complex128)
        full[(1 << m) - (1 << k):, (1 << m) - (1 << k):] = np.asarray(inner.data, dtype=np.complex128).reshape(1 << k, 1 << k)
        psi = np.tensordot(full.reshape((2,) * (2 * m)), psi, axes=(list(range(m, 2 * m)), qubits))
        psi = np.moveaxis(psi, list(range(m)), qubits)
    return np.ascontiguousarray(psi).reshape(-1)
