"""An exact reference for measurement on a device state, and the cases the measurement tests run — shared by
tests/test_measure_ref_cpu.py and tests/test_gpu_f1_measure_paths.py.  A plain helper module: numpy only, no fixtures.

The device forms |amp|^2 = re*re + im*im in the state's own precision, without contraction, and accumulates in double.  The
oracle sums `P` values one after the other in `P`, as the reference does, so for Complex<f32> it is far from the true sum
(5.8e-4 at n = 23, k = 1).  Here the same products are widened to np.longdouble (64-bit mantissa on x86) and summed per
outcome, rounded to float64 once: one bar, 1e-13, then serves both precisions.

Qubit q is amplitude-index bit n - 1 - q (`position`); bit i of an outcome is the bit of qubit indices[i]."""
import numpy as np

PIECE = 1 << 22  # amplitudes per piece when a large state is reduced piecewise


def make_state(n, seed, dtype=np.complex128, zero_every=5, norm=1.0):
    """random state with every `zero_every`-th amplitude zero (the reference skips zeros), scaled to norm^2 = `norm`"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    v[::zero_every] = 0
    v *= np.sqrt(norm) / np.linalg.norm(v)
    return v.astype(dtype)


def products(x):
    """re*re + im*im of every amplitude, formed in the precision of `x` (two roundings of the products, one of the sum),
    widened to longdouble"""
    x = np.asarray(x)
    re, im = x.real, x.imag
    p = re * re + im * im
    assert p.dtype == (np.float32 if x.dtype == np.complex64 else np.float64)
    return p.astype(np.longdouble)


def probs_partial(n, indices, p, offset=0):
    """longdouble[2^k]: what the amplitudes [offset, offset + len(p)) add to every outcome; `p` = products(...) of them.
    len(p) is a power of two and divides offset, so the piece is a sub-cube: its low bits run, its high bits are fixed."""
    length = len(p)
    low = length.bit_length() - 1
    assert length == 1 << low and offset % length == 0 and offset + length <= 1 << n
    pos = [n - 1 - int(q) for q in indices]
    assert len(set(pos)) == len(pos) and all(0 <= b < n for b in pos)
    inside = sorted((b for b in pos if b < low), reverse=True)  # measured positions that run inside the piece, MSB first
    # one axis per run of index bits that are all measured or all not (most significant first)
    shape, measured_axis = [], []
    b = low - 1
    while b >= 0:
        if b in inside:
            shape.append(2)
            measured_axis.append(True)
            b -= 1
        else:
            e = b
            while e >= 0 and e not in inside:
                e -= 1
            shape.append(1 << (b - e))
            measured_axis.append(False)
            b = e
    cube = p.reshape(shape) if shape else p.reshape(())
    drop = tuple(a for a, m in enumerate(measured_axis) if not m)
    sub = np.sum(cube, axis=drop, dtype=np.longdouble).reshape(-1)  # index: the `inside` bits, first of them most significant
    out = np.zeros(1 << len(pos), dtype=np.longdouble)
    j = np.arange(len(sub), dtype=np.int64)
    m = np.zeros(len(sub), dtype=np.int64)
    for i, b in enumerate(pos):
        if b < low:
            bit = (j >> (len(inside) - 1 - inside.index(b))) & 1
        else:
            bit = (offset >> b) & 1
        m |= bit << i
    out[m] = sub  # (distinct outcomes: `m` is one-to-one in the inside bits)
    return out


def _pieces(x, offset, length):
    x = np.asarray(x)
    length = len(x) - offset if length is None else length
    step = min(PIECE, length & -length, (offset & -offset) or length) if length else 1
    for o in range(offset, offset + length, step):
        yield o, x[o:o + step]


def probs_ref(n, indices, x, offset=0, length=None):
    """float64[2^k]: exact probabilities of every outcome over the amplitudes [offset, offset + length) of the state `x`
    (default: all of it), reduced in pieces of at most PIECE with the partial sums added in longdouble"""
    acc = np.zeros(1 << len(indices), dtype=np.longdouble)
    for o, piece in _pieces(x, offset, length):
        acc += probs_partial(n, indices, products(piece), o)
    return acc.astype(np.float64)


def prob_ref(n, m, indices, x, offset=0, length=None):
    """exact probability of the one outcome `m`"""
    return float(probs_ref(n, indices, x, offset, length)[m])


def norm_partial(p):
    return np.sum(p, dtype=np.longdouble)


def norm_ref(x):
    """exact sum of |amp|^2"""
    acc = np.longdouble(0)
    for _, piece in _pieces(x, 0, None):
        acc += norm_partial(products(piece))
    return float(acc)


def crossing_ref(x, r):
    """soft_measure's scan without rounding: (the first index at which the running sum of the products reaches `r`, or 0
    when it never does; the distance from `r` to the nearest partial sum).  A sample closer to a partial sum than the
    scanning precision resolves has no defined outcome."""
    cum = np.cumsum(products(x), dtype=np.longdouble)
    r = np.longdouble(r)
    hit = np.nonzero(r - cum <= 0)[0]
    return (int(hit[0]) if len(hit) else 0), float(np.min(np.abs(cum - r)))


def outcome_of(n, indices, index):
    """the outcome an amplitude index stands for"""
    return sum(((int(index) >> (n - 1 - int(q))) & 1) << i for i, q in enumerate(indices))


# ---- the cases -----------------------------------------------------------------------------------------------------------
# Index sets are written as amplitude-index POSITIONS in outcome-bit order and turned into qubits by `qubits`.
DTYPES = (np.complex128, np.complex64)


def qubits(n, positions):
    return [n - 1 - b for b in positions]


def seed_of(n, dtype):
    return 1000 + 2 * n + (1 if dtype == np.complex64 else 0)


# k <= 4 (k_measure_probs_small).  One round of a block is 8192 elements; a packed Complex<f32> element is two amplitudes:
#   n = 1, 2, 3, 9, 12   tail only (n = 1 is not packed: a lone 8-byte element);
#   n = 13               f64: exactly one round, no tail;  f32: 4096 elements, tail only;
#   n = 14               f64: two rounds;  f32: exactly one round;
#   n = 15               f64: four rounds; f32: two rounds.
SMALL_NS = (1, 2, 3, 9, 12, 13, 14, 15)
_SMALL_POSITIONS = (
    # position 0 is qubit n-1 (the half of a packed element), 1 is qubit n-2 (bit 0 of the element index), 8 is the block row
    # (bit 7 of a packed element index is position 8, bit 8 is position 9), 11 is kStrideShift (12 for packed elements)
    [0], [1], [7], [8], [9], [10], [11], [12], [13],
    [0, 1], [1, 0], [0, 8], [7, 9], [11, 10], [12, 0], [8, 13],
    [0, 2, 1], [3, 0, 8], [2, 1, 0], [8, 7, 1], [12, 11, 10], [9, 2, 13], [11, 0, 12],
    [0, 8, 3, 1], [5, 0, 11, 2], [7, 8, 1, 0], [0, 1, 7, 8], [12, 11, 10, 9], [13, 3, 12, 8], [9, 12, 0, 10], [3, 2, 1, 0],
)


def small_index_sets(n):
    """every k from 1 to min(4, n); qubit n-1 as the first, a middle and the last outcome bit; qubit n-2; qubit 0 (position
    n-1); either side of positions 8 and 11; ascending, descending and scrambled outcome-bit orders"""
    top = n - 1
    sets = [s for s in _SMALL_POSITIONS if max(s) < n]
    sets += [[top], [top, 0], [0, top]] + ([[1, top, 0], [top, 0, top - 1], [0, top - 1, top, 1]] if n >= 3 else [])
    out = []
    for s in sets:
        if len(set(s)) == len(s) and max(s) < n and s not in out:
            out.append(list(s))
    return [qubits(n, s) for s in out]


# k >= 5 (k_measure_probs_grid).
def grid_route(n, positions, packed):
    """(ki, kg, kl, b0, gx) of a measure_probs call with k >= 5, restated from measure_probs_t: positions are ELEMENT
    positions (one less in a packed Complex<f32> state, whose amplitude position 0 is the half bit: b0 = its outcome bit, else
    -1); the measured positions >= 8 are `high`; ki of them (as many as exceed 11, at most 3) are step bits walked per lane,
    the other kg are on the grid, the kl positions < 8 are lane bits; every (grid outcome, step value) covers `count` elements
    and is shared by gx blocks."""
    shift = 1 if packed and n >= 2 else 0
    b0 = positions.index(0) if shift and 0 in positions else -1
    el = [b - shift for i, b in enumerate(positions) if i != b0]
    high = len([b for b in el if b >= 8])
    ki = min(max(high - 11, 0), 3)
    kg, kl = high - ki, len(el) - high
    count = 1 << (n - shift - high)
    gx = min(max(8192 >> kg, 1), max((count << ki) >> 10, 1))
    return ki, kg, kl, b0, gx


def _scrambled(positions, seed):
    return [int(b) for b in np.random.default_rng(seed).permutation(positions)]


# (n, positions, (ki, kg, kl, b0, gx) for Complex<f64>, the same for packed Complex<f32>); every case runs in both precisions.
# KI = 0 everywhere here; tests/test_measure_ref_cpu.py holds the tuples to grid_route.
GRID_SMALL_CASES = (
    # k = n: count = 1 (f64, n <= 8): 2^n lanes hold one amplitude each and the idle lanes are folded in; n = 9 puts position 8
    # on the grid (two blocks of 256 busy lanes).  Packed: b0 with kl = n - 1, up to b0 + kl = 8 on one block at n = 9.
    (5, [0, 1, 2, 3, 4], (0, 0, 5, -1, 1), (0, 0, 4, 0, 1)),
    (5, [4, 3, 2, 1, 0], (0, 0, 5, -1, 1), (0, 0, 4, 4, 1)),
    (6, [0, 1, 2, 3, 4, 5], (0, 0, 6, -1, 1), (0, 0, 5, 0, 1)),
    (6, [5, 4, 3, 2, 1, 0], (0, 0, 6, -1, 1), (0, 0, 5, 5, 1)),
    (7, [0, 1, 2, 3, 4, 5, 6], (0, 0, 7, -1, 1), (0, 0, 6, 0, 1)),
    (7, [6, 5, 4, 3, 2, 1, 0], (0, 0, 7, -1, 1), (0, 0, 6, 6, 1)),
    (8, [0, 1, 2, 3, 4, 5, 6, 7], (0, 0, 8, -1, 1), (0, 0, 7, 0, 1)),
    (8, [7, 6, 5, 4, 3, 2, 1, 0], (0, 0, 8, -1, 1), (0, 0, 7, 7, 1)),
    (9, [0, 1, 2, 3, 4, 5, 6, 7, 8], (0, 1, 8, -1, 1), (0, 0, 8, 0, 1)),
    (9, [8, 7, 6, 5, 4, 3, 2, 1, 0], (0, 1, 8, -1, 1), (0, 0, 8, 8, 1)),
    (9, [8, 0, 3, 5, 6], (0, 1, 4, -1, 1), (0, 0, 4, 1, 1)),        # a k = 5 subset
    (13, [8, 9, 10, 11, 12], (0, 5, 0, -1, 1), (0, 4, 1, -1, 1)),   # f64: kl = 0, the whole shuffle + LDS fold; gx = 1
    (13, [9, 10, 0, 11, 12], (0, 4, 1, -1, 1), (0, 4, 0, 2, 1)),    # packed: kl = 0 (with b0)
    (13, [6, 2, 9, 10, 11], (0, 3, 2, -1, 1), (0, 3, 2, -1, 1)),    # f64: lane bit 6 measured, 7 folded through LDS
    (13, [7, 2, 9, 10, 11], (0, 3, 2, -1, 1), (0, 3, 2, -1, 1)),    # f64: lane bit 7, not 6;  packed: lane bit 6, not 7
    (13, [8, 2, 10, 11, 12], (0, 4, 1, -1, 1), (0, 3, 2, -1, 1)),   # packed: lane bit 7, not 6
    (13, [0, 1, 2, 3, 4, 5, 6, 7, 8], (0, 1, 8, -1, 4), (0, 0, 8, 0, 4)),  # packed: b0 + kl = 8, 512 lane outcomes per block
)


def _step_cases():
    cases = []
    # Complex<f64>, every position >= 8 measured: 12, 13, 14 high positions -> KI = 1, 2, 3, kg = 11 (2048 grid outcomes),
    # count = 256, gx = 1 (KI = 3: gx = 2, so k_sum_partials runs).  The kernels: k_measure_probs_grid<double, 1>, <double, 2>,
    # <double, 3>.
    for n, ki, gx in ((20, 1, 1), (21, 2, 1), (22, 3, 2)):
        high = list(range(8, n))
        cases.append((n, np.complex128, high, (ki, 11, 0, -1, gx)))                                # kl = 0: the whole fold
        cases.append((n, np.complex128, _scrambled(high + [5, 0, 7], n), (ki, 11, 3, -1, gx)))    # three lane bits, scrambled
    # KI = 1 has UN = 2 rows in flight; its main loop needs count >= 512: twelve high positions, one high position left out
    cases.append((21, np.complex128, list(range(9, 21)), (1, 11, 0, -1, 1)))
    # packed Complex<f32>: element positions >= 8 are amplitude positions >= 9.  The kernels:
    # k_measure_probs_grid<float, KI, f32x4> and, with qubit n-1 measured, <float, KI, f32x4, true>, KI = 1, 2, 3
    for n, ki, gx in ((21, 1, 1), (22, 2, 1), (23, 3, 2)):
        high = list(range(9, n))
        cases.append((n, np.complex64, high, (ki, 11, 0, -1, gx)))
        cases.append((n, np.complex64, _scrambled(high + [6, 1, 8], n), (ki, 11, 3, -1, gx)))
        cases.append((n, np.complex64, high[:5] + [0] + high[5:], (ki, 11, 0, 5, gx)))             # b0: the halves split
    cases.append((22, np.complex64, list(range(10, 22)), (1, 11, 0, -1, 1)))                      # UN = 2 main loop, packed
    cases.append((22, np.complex64, [0] + list(range(10, 22)), (1, 11, 0, 0, 1)))                 # ... with b0
    return tuple(cases)


# (n, dtype, positions, (ki, kg, kl, b0, gx))
GRID_STEP_CASES = _step_cases()

# The Complex<f32> index sets that test_measure_probs_many_outcomes used to hold to the oracle at a loose bar, n = 18, as QUBITS:
# bit 0 (qubit n-1) as the first / last / a middle outcome bit, with and without other row positions, k = 5..16
MANY_N = 18


def many_outcome_sets_f32():
    n = MANY_N
    rng = np.random.default_rng(18)
    for _ in range(7):  # (the draws of that test's Complex<f64> sets come first: the same random sets as before)
        rng.permutation(n)
    cases = [[n - 1, 0, 3, 9, 12], [0, 3, 9, 12, n - 1], [4, n - 1, n - 2, 7, n - 5, 1, 10], list(range(n - 12, n)),
             list(range(n - 1, n - 13, -1)), [0, n - 1, 3, n - 4, 7, n - 9, 11, n - 13, 15, 13, n - 2, 1], list(range(2, n))]
    for k in (5, 8, 11, 14):
        c = [int(v) for v in rng.permutation(n - 1)[:k - 1]]
        c.insert(int(rng.integers(0, k)), n - 1)
        cases.append(c)
    return cases


# measure_prob (k_measure_probs, one outcome): (n, positions, outcomes).  count = 2^(n-k) indices, 2048 per block:
# n = 14 with k = 1, 2: 4 and 2 blocks; n = 13 with k = 13: one index; n = 9 with k = 3: 64 of a block's 256 lanes busy.
def prob_cases():
    rng = np.random.default_rng(13)
    some = sorted(int(v) for v in rng.choice(1 << 13, 8, replace=False))
    return (
        (14, [0], (0, 1)), (14, [6], (0, 1)),
        (14, [0, 9], (0, 1, 2, 3)), (14, [13, 4], (0, 1, 2, 3)),
        (13, _scrambled(range(13), 5), tuple(some)),
        (9, [0, 4, 8], tuple(range(8))), (9, [1, 8, 5], tuple(range(8))),
    )


# soft_measure on small states (one chunk, n = 12: four: the host walk is short, k_find_crossing does the work)
SOFT_F64_NS = (1, 3, 6, 10, 12)
SOFT_F32_NS = (3, 6, 10)
SOFT_EDGES = (0.0, 1e-300, 1.5)  # crossing at once (the first amplitude is zero: r - 0 <= 0), and never
# Complex<f32>: a sample closer than this to a partial sum is left out — r is rounded to f32 (<= 6e-8 for r <= 1) and the
# crossing sub-range is replayed with f32 subtractions of 6e-8 each.  The sample seeds below leave out none
# (tests/test_measure_ref_cpu.py); with 2^10 boundaries 0.2 % of uniform samples would be.
SOFT_MARGIN = 1e-6
SOFT_SAMPLE_SEED = {3: 3, 6: 6, 10: 10}


def soft_samples(seed, count=64):
    return [float(v) for v in np.random.default_rng(seed).uniform(0, 1, count)]


def soft_index_set(n):
    return sorted({0, n // 2, n - 1}, reverse=True)


# The large case of measure_probs with k <= 4, measure_prob and norm_sqr: n = 25 Complex<f64> / n = 26 Complex<f32>, 512 MiB.
# k_measure_probs_small: 2^25 elements = 4096 rounds on 2048 blocks, two per block; k_chunk_norms: 4096 chunks of 8192 elements,
# its four-loads-in-flight loop; k_measure_probs: 1024 blocks (the cap), 16 to 64 strides each.
BIG = ((25, np.complex128), (26, np.complex64))


def big_index_sets(n):
    return [qubits(n, s) for s in ([n - 1], [0, n - 1], [12, 0, 8], [n - 1, 1, 0, 11])]


def big_prob_cases(n):
    return ((qubits(n, [0, 13]), 1), (qubits(n, [n - 1, 7, 2]), 5))
