"""A reference for the quantum Fourier transform of a register (include/qip_hipx.h: qipx_state_apply_qft) and the bar it is held
to.  Nothing of the kernel's tiles, steps or LDS words appears here.

    qft_exact     every fibre (the 2^m amplitudes that share all other index bits) gathered by index arithmetic into a row in the
                  order of the register value, transformed by a vectorised radix-2 FFT in np.clongdouble (a 64-bit significand
                  is asserted below; the twiddles are np.exp of a long-double argument) and scattered back; the four flag
                  combinations are permutations of the rows' columns before or after (qft_exact_all: all four from two
                  transforms).  A complex64 state is held to the same transform in complex128, 2^29 times finer than its u
    BAR           |got_fibre - exact_fibre|_2 <= 8 m u |old_fibre|_2, u = 2^-53 / 2^-24.  First-order worst case of a radix-2
                  flow: a stage costs one rounding for the sum or difference (1 u), two for the 1/sqrt2 scale and its rounded
                  constant (2 u), sqrt(5) u for the complex product with a twiddle and 1.5 u for the twiddle itself, evaluated in
                  double from an exact integer exponent and rounded once: under 6.8 u per stage, relative to the fibre's norm,
                  which a unitary stage keeps.  One more twiddle product (3.7 u) per pass, at most ceil(m / 6) + 1 passes, stays
                  under 1.2 u per stage.  Folding the scale in once per pass or higher radices only lower the count.
    worst_ratio   max over fibres of |got - exact|_2 / (m u |old|_2): the bar is worst_ratio <= 8
    emulate_flow  the planned flow in numpy in the state's own precision: decimation in frequency from the register's top bit
                  down, passes cut greedily at `tile_high` register positions outside the six low index bits, twiddles
                  W_(2^L)^(v << (L-1-j)) inside a pass from integer exponents, rounded once from a long-double evaluation via
                  double, the scale 2^(-L/2) and the outer twiddle W_(2^hi)^(k xlow) once per pass, the closing bit reversal for
                  natural order.  `wrong=(pass, stage)` adds one to the exponent of that stage's twiddles: what the bar must see."""
import numpy as np

from function_ref import DTYPES, UNIT, gather, scatter  # noqa: F401  (the tests take them from here)

assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble has no 64-bit significand here: no reference for complex128"

BAR = 8.0
ROUND_TRIP_BAR = 16.0
FLAGS = ((False, False), (True, False), (False, True), (True, True))  # (inverse, reversed)
PI_LD = np.arctan(np.longdouble(1)) * 4


def make_state(n, seed, dtype, binades=20):
    """seeded, dense, entries spanning `binades` binades"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(2 ** n) + 1j * rng.standard_normal(2 ** n)
    x *= np.exp2(rng.integers(-binades // 2, binades // 2 + 1, size=2 ** n).astype(np.float64))
    return x.astype(dtype)


def bit_reverse(v, m):
    v = np.asarray(v, dtype=np.uint64)
    r = np.zeros_like(v)
    for b in range(m):
        r |= ((v >> np.uint64(b)) & np.uint64(1)) << np.uint64(m - 1 - b)
    return r


def fibre_index(n, qubits):
    """int64[2^(n-m), 2^m]: row f holds the indices of fibre f, column x the one whose register reads x"""
    m = len(qubits)
    others = [qb for qb in range(n) if qb not in set(qubits)]
    f = scatter(n, np.arange(2 ** (n - m), dtype=np.uint64), others)
    x = scatter(n, np.arange(2 ** m, dtype=np.uint64), list(qubits))
    return (f[:, None] | x[None, :]).astype(np.int64)


def wide_type(dtype):
    """the reference precision: long double for a complex128 state, double for a complex64 one"""
    return np.clongdouble if np.dtype(dtype) == np.complex128 else np.complex128


def _roots(size, sign, wide):
    """exp(sign 2 pi i k / size) for k < size / 2, in the reference precision from a long-double argument"""
    k = np.arange(size // 2).astype(np.longdouble)
    return np.exp((sign * 2j) * (PI_LD * k / np.longdouble(size)).astype(np.clongdouble)).astype(wide)


def fft_rows(a, sign):
    """the unnormalised DFT of every row of a (a power-of-two row length), in a's precision:
    out[y] = sum_x exp(sign 2 pi i x y / M) a[x].  Radix 2, decimation in frequency, every stage one vectorised step."""
    rows, size = a.shape
    m = size.bit_length() - 1
    a = a.copy()
    for s in range(m):
        half = size >> (s + 1)
        v = a.reshape(rows, 1 << s, 2, half)
        top, bot = v[:, :, 0, :].copy(), v[:, :, 1, :].copy()
        v[:, :, 0, :] = top + bot
        v[:, :, 1, :] = (top - bot) * _roots(2 * half, sign, a.dtype)[None, None, :]
    return a[:, bit_reverse(np.arange(size), m).astype(np.int64)]


def qft_exact_all(n, psi, qubits):
    """{(inverse, reversed): the definition of include/qip_hipx.h applied to psi} in the reference precision, from two
    transforms: the inverse is the forward one read at -y, and the reversed orders permute columns"""
    m = len(qubits)
    wide = wide_type(psi.dtype)
    base = np.asarray(psi).astype(wide)
    if m == 0:
        return {f: base.copy() for f in FLAGS}
    idx = fibre_index(n, qubits)
    rev = bit_reverse(np.arange(2 ** m), m).astype(np.int64)
    neg = ((2 ** m - np.arange(2 ** m)) % 2 ** m).astype(np.int64)
    norm = np.sqrt(np.longdouble(2)) ** m
    rows = base[idx]
    fwd = (fft_rows(rows, 1) / norm).astype(wide)
    fwd_of_reversed = (fft_rows(rows[:, rev], 1) / norm).astype(wide)  # the input read in reversed order
    out = {}
    for flags, r in (((False, False), fwd), ((False, True), fwd[:, rev]), ((True, False), fwd[:, neg]),
                     ((True, True), fwd_of_reversed[:, neg])):
        y = base.copy()
        y[idx] = r
        out[flags] = y
    return out


def qft_exact(n, psi, qubits, inverse=False, reversed=False):
    return qft_exact_all(n, psi, qubits)[(bool(inverse), bool(reversed))]


def fibre_errors(n, got, exact, old, qubits, dtype):
    """per fibre |got - exact|_2 / (m u |old|_2) (0 where the fibre is zero and stayed zero; inf where it did not)"""
    m = len(qubits)
    idx = fibre_index(n, qubits) if m else np.arange(2 ** n, dtype=np.int64)[:, None]
    d = np.asarray(got).astype(np.clongdouble) - np.asarray(exact).astype(np.clongdouble)
    num = np.sqrt(np.sum(np.abs(d[idx]) ** 2, axis=1)).astype(np.float64)
    den = np.sqrt(np.sum(np.abs(np.asarray(old).astype(np.clongdouble)[idx]) ** 2, axis=1)).astype(np.float64)
    scale = max(m, 1) * UNIT[np.dtype(dtype).type]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, num / (scale * den), np.where(num > 0, np.inf, 0.0))


def worst_ratio(n, got, exact, old, qubits, dtype):
    return float(np.max(fibre_errors(n, got, exact, old, qubits, dtype)))


def pass_groups(n, qubits, tile_high=6):
    """[(lo, hi)] from the top: a pass takes register bits downward until position number tile_high + 1 outside the six low
    index bits would enter"""
    pos = [n - 1 - qb for qb in qubits]
    groups, hi = [], len(pos)
    while hi > 0:
        lo, out = hi, 0
        while lo > 0:
            outside = pos[lo - 1] >= 6
            if outside and out == tile_high:
                break
            out += outside
            lo -= 1
        groups.append((lo, hi))
        hi = lo
    return groups


def pass_count(n, qubits, reversed, tile_high=6):
    """the rule of qipx_qft_passes"""
    if len(qubits) == 0:
        return 0
    h = sum(1 for qb in qubits if n - 1 - qb >= 6)
    p = max(1, -(-h // tile_high))
    return p if (reversed or p == 1) else p + 1


def _unit_root(exponent, log_size, sign, dtype):
    """exp(sign 2 pi i exponent / 2^log_size) from the integer exponent: long double, rounded to double, then to dtype"""
    e = np.asarray(exponent, dtype=np.uint64) & np.uint64(2 ** log_size - 1)
    if log_size <= 12:  # (few distinct exponents: a table)
        return _unit_root_direct(np.arange(2 ** log_size, dtype=np.uint64), log_size, sign)[e.astype(np.int64)]
    return _unit_root_direct(e, log_size, sign)


def _unit_root_direct(e, log_size, sign):
    w = np.exp((sign * 2j) * (PI_LD * e.astype(np.longdouble) / np.longdouble(2) ** log_size).astype(np.clongdouble))
    return w.astype(np.complex128)


def emulate_flow(n, psi, qubits, inverse=False, reversed=False, tile_high=6, wrong=None):
    dtype = np.dtype(psi.dtype)
    real = np.float64 if dtype == np.complex128 else np.float32
    m = len(qubits)
    x = np.array(psi, dtype=dtype)
    if m == 0:
        return x
    flow = list(qubits)[::-1] if (inverse and reversed) else list(qubits)
    sign = -1 if inverse else 1
    j = np.arange(2 ** n, dtype=np.uint64)
    value = gather(n, j, flow)
    with np.errstate(all="ignore"):
        for number, (lo, hi) in enumerate(pass_groups(n, flow, tile_high)):
            length = hi - lo
            for i in range(hi - 1, lo - 1, -1):
                a_idx = np.flatnonzero(((value >> np.uint64(i)) & np.uint64(1)) == 0)
                b_idx = a_idx + (1 << (n - 1 - flow[i]))
                v = (value[a_idx] >> np.uint64(lo)) & np.uint64(2 ** (i - lo) - 1)
                exponent = v << np.uint64(length - 1 - (i - lo))
                if wrong == (number, i):
                    exponent = exponent + np.uint64(1)
                w = _unit_root(exponent, length, sign, dtype).astype(dtype)
                a, b = x[a_idx], x[b_idx]
                x[a_idx] = a + b
                x[b_idx] = w * (a - b)
            scale = np.ldexp(np.sqrt(0.5) if length & 1 else 1.0, -(length // 2))
            if lo > 0:
                k = bit_reverse((value >> np.uint64(lo)) & np.uint64(2 ** length - 1), length)
                xlow = value & np.uint64(2 ** lo - 1)
                w = (_unit_root(k * xlow, hi, sign, dtype) * scale).astype(dtype)
                x = (w * x).astype(dtype)
            else:
                x = (x * real(scale)).astype(dtype)
    assert x.dtype == dtype
    if not reversed:  # the flow leaves the register bit-reversed
        idx = fibre_index(n, flow)
        rows = x[idx]
        x[idx] = rows[:, bit_reverse(np.arange(2 ** m), m).astype(np.int64)]
    return x


# ---- the shapes the GPU tests use (tests/test_gpu_f3_qft.py) and the CPU bar test runs the emulation on (tests/test_qft_cpu.py)

def qubits_at(n, positions):
    """the register whose bit i is index position positions[i]"""
    return [n - 1 - p for p in positions]


def small_cases():
    """(n, qubits) for every n = 1 .. 13 with registers of 1 - 4 qubits: at the low end, at the high end, across index bits 5 / 6
    and 0 / 1, and in scrambled significance order"""
    cases = []
    for n in range(1, 14):
        seen = set()
        rng = np.random.default_rng(40 + n)
        for m in range(1, min(4, n) + 1):
            placed = [list(range(m)), list(range(n - m, n))]
            if n >= 7 + (m - 1) // 2 and m >= 2:
                start = 6 - m // 2
                placed.append(list(range(start, start + m)))                       # across index bits 5 / 6
            if m >= 2:
                placed.append([1, 0] + [int(p) for p in rng.permutation(np.arange(2, n))[:m - 2]])  # across 0 / 1, scrambled
                placed.append([int(p) for p in rng.permutation(n)[:m]])            # anywhere, scrambled
                placed.append(list(range(n - m, n))[::-1])                         # the high end, most significant bit lowest
                for _ in range(3):                                                 # three more anywhere, scrambled
                    placed.append([int(p) for p in rng.permutation(n)[:m]])
            else:
                placed += [[p] for p in range(1, n - 1)]                           # one qubit: every position
            for pos in placed:
                if tuple(pos) not in seen:
                    seen.add(tuple(pos))
                    cases.append((n, qubits_at(n, pos)))
    return cases


def placement_cases():
    """n = 14: the register wholly inside the row, wholly outside, mixed, mixed with reversed and scrambled significance, beside
    bystander bits inside and outside the row"""
    n = 14
    return [(n, qubits_at(n, p)) for p in (
        [0, 1, 2, 3, 4, 5], [2, 4, 1], [6, 7, 8, 9, 10, 11, 12, 13], [13, 9, 7], [3, 4, 5, 6, 7, 8], [8, 7, 6, 5, 4, 3],
        [10, 2, 13, 5, 6, 0, 8], [1, 12, 3, 7], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13], [13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0])]


def boundary_cases():
    """(n, qubits, passes natural, passes reversed) at the smallest n that shows each pass boundary.  The greedy cut opens a later
    group with the position outside the row that forced the cut, so a row bit can be the top bit of the first group only: the
    last two cases put row bits there and directly below the top of the second group."""
    return [
        (13, qubits_at(13, [7, 8, 9, 10, 11, 12]), 1, 1),                       # h = 6
        (13, qubits_at(13, [6, 7, 8, 9, 10, 11, 12]), 3, 2),                    # h = 7
        (13, qubits_at(13, [6, 0, 3, 7, 8, 9, 10, 11, 12, 5]), 3, 2),           # h = 7, a row bit on top, two below the cut
        (13, qubits_at(13, [2, 12, 4, 6, 7, 1, 8, 9, 10, 11, 3]), 3, 2),        # the second group: outside, row, outside, row
        (19, qubits_at(19, list(range(6, 18))), 3, 2),                          # h = 12
        (19, qubits_at(19, list(range(6, 19))), 4, 3),                          # h = 13
        (19, qubits_at(19, list(range(19))), 4, 3),                             # m = n = 19
    ]


TIE_REGISTER = qubits_at(12, [7, 2, 11, 0, 9, 5, 6, 3, 10])  # n = 12: nine qubits, scrambled (the tie to apply_ops)


# the other registers of tests/test_gpu_f3_qft.py and tests/test_gpu_g_wrapped_qft.py
ZERO_FIBRE_CASES = [(13, qubits_at(13, [6, 0, 3, 7, 8, 9, 10, 11, 12, 5])), (10, qubits_at(10, [7, 2, 9])), (5, qubits_at(5, [1, 3]))]
ROUND_TRIP_CASES = [(13, qubits_at(13, [6, 0, 3, 7, 8, 9, 10, 11, 12, 5])), (14, qubits_at(14, [3, 4, 5, 6, 7, 8])),
                    (9, qubits_at(9, [8, 0, 4, 1]))]
ORDER_FINDING = (12, list(range(8)), list(range(8, 12)))  # n, counting, work
EMPTY_CASE = (9, [])
WRAPPED_N = 15
WRAPPED_ONE_PASS = [(qubits_at(15, [0, 1, 2, 3, 4, 5, 6, 7]), False, False), (qubits_at(15, [14, 3, 9, 0, 12]), True, False),
                    (qubits_at(15, [9, 10, 11, 12, 13, 14]), False, True)]
WRAPPED_REVERSED_PASSES = [(qubits_at(15, [6, 7, 8, 9, 10, 11, 12, 13, 14]), False, True), (list(range(15)), True, True)]
WRAPPED_NATURAL_PASSES = [(qubits_at(15, [6, 2, 7, 8, 9, 10, 11, 12, 13]), False, False)]


def all_gpu_shapes():
    """every (n, register) a GPU test transforms"""
    shapes = small_cases() + placement_cases() + [(n, qs) for n, qs, _, _ in boundary_cases()] + [(12, TIE_REGISTER)]
    shapes += ZERO_FIBRE_CASES + ROUND_TRIP_CASES + [(ORDER_FINDING[0], ORDER_FINDING[1]), (1, [0])]
    shapes += [(WRAPPED_N, qs) for qs, _, _ in WRAPPED_ONE_PASS + WRAPPED_REVERSED_PASSES + WRAPPED_NATURAL_PASSES]
    seen, out = set(), []
    for n, qs in shapes:
        if (n, tuple(qs)) not in seen:
            seen.add((n, tuple(qs)))
            out.append((n, list(qs)))
    return out
