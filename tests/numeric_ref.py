"""High-precision reference and scale-free error measure of the dense / controlled-dense op (plain numpy, no GPU).

The matrix-core dense kernels are not bit-equal to the oracle: they fold in another order, fused, and (k >= 5) with three real
products per complex one.  The oracle computes in the SAME precision, so a comparison with it cannot tell whose rounding is
the larger one, and an absolute bar on normalised states is a relative bar of per cent in Complex<f32>.  This module gives

  * dense_reference: the op of the reference's convention (oracle/qip_oracle.py: qubit t is index bit n-1-t; the matrix is
    row-major; the first listed qubit is the most significant bit of the row index; a controlled op touches the amplitudes
    whose control bits are all set) in np.clongdouble for a complex128 state and in complex128 for a complex64 one;
  * scaled_error: per real component, e = (got - exact) / (u * a_r) with a_r = sum_c (|Re g_rc| + |Im g_rc|) (|Re x_c| + |Im x_c|)
    and u the unit roundoff of the state's precision: e does not change when x or G is scaled, so a state of 2^20, a state
    with forty binades of dynamic range and a non-unitary matrix are held as tightly as a normalised state;
  * hard_bound(k): the derived worst case of every arithmetic form the kernels use;
  * seeded input and matrix builders, and numpy emulations of the three arithmetic forms (tests/test_numeric_ref_cpu.py shows
    that correct arithmetic of each form meets every cap that tests/test_gpu_a_dense_accuracy.py sets).
"""
import functools

import numpy as np

assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble has no 64-bit significand here: no reference for complex128"

U64 = 2.0 ** -53
U32 = 2.0 ** -24
WORK_CAP = 1 << 24   # complex multiply-adds of one long-double reference
MIN_GROUPS = 16

INPUTS = ("normal", "big", "range", "realdom", "cancel")
MATRICES = ("U", "iU", "orth", "wild")


def unit(dtype):
    return U64 if np.dtype(dtype) == np.complex128 else U32


def hard_bound(k):
    """max |e| that no correct form can exceed (derived, not measured).  Every form in the code is a chain of at most 2 * 2^k
    multiply-adds per real component (four products: 2^k terms of G_re x_re and 2^k of G_im x_im in one chain; three products:
    2^k terms of P Xs, then 2^k of R X_im or Q X_re on the same accumulator).  Counted as if no matrix instruction were fused, a
    term passes through its product's rounding and at most 2 * 2^k additions, plus one rounding for X_re + X_im, one for the
    host-built R / Q and one for the final conversion: 2 * 2^k + 4, whatever the summation order (Higham, gamma_m).  The
    magnitudes of the terms of the three-product form add up to at most 2 a_r (|P||Xs| <= a_r; |R||X_im|, |Q||X_re| <= a_r; the
    four- and two-product forms: a_r itself).  Together (2 * 2^k + 4) * 2 units of u * a_r."""
    return 4 * (1 << k) + 8


# ---- index geometry ------------------------------------------------------------------------------------------------------
def group_count(n, targets, controls):
    return 1 << (n - len(targets) - len(controls))


def group_index_table(n, targets, controls=(), groups=None):
    """idx[g, c]: the full index of sub-index c of group g.  Bit b of g goes to the b-th lowest free bit position; the control bits
    are set; bit k-1-j of c is the bit of targets[j]."""
    k = len(targets)
    tpos = [n - 1 - int(t) for t in targets]
    cpos = [n - 1 - int(c) for c in controls]
    assert len(set(tpos + cpos)) == k + len(cpos) and all(0 <= p < n for p in tpos + cpos)
    free = [p for p in range(n) if p not in tpos and p not in cpos]
    g = np.arange(1 << len(free), dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64)
    base = np.zeros_like(g)
    for b, p in enumerate(free):
        base |= ((g >> b) & 1) << p
    for p in cpos:
        base |= 1 << p
    c = np.arange(1 << k, dtype=np.int64)
    sub = np.zeros_like(c)
    for j, p in enumerate(tpos):
        sub |= ((c >> (k - 1 - j)) & 1) << p
    return base[:, None] | sub[None, :]


def sample_groups(n, targets, controls, dtype, seed=0):
    """the groups a case is measured on: None = all of them (every Complex<f32> case; a Complex<f64> case of at most 2^24
    complex multiply-adds), else max(16, 2^24 / 4^k) of them: the first, the last, the rest drawn from a seeded generator"""
    k = len(targets)
    ng = group_count(n, targets, controls)
    if np.dtype(dtype) == np.complex64 or ng * (1 << (2 * k)) <= WORK_CAP:
        return None
    want = max(MIN_GROUPS, WORK_CAP >> (2 * k))
    if want >= ng:
        return None
    rng = np.random.default_rng([seed, n, k, 77])
    rest = rng.choice(np.arange(1, ng - 1, dtype=np.int64), size=want - 2, replace=False)
    return np.sort(np.concatenate([[0], rest, [ng - 1]]).astype(np.int64))


def dense_reference(n, targets, controls, G, x, groups=None):
    """(idx, x_groups, exact): the index table of the (sampled) groups, the input amplitudes there, and G applied to each group in
    the reference precision (np.clongdouble for complex128 input, complex128 for complex64 input)"""
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble has no 64-bit significand here"
    k = len(targets)
    S = 1 << k
    x = np.asarray(x)
    assert x.shape == (1 << n,) and x.dtype in (np.complex128, np.complex64)
    G = np.asarray(G).reshape(S, S)
    hp = np.clongdouble if x.dtype == np.complex128 else np.complex128
    idx = group_index_table(n, targets, controls, groups)
    xg = x[idx]
    exact = xg.astype(hp) @ np.ascontiguousarray(G.astype(hp).T)
    return idx, xg, exact


def scaled_error(got, exact, G, x_groups, dtype):
    """(rms(e), max|e|) over the real components of `got` (same shape as `exact`: groups x 2^k).  A component with a_r = 0
    (a zero row, or only zeros met) must be an exact zero: it counts as e = 0 if it is and as infinity if not."""
    u = unit(dtype)
    G = np.asarray(G).reshape(exact.shape[1], exact.shape[1]).astype(np.complex128)
    xg = np.asarray(x_groups).astype(np.complex128)
    a = (np.abs(xg.real) + np.abs(xg.imag)) @ (np.abs(G.real) + np.abs(G.imag)).T
    hp = exact.real.dtype
    got = np.asarray(got)
    d = np.stack([got.real.astype(hp) - exact.real, got.imag.astype(hp) - exact.imag]).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(a > 0, d / (u * a), np.where(d == 0, 0.0, np.inf))
    return float(np.sqrt(np.mean(e * e))), float(np.max(np.abs(e)))


# ---- matrices ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _matrix64(kind, k, seed):
    rng = np.random.default_rng([seed, k, 11])
    S = 1 << k
    if kind in ("U", "iU"):
        a = rng.standard_normal((S, S)) + 1j * rng.standard_normal((S, S))
        return np.linalg.qr(a)[0] if kind == "U" else 1j * _matrix64("U", k, seed)
    if kind == "orth":
        return np.linalg.qr(rng.standard_normal((S, S)))[0].astype(np.complex128)
    if kind == "wild":  # not unitary, entries over twenty binades, a quarter exact zeros, one zero row and one zero column
        m = (rng.standard_normal((S, S)) + 1j * rng.standard_normal((S, S))) * np.exp2(rng.integers(-10, 11, (S, S)))
        m[rng.random((S, S)) < 0.25] = 0
        m[int(rng.integers(S)), :] = 0
        m[:, int(rng.integers(S))] = 0
        return m
    if kind == "gint":  # Gaussian integers in [-3, 3]^2
        return rng.integers(-3, 4, (S, S)) + 1j * rng.integers(-3, 4, (S, S))
    if kind == "rint":  # integers in [-3, 3], no imaginary part (the two-product form)
        return rng.integers(-3, 4, (S, S)).astype(np.complex128)
    if kind == "ones":  # [[1, 1], [1, 1]] on every target
        return np.ones((S, S), dtype=np.complex128)
    raise ValueError(kind)


def make_matrix(kind, k, dtype, seed=0):
    """the matrix of a case in complex128; for a Complex<f32> state it has been through complex64 first, so that the
    reference sees the matrix the kernel sees"""
    m = _matrix64(kind, k, seed).astype(np.complex128)
    if np.dtype(dtype) == np.complex64:
        m = m.astype(np.complex64).astype(np.complex128)
    return m


# ---- states --------------------------------------------------------------------------------------------------------------
def make_state(kind, n, dtype, seed=0, targets=None, controls=(), G=None):
    """a whole state vector of the input class `kind` (`cancel` needs the op: each of its groups is a column of G^dagger)"""
    if kind != "cancel":
        return _plain_state(kind, n, np.dtype(dtype), seed).copy()
    return _state(kind, n, dtype, seed, targets, controls, G)


@functools.lru_cache(maxsize=4)
def _plain_state(kind, n, dtype, seed):
    return _state(kind, n, dtype, seed)


def _state(kind, n, dtype, seed=0, targets=None, controls=(), G=None):
    dtype = np.dtype(dtype)
    f64 = dtype == np.complex128
    rng = np.random.default_rng([seed, n, INPUTS.index(kind)])
    N = 1 << n
    v = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    if kind in ("normal", "big", "realdom", "cancel"):
        v /= np.linalg.norm(v)
    if kind == "big":
        v *= 2.0 ** 20
    elif kind == "range":
        v *= np.exp2(rng.integers(-40 if f64 else -20, 1, N))
    elif kind == "realdom":
        v = v.real + 1j * v.imag * (2.0 ** -30 if f64 else 2.0 ** -12)
    elif kind == "cancel":
        idx = group_index_table(n, targets, controls)
        S = idx.shape[1]
        Gd = np.conj(np.asarray(G).reshape(S, S))  # row j of conj(G) = column j of G^dagger
        j = rng.integers(0, S, idx.shape[0])
        v[idx] = Gd[j, :] * np.exp2(rng.integers(-5, 6, idx.shape[0]))[:, None]
    elif kind != "normal":
        raise ValueError(kind)
    return v.astype(dtype)


def make_int_state(n, dtype, seed=0):
    """integer components in [-256, 256]"""
    rng = np.random.default_rng([seed, n, 99])
    return (rng.integers(-256, 257, 1 << n) + 1j * rng.integers(-256, 257, 1 << n)).astype(dtype)


def int_reference(n, targets, controls, G, x):
    """the whole output vector in exact int64 arithmetic (G and x have integer components)"""
    S = 1 << len(targets)
    G = np.asarray(G).reshape(S, S)
    gr, gi = np.rint(G.real).astype(np.int64), np.rint(G.imag).astype(np.int64)
    xr, xi = np.rint(x.real).astype(np.int64), np.rint(x.imag).astype(np.int64)
    assert np.array_equal(gr + 1j * gi, G) and np.array_equal(xr + 1j * xi, x)
    idx = group_index_table(n, targets, controls)
    big = np.block([[gr.T, gi.T], [-gi.T, gr.T]])              # [x_re x_im] . big = [y_re y_im]
    y = np.concatenate([xr[idx], xi[idx]], axis=1) @ big
    out_r, out_i = xr.copy(), xi.copy()
    out_r[idx] = y[:, :S]
    out_i[idx] = y[:, S:]
    return out_r, out_i


def same_bits(a, b):
    """equality of the words, not of the values (-0.0 != 0.0, a NaN equals itself)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    w = np.uint64 if a.dtype == np.complex128 else np.uint32
    return np.array_equal(a.view(w), b.view(w))


def untouched_mask(n, targets, controls):
    m = np.ones(1 << n, dtype=bool)
    m[group_index_table(n, targets, controls).ravel()] = False
    return m


class Case:
    """one op on one state: the reference on the sampled groups, computed once; errors(y) measures any whole output vector"""

    def __init__(self, n, targets, controls, G, x, seed=0, reference=True):
        self.n, self.targets, self.controls, self.G, self.x = n, list(targets), list(controls), G, x
        self.k = len(targets)
        if not reference:
            return
        self.groups = sample_groups(n, targets, controls, x.dtype, seed)
        self.idx, self.xg, self.exact = dense_reference(n, targets, controls, G, x, self.groups)
        self.components = self.exact.size * 2

    def errors(self, y):
        assert y.dtype == self.x.dtype and y.shape == self.x.shape
        return scaled_error(y[self.idx], self.exact, self.G, self.xg, self.x.dtype)

    def untouched_equal(self, y):
        if not self.controls:
            return True
        m = untouched_mask(self.n, self.targets, self.controls)
        return same_bits(y[m], self.x[m])


MIN_COMPONENTS = 1 << 14  # of a sample set, so that its maximum is a stable statistic


def repeats(n, targets, controls, dtype):
    """states (seeds) a small case is measured on to reach MIN_COMPONENTS real components"""
    ng = group_count(n, targets, controls)
    groups = sample_groups(n, targets, controls, dtype)
    per = 2 * (ng if groups is None else len(groups)) << len(targets)
    return max(1, -(-MIN_COMPONENTS // per))


def pool(errors):
    """(rms, max) of equally large sample sets taken together"""
    return float(np.sqrt(np.mean([e[0] ** 2 for e in errors]))), max(e[1] for e in errors)


def check_caps(k, kernel, oracle, ratios=True):
    """the three caps of a kernel's (rms, max) against the oracle's on the same samples; returns the failures as text"""
    bad = []
    if not kernel[1] <= hard_bound(k):
        bad.append(f"max|e| = {kernel[1]:.3g} > hard bound {hard_bound(k)}")
    if ratios and not kernel[0] <= 4.0 * oracle[0]:
        bad.append(f"rms(e) = {kernel[0]:.3g} > 4 x oracle's {oracle[0]:.3g}")
    if ratios and not kernel[1] <= 8.0 * oracle[1]:
        bad.append(f"max|e| = {kernel[1]:.3g} > 8 x oracle's {oracle[1]:.3g}")
    return bad


# ---- numpy emulations of the arithmetic forms (groups x 2^k arrays in, groups x 2^k out, in the state's precision) -----------
def _real_types(dtype):
    return (np.float64, np.longdouble) if np.dtype(dtype) == np.complex128 else (np.float32, np.float64)


def _fma(a, b, c, T, W):
    """fl_T(a * b + c) through the wider type W: f32 through f64 is one rounding but for rare double roundings, f64 through the
    64-bit significand is within 2^-10 ulp of fused; exact on integers, exactly homogeneous under powers of two"""
    return (a.astype(W) * b.astype(W) + c.astype(W)).astype(T)


def emulate_four_products(G, X, dtype, drop=None, frag_bits=None):
    """k_gate_kq_mfma / k_gate_tile_mfma: [y_re; y_im] = [[G_re, -G_im], [G_im, G_re]] [x_re; x_im] as one fused chain per row,
    K-steps of four columns, the real-part step before the imaginary-part step.  drop = (row, column): that term is left out
    (a broken chain); frag_bits: the matrix fragments rounded to that many mantissa bits (a coarse data path)."""
    T, W = _real_types(dtype)
    S = X.shape[1]
    gr, gi = G.real.astype(T), G.imag.astype(T)
    if frag_bits is not None:
        gr, gi = _round_bits(gr, frag_bits), _round_bits(gi, frag_bits)
    xr, xi = X.real.astype(T), X.imag.astype(T)
    re = np.zeros(X.shape, T)
    im = np.zeros(X.shape, T)
    for c0 in range(0, S, 4):
        for part in (0, 1):
            for c in range(c0, min(c0 + 4, S)):
                b = (xr if part == 0 else xi)[:, c:c + 1]
                a_re = (gr if part == 0 else -gi)[:, c].copy()
                a_im = (gi if part == 0 else gr)[:, c].copy()
                if drop is not None and drop[1] == c and part == 0:
                    a_re[drop[0]] = 0
                re = _fma(a_re[None, :], b, re, T, W)
                im = _fma(a_im[None, :], b, im, T, W)
    return (re + 1j * im).astype(dtype)


def emulate_three_products(G, X, dtype, drop=None):
    """mfma3_item, NP = 3: Xs = fl(X_re + X_im); K1 = chain of P Xs; re = K1 continued with R X_im, im = K1 continued with Q X_re;
    P = G_re, R = -(G_re + G_im), Q = G_im - G_re built in double and rounded once to the state's precision"""
    T, W = _real_types(dtype)
    S = X.shape[1]
    g_re, g_im = G.real.astype(np.float64), G.imag.astype(np.float64)
    P, R, Q = g_re.astype(T), (-(g_re + g_im)).astype(T), (g_im - g_re).astype(T)
    xr, xi = X.real.astype(T), X.imag.astype(T)
    xs = (xr + xi).astype(T)
    k1 = np.zeros(X.shape, T)
    for c in range(S):
        a = P[:, c].copy()
        if drop is not None and drop[1] == c:
            a[drop[0]] = 0
        k1 = _fma(a[None, :], xs[:, c:c + 1], k1, T, W)
    re, im = k1, k1
    for c in range(S):
        re = _fma(R[None, :, c], xi[:, c:c + 1], re, T, W)
        im = _fma(Q[None, :, c], xr[:, c:c + 1], im, T, W)
    return (re + 1j * im).astype(dtype)


def emulate_two_products(G, X, dtype, drop=None):
    """mfma3_item, NP = 1 (a matrix without an imaginary part): re = chain of P X_re, im = chain of P X_im"""
    T, W = _real_types(dtype)
    assert not np.any(G.imag)
    P = G.real.astype(T)
    xr, xi = X.real.astype(T), X.imag.astype(T)
    re = np.zeros(X.shape, T)
    im = np.zeros(X.shape, T)
    for c in range(X.shape[1]):
        a = P[:, c].copy()
        if drop is not None and drop[1] == c:
            a[drop[0]] = 0
        re = _fma(a[None, :], xr[:, c:c + 1], re, T, W)
        im = _fma(a[None, :], xi[:, c:c + 1], im, T, W)
    return (re + 1j * im).astype(dtype)


def _round_bits(a, bits):
    """round to `bits` stored mantissa bits (nearest): the leading one and `bits` more"""
    m, e = np.frexp(a.astype(np.float64))
    return np.ldexp(np.rint(m * 2.0 ** (bits + 1)) / 2.0 ** (bits + 1), e).astype(a.dtype)


def apply_emulation(form, case, **kw):
    """the whole output vector of an emulated kernel on a Case's op (every group; amplitudes outside stay as they are)"""
    idx = group_index_table(case.n, case.targets, case.controls)
    y = case.x.copy()
    y[idx] = form(case.G, case.x[idx], case.x.dtype, **kw)
    return y


# ---- the kernel cases of tests/test_gpu_a_dense_accuracy.py and tools/dense_accuracy_table.py ----------------------------------
class KernelCase:
    """one row of the case table: the kernel (by the profile label it runs under), precision, k, n, the handle's options, and the
    matrix class every placement is run with (`U`: the four- / three-product forms; `orth`: the two-product form of k >= 5)"""

    def __init__(self, kernel, label, dtype, k, n, options=(), matrix="U", control_all=False):
        self.kernel, self.label, self.dtype, self.k, self.n = kernel, label, np.dtype(dtype), k, n
        self.options, self.matrix, self.control_all = dict(options), matrix, control_all
        self.tile = kernel.startswith("k_gate_tile_mfma")
        self.id = f"{kernel}-{'f64' if self.dtype == np.complex128 else 'f32'}-k{k}-n{n}" + ("" if matrix == "U" else "-real")

    def __repr__(self):
        return self.id


def kernel_cases():
    """the smallest sizes each kernel accepts and the size just past the edge the parity tests use.  k_gate_kq_mfma needs 16 groups
    (n >= k + 4); for k = 3, 4 the default picks it only with two or more targets on low positions, so option mfma = 2 (the
    matrix-core form for every placement) is set there.  k_gate_tile_mfma shares k_gate_kq_mfma's profile label; K = 4 takes
    states of 17 qubits up, K = 5 Complex<f64> states of 23 qubits up plus one per control (n = 24: every placement carries a
    control above the rows)."""
    c128, c64 = np.complex128, np.complex64
    out = []
    for k in (3, 4, 5):
        for n in (k + 4, 10):
            out.append(KernelCase("k_gate_kq_mfma", "k_gate_kq_mfma", c128, k, n, {"mfma": 2} if k < 5 else {}))
    for k in (3, 4, 5):
        out.append(KernelCase("k_gate_kq_mfma", "k_gate_kq_mfma", c64, k, 11, {"mfma": 2}))
    for dt in (c128, c64):
        for n in (17, 19):
            out.append(KernelCase("k_gate_tile_mfma_k4", "k_gate_kq_mfma", dt, 4, n, {"mfma": 2}))
    out.append(KernelCase("k_gate_tile_mfma_k5", "k_gate_kq_mfma", c128, 5, 23))
    out.append(KernelCase("k_gate_tile_mfma_k5", "k_gate_kq_mfma", c128, 5, 24, control_all=True))
    for dt in (c128, c64):
        for k in (6, 7, 8):
            for n in (k + 4, k + 7):
                for mk in ("U", "orth"):
                    out.append(KernelCase("k_gate_big_mfma", "k_gate_big_mfma", dt, k, n, matrix=mk))
    for dt in (c128, c64):
        for k in (9, 10):
            for n in (k + 4, k + 5):
                out.append(KernelCase("k_gate_huge_mfma", "k_gate_big_mfma", dt, k, n))  # (one profile label for k = 6..10)
    return out


def placements(kc):
    """[(name, targets, controls)] as qubit numbers (qubit t is bit position n-1-t): the k lowest positions, the k highest, two
    seeded mixed ones, one mixed with a control (where the state leaves 16 groups beside it), and for the tile kernels one on
    position 5 and one on the split position 11.  A tile kernel's control lies above the rows (position >= 12)."""
    n, k = kc.n, kc.k
    rng = np.random.default_rng([n, k, 5])
    Q = lambda pos: [n - 1 - int(p) for p in pos]  # noqa: E731
    cpos = 15 if kc.control_all else None
    avail = [p for p in range(n) if p != cpos]

    def mixed(must=()):
        rest = [p for p in avail if p not in must]
        return list(must) + [int(p) for p in rng.permutation(rest)[:k - len(must)]]

    def order(pos):  # the listed order decides the row bits: shuffle it
        return [int(p) for p in rng.permutation(pos)]

    out = [("low", Q(avail[:k]), []), ("high", Q(avail[-k:][::-1]), []), ("mixed0", Q(order(mixed())), []), ("mixed1", Q(order(mixed())), [])]
    if kc.tile:
        out.append(("pos5", Q(order(mixed((5,)))), []))
        out.append(("pos11", Q(order(mixed((11,)))), []))
    if kc.control_all:
        out = [(name, t, Q([cpos])) for name, t, _ in out]
    elif n >= k + 1 + 4 and not (kc.tile and kc.k == 5):
        c = int(rng.integers(12, n)) if kc.tile else int(rng.integers(0, n))
        t = [int(p) for p in rng.permutation([p for p in range(n) if p != c])[:k]]
        out.append(("mixed_ctl", Q(t), Q([c])))
    return out


def make_op(q, kc, targets, controls, G):
    op = q.make_matrix_op(list(targets), np.asarray(G).astype(kc.dtype).ravel())
    return q.make_control_op(list(controls), op) if controls else op


class HipRunner:
    """one device handle with a case's options; run() is op . x with the assertion that the profile names the intended kernel
    class and no other (a fall-back must not pass silently)"""

    def __init__(self, q, kc):
        self.q, self.kc = q, kc

    def __enter__(self):
        self.st = self.q.HipState(self.kc.n, self.kc.dtype)
        self.st.__enter__()
        self.st.set_option("profile", 1)
        for key, v in self.kc.options.items():
            self.st.set_option(key, v)
        return self

    def __exit__(self, *exc):
        return self.st.__exit__(*exc)

    def run(self, targets, controls, G, x):
        self.st.upload(x)
        self.st.profile_reset()
        self.st.apply_op(make_op(self.q, self.kc, targets, controls, G))
        y = self.st.download()
        prof = self.st.profile()
        assert set(prof) == {self.kc.label}, (self.kc, targets, controls, prof)
        return y


def oracle_run(O, q, kc, targets, controls, G, x):
    return O.apply_ops_in_place(kc.n, [make_op(q, kc, targets, controls, G)], x.copy())


def measure(O, q, dev, kc, targets, controls, mk, ik):
    """the kernel's and the oracle's (rms(e), max|e|) on the same samples: at least 2^14 real components, over several seeded states
    where one state has fewer; the amplitudes a controlled op leaves alone must come back bit for bit"""
    G = make_matrix(mk, kc.k, kc.dtype)
    ek, eo = [], []
    for seed in range(repeats(kc.n, targets, controls, kc.dtype)):
        x = make_state(ik, kc.n, kc.dtype, seed=seed, targets=targets, controls=controls, G=G)
        case = Case(kc.n, targets, controls, G, x)
        y = dev.run(targets, controls, G, x)
        assert case.untouched_equal(y), (kc, targets, controls, mk, ik, "an amplitude outside the controlled half changed")
        ek.append(case.errors(y))
        eo.append(case.errors(oracle_run(O, q, kc, targets, controls, G, x)))
    return pool(ek), pool(eo)


OTHER_INPUTS = ("big", "realdom", "cancel")
OTHER_MATRICES = (("iU", "realdom"), ("iU", "range"), ("orth", "range"), ("wild", "range"), ("wild", "normal"))


def accuracy_parts(kc):
    """a case's accuracy runs in parts of a few seconds: {part: [(placement, targets, controls, matrix class, input class)]} — `normal`
    and `range` on every placement; the other input classes and the other matrix classes on the first mixed placement"""
    parts = {}
    for name, targets, controls in placements(kc):
        parts[name] = [(name, targets, controls, kc.matrix, ik) for ik in ("normal", "range")]
        if name == "mixed0":
            parts["mixed0-inputs"] = [(name, targets, controls, kc.matrix, ik) for ik in OTHER_INPUTS]
            if kc.matrix == "U":
                parts["mixed0-matrices"] = [(name, targets, controls, mk, ik) for mk, ik in OTHER_MATRICES]
    if kc.n < 17 and kc.k < 8:  # (small states and matrices: one part)
        parts = {"all": [r for runs in parts.values() for r in runs]}
    return parts
