"""qip_hip_apply_op_device on Complex<f64> / Complex<f32> slices for ops whose payload does not fit the kernel arguments: a dense
op on >= 4 qubits and every SparseMatrix.  The payload lives in the library's device-resident cache, keyed by content; once it is
there the call is ONE launch on the caller's stream — the literal fold behind pointers (k_gather_cplx) for windows, repeated
shapes and sparse rows, read-once kernels over the whole vector for a dense op on 4 (k_cplx_dense4) and on 5 / 6 qubits
(k_cplx_dense_tile, from n = k + 6).  Bar: bit-equal (values, NaNs, signs) to the oracle AND to the literal kernel of the state
path (option force_generic); the call can be recorded into a hipGraph."""
import ctypes

import numpy as np
import pytest

import rustqip_amd as q
from rustqip_amd import _ffi
from rustqip_amd.ops import MatrixOp
from test_gpu_a_complex_slices import COMPLEX_TYPES, Hip, cvals, nan_signs, run, same
from test_gpu_a_generic_p import WINDOWS, Buf, device_sync, vector
from test_oracle_golden import REAL_TYPES

pytestmark = pytest.mark.gpu


def both_routes(n, op, x, y0, acc, io=0, oo=0):
    """the call as it is routed, and the same under force_generic (the literal kernel through a handle)"""
    outs = []
    for generic in (0, 1):
        q.set_global_option("force_generic", generic)
        try:
            outs.append(run(n, op, x, y0, acc, io, oo))
        finally:
            q.set_global_option("force_generic", 0)
    return outs


def table(rng, k):
    """a dense table with entries that are zero in both parts (skipped), purely imaginary ones, one with a zero real part and a
    negative-zero imaginary part, and a whole zero row"""
    side = 1 << k
    m = cvals(rng, side * side).reshape(side, side)
    m[rng.integers(0, side, size=side), rng.integers(0, side, size=side)] = 0
    r, c = rng.integers(0, side, size=side), rng.integers(0, side, size=side)
    m[r, c] = 1j * m[r, c].imag
    m[1, 2] = complex(0.0, -0.0)
    m[int(rng.integers(2, side))] = 0
    return m.ravel()


def qubits(n, positions):
    return [n - 1 - p for p in positions]


def dense_shapes(n, k, rng):
    """op bits at positions 0 and 1 (inside a Complex<f32> pair), at n - 1, scattered, in descending index order; 0, 1 and 3
    controls, inside and outside the low six positions"""
    shapes = []
    rest = [int(p) for p in rng.permutation(np.arange(2, n))]
    a = [0, 1] + rest[:k - 2]
    rng.shuffle(a)
    shapes.append(MatrixOp.new_matrix(qubits(n, a), table(rng, k)))
    if n >= k + 1:  # the top position, indices descending (positions ascending), one control on the lowest position left
        b = sorted([n - 1] + [int(p) for p in rng.permutation(np.arange(1, n - 1))[:k - 1]])
        free = [p for p in range(n) if p not in b]
        idx = qubits(n, b)
        assert idx == sorted(idx, reverse=True)
        ctl = qubits(n, free[:1])
        shapes.append(MatrixOp.new_control(ctl, idx, MatrixOp.new_matrix(idx, table(rng, k))))
        if free[-1] >= 6:  # ... and one outside the low six
            ctl = qubits(n, free[-1:])
            shapes.append(MatrixOp.new_control(ctl, idx, MatrixOp.new_matrix(idx, table(rng, k))))
    if n >= k + 3:  # scattered, three controls: the lowest and the two highest positions left
        c = [int(p) for p in rng.permutation(n)[:k]]
        free = [p for p in range(n) if p not in c]
        ctl = qubits(n, [free[0], free[-1], free[-2]])
        shapes.append(MatrixOp.new_control(ctl, qubits(n, c), MatrixOp.new_matrix(qubits(n, c), table(rng, k))))
    return shapes


# n = 7 (one free bit for a 6-qubit op), 8, 11; k_cplx_dense_tile admits n >= k + 6: 10 | 11 for k = 5, 11 | 12 for k = 6
@pytest.mark.parametrize("k", (4, 5, 6))
@pytest.mark.parametrize("dtype", COMPLEX_TYPES)
def test_dense_whole_vector(O, dtype, k):
    rng = np.random.default_rng(400 + k)
    for n in (7, 8, 10, 11, 12):
        N = 1 << n
        for op in dense_shapes(n, k, rng):
            x, y0 = vector(rng, N, dtype), vector(rng, N, dtype)
            x[3], x[N - 1] = complex(-0.0, 1.5), complex(np.inf, -0.25)
            for acc in (True, False):
                want = y0.copy()
                O.apply_op(n, op, x, want, accumulate=acc)
                got, lit = both_routes(n, op, x, y0, acc)
                assert same(got, want) and same(lit, want) and same(got, lit), (n, op, dtype, acc, nan_signs(got, lit, want))


def sparse_rows(rng, k, per_row, ragged):
    """`per_row` stored entries in every row (columns drawn with replacement: repeats happen) or, ragged, 0 .. per_row of them
    with row 1 empty; one stored value is zero"""
    side = 1 << k
    rows = []
    for r in range(side):
        cnt = int(rng.integers(0, per_row + 1)) if ragged else per_row
        if ragged and r == 1:
            cnt = 0
        rows.append([(int(c), complex(v)) for c, v in zip(rng.integers(0, side, size=cnt), cvals(rng, cnt))])
    for r in (0, side - 1):
        if rows[r]:
            rows[r][-1] = (rows[r][-1][0], 0j)  # a stored zero is NOT skipped (0 * inf = NaN, as in the reference)
            break
    return rows


def sparse_op(n, k, rng, per_row, ragged, controlled):
    idx = [int(v) for v in rng.permutation(n)[:k + (1 if controlled else 0)]]  # (targets in any order)
    if controlled:
        return MatrixOp.new_control(idx[:1], idx[1:], MatrixOp.new_sparse(idx[1:], sparse_rows(rng, k, per_row, ragged)))
    return MatrixOp.new_sparse(idx, sparse_rows(rng, k, per_row, ragged))


def check_sparse(O, dtype, n, ops, rng):
    N = 1 << n
    for op in ops:
        x, y0 = vector(rng, N, dtype), vector(rng, N, dtype)
        x[3], x[N - 1] = complex(-0.0, 1.5), complex(np.inf, -0.25)
        for acc in (True, False):
            want = y0.copy()
            O.apply_op(n, op, x, want, accumulate=acc)
            got, lit = both_routes(n, op, x, y0, acc)
            assert same(got, want) and same(lit, want) and same(got, lit), (n, op.indices, dtype, acc, nan_signs(got, lit, want))


@pytest.mark.parametrize("dtype", COMPLEX_TYPES)
def test_sparse_whole_vector(O, dtype):
    n = 10
    rng = np.random.default_rng(410)
    ops = []
    for k in (2, 5, 6, 8):
        for per_row in (1, 2, 4, 5):
            ops.append(sparse_op(n, k, rng, per_row, ragged=per_row in (2, 5), controlled=per_row in (1, 5)))
    check_sparse(O, dtype, n, ops, rng)


@pytest.mark.parametrize("dtype", COMPLEX_TYPES)
def test_sparse_on_sixteen_qubits(O, dtype):
    """the reference's sparse bench shape (state_bench.rs:380-393) and a wide ragged one"""
    n, k = 18, 16
    rng = np.random.default_rng(411)
    perm = rng.permutation(1 << k)
    one = MatrixOp.new_sparse([int(v) for v in rng.permutation(n)[:k]], [[(int(c), complex(0.5, -2.0))] for c in perm])
    check_sparse(O, dtype, n, [one, sparse_op(n, k, rng, 5, ragged=True, controlled=True)], rng)


def window_ops(n, rng, vals):
    d = [int(v) for v in rng.permutation(n)[:4]]
    s = [int(v) for v in rng.permutation(n)[:6]]
    rows = [[(int(c), complex(v)) for c, v in zip(rng.integers(0, 64, size=3), vals(3))] for _ in range(64)]
    return [MatrixOp.new_matrix(d, vals(256)), MatrixOp.new_sparse(s, rows)]


@pytest.mark.parametrize("dtype", COMPLEX_TYPES)
def test_windows_single_calls(O, dtype):
    n = 9
    N = 1 << n
    rng = np.random.default_rng(420)
    for op in window_ops(n, rng, lambda c: cvals(rng, c)):
        x, y0 = vector(rng, N, dtype), vector(rng, N, dtype)
        for (io, il, oo, ol) in WINDOWS(N):
            xin = np.ascontiguousarray(x[io:io + il])
            for acc in (True, False):
                want = y0[:ol].copy()
                O.apply_op(n, op, xin, want, io, oo, accumulate=acc)
                got, lit = both_routes(n, op, xin, y0[:ol], acc, io, oo)
                assert same(got, want) and same(lit, want), (op.indices, dtype, io, il, oo, ol, acc)


def test_input_windows_accumulate_to_the_whole_vector(O):
    """accumulate calls over four input windows into each of two output windows rebuild the whole product, exactly with
    integer-valued data and payloads"""
    n = 9
    N = 1 << n
    rng = np.random.default_rng(421)
    ints = lambda c: (rng.integers(-3, 4, size=c) + 1j * rng.integers(-3, 4, size=c)).astype(np.complex128)  # noqa: E731
    for op in window_ops(n, rng, ints):
        x = (rng.integers(-(1 << 20), 1 << 20, size=N) + 1j * rng.integers(-(1 << 20), 1 << 20, size=N)).astype(np.complex128)
        want = np.zeros(N, dtype=np.complex128)
        O.apply_op(n, op, x, want)
        ins = [(io, Buf(np.ascontiguousarray(x[io:io + N // 4]))) for io in range(0, N, N // 4)]
        got = np.zeros(N, dtype=np.complex128)
        for oo in range(0, N, N // 2):
            d_out = Buf(np.zeros(N // 2, dtype=np.complex128))
            for io, d_in in ins:
                q.apply_op_device(n, op, d_in.slice(), d_out.slice(), io, oo)
            got[oo:oo + N // 2] = d_out.get()
            d_out.close()
        for _, d_in in ins:
            d_in.close()
        assert np.array_equal(got, want), op.indices


@pytest.mark.parametrize("dtype", COMPLEX_TYPES)
def test_the_key_is_the_content_not_the_pointer(O, dtype):
    """the table rewritten in place in the same host buffer between two calls: the second result follows the new bytes — and the
    first bytes, written back, find their entry again"""
    n = 11
    N = 1 << n
    rng = np.random.default_rng(430)
    cdt = _ffi.QIP_C64 if dtype == np.complex128 else _ffi.QIP_C32
    x, y0 = vector(rng, N, dtype), vector(rng, N, dtype)
    for k in (4, 5):
        idx = [int(v) for v in rng.permutation(n)[:k]]
        first, second = cvals(rng, 4 ** k), cvals(rng, 4 ** k)
        cop = MatrixOp.new_matrix(idx, first).to_c(cdt)
        payload = cop._keep[1]  # the descriptor's table: cop.dense points at it
        assert payload.ctypes.data == cop.dense and payload.size == 4 ** k
        for data in (first, second, first):
            payload[:] = data
            want = y0.copy()
            O.apply_op(n, MatrixOp.new_matrix(idx, data), x, want)
            assert same(run(n, cop, x, y0, True), want), (k, dtype)


@pytest.mark.parametrize("cap_mb", (0, 1))
def test_without_the_cache_the_old_route_gives_the_same_bits(O, cap_mb):
    """option slice_payload_cache_mb at 0 (disabled, entries freed) and at 1 MiB with a 4-MiB payload (a dense op on 9 qubits)"""
    n = 9
    N = 1 << n
    rng = np.random.default_rng(440)
    ops = [MatrixOp.new_matrix([int(v) for v in rng.permutation(n)], cvals(rng, 4 ** 9)), sparse_op(n, 6, rng, 3, True, False)]
    if cap_mb == 0:
        ops.append(MatrixOp.new_matrix([2, 7, 0, 5], table(rng, 4)))
    q.set_global_option("slice_payload_cache_mb", cap_mb)
    try:
        for op in ops:
            x, y0 = vector(rng, N, np.complex128), vector(rng, N, np.complex128)
            for acc in (True, False):
                want = y0.copy()
                O.apply_op(n, op, x, want, accumulate=acc)
                assert same(run(n, op, x, y0, acc), want), (op.indices, acc)
            xr = rng.integers(-4, 5, size=N).astype(np.int64)  # real / integer P: the buffer of the call
            rop = MatrixOp.new_matrix(op.indices, rng.integers(-3, 4, size=4 ** len(op.indices)).astype(float)) if op.kind == "Matrix" else None
            if rop is not None:
                want = np.zeros(N, dtype=np.int64)
                O.apply_op(n, rop, xr, want)
                assert np.array_equal(run(n, rop, xr, np.zeros(N, dtype=np.int64), True), want)
    finally:
        q.set_global_option("slice_payload_cache_mb", 256)


class Capture:
    """a stream capture under hipStreamCaptureModeGlobal: an allocation, a copy from pageable memory or a synchronisation inside it
    fails it"""

    def __init__(self, hip):
        self.hip, self.stream, self.graph = hip, ctypes.c_void_p(), ctypes.c_void_p()
        hip("hipStreamCreate", ctypes.byref(self.stream))

    def record(self, body):
        self.hip("hipStreamBeginCapture", self.stream, ctypes.c_int(0))
        try:
            body(self.stream.value)
        finally:
            end = self.hip.lib.hipStreamEndCapture(self.stream, ctypes.byref(self.graph))
        assert end == 0 and self.graph.value, f"hipStreamEndCapture failed with hipError_t {end}"
        count = ctypes.c_size_t(0)
        self.hip("hipGraphGetNodes", self.graph, None, ctypes.byref(count))
        return count.value

    def launch(self, times):
        gexec = ctypes.c_void_p()
        self.hip("hipGraphInstantiate", ctypes.byref(gexec), self.graph, None, None, ctypes.c_size_t(0))
        try:
            for _ in range(times):
                self.hip("hipGraphLaunch", gexec, self.stream)
            self.hip("hipStreamSynchronize", self.stream)
        finally:
            self.hip("hipGraphExecDestroy", gexec)

    def close(self):
        if self.graph.value:
            self.hip("hipGraphDestroy", self.graph)
        self.hip("hipStreamDestroy", self.stream)


def test_the_call_is_only_a_launch(O):
    """a dense 5-qubit op, a controlled dense 4-qubit op, a sparse 8-qubit op (whole vector) and a windowed dense 4-qubit call,
    each issued once before the capture and once inside it: four kernel nodes; two launches of the graph = the oracle applied
    the matching number of times.  A payload first seen INSIDE a capture is refused with QIP_ERR_DEVICE, and the capture goes on."""
    n = 12
    N = 1 << n
    rng = np.random.default_rng(450)
    d5 = MatrixOp.new_matrix([3, 9, 0, 11, 6], cvals(rng, 4 ** 5))
    c4 = MatrixOp.new_control([5], [1, 10, 4, 7], MatrixOp.new_matrix([1, 10, 4, 7], cvals(rng, 256)))
    s8 = sparse_op(n, 8, rng, 3, ragged=True, controlled=False)
    w4 = MatrixOp.new_matrix([2, 8, 11, 5], cvals(rng, 256))
    wio, wil = N // 8, N // 2 + 5  # the windowed call reads x[wio : wio + wil] and accumulates into the whole output
    x = vector(rng, N, np.complex128)
    xw = np.ascontiguousarray(x[wio:wio + wil])
    want = np.zeros(N, dtype=np.complex128)
    for _ in range(3):  # once before the capture, two launches of the graph
        for op in (d5, c4, s8):
            O.apply_op(n, op, x, want)
        O.apply_op(n, w4, xw, want, wio, 0)
    cops = [op.to_c(_ffi.QIP_C64) for op in (d5, c4, s8, w4)]
    unseen = MatrixOp.new_matrix([3, 9, 0, 11, 6], cvals(rng, 4 ** 5)).to_c(_ffi.QIP_C64)
    d_in, d_win, d_out = Buf(x), Buf(xw), Buf(np.zeros(N, dtype=np.complex128))
    si, sw, so = d_in.slice(), d_win.slice(), d_out.slice()

    def calls(stream):
        for cop in cops[:3]:
            q.apply_op_device(n, cop, si, so, stream=stream)
        q.apply_op_device(n, cops[3], sw, so, wio, 0, stream=stream)

    calls(0)
    device_sync()
    cap = Capture(Hip())
    try:
        assert cap.record(calls) == 4
        cap.launch(2)
    finally:
        cap.close()
    got = d_out.get()
    assert same(got, want) and want[0] != 0

    def refused_then_accepted(stream):
        with pytest.raises(q.QipHipError, match="status 2: .*outside the capture"):  # QIP_ERR_DEVICE
            q.apply_op_device(n, unseen, si, so, stream=stream)
        q.apply_op_device(n, cops[0], si, so, stream=stream)

    cap = Capture(Hip())
    try:
        assert cap.record(refused_then_accepted) == 1
    finally:
        cap.close()
    d_in.close(), d_win.close(), d_out.close()


@pytest.mark.parametrize("dtype", REAL_TYPES)
def test_real_p_through_the_cache_inside_a_capture(O, dtype):
    """a dense 5-qubit op and a sparse 6-qubit op per real / integer P: seen once, then recorded (two kernel nodes) and launched"""
    n = 10
    N = 1 << n
    rng = np.random.default_rng(460)
    integer = np.issubdtype(dtype, np.integer)
    vals = lambda c: rng.integers(-3, 4, size=c).astype(float) if integer else rng.standard_normal(c)  # noqa: E731
    rows = [[(int(c), float(v)) for c, v in zip(rng.integers(0, 64, size=2), vals(2))] for _ in range(64)]
    ops = [MatrixOp.new_matrix([int(v) for v in rng.permutation(n)[:5]], vals(4 ** 5)),
           MatrixOp.new_sparse([int(v) for v in rng.permutation(n)[:6]], rows)]
    x = vector(rng, N, dtype)
    want = np.zeros(N, dtype=dtype)
    for _ in range(2):
        for op in ops:
            O.apply_op(n, op, x, want)
    d_in, d_out = Buf(x), Buf(np.zeros(N, dtype=dtype))
    si, so = d_in.slice(), d_out.slice()
    cops = [op.to_c(q.state._slice_dtype_of(x)) for op in ops]

    def calls(stream):
        for cop in cops:
            q.apply_op_device(n, cop, si, so, stream=stream)

    calls(0)
    device_sync()
    cap = Capture(Hip())
    try:
        assert cap.record(calls) == 2
        cap.launch(1)
    finally:
        cap.close()
    got = d_out.get()
    d_in.close(), d_out.close()
    assert np.array_equal(got, want) and np.any(want != 0)


@pytest.mark.slow
@pytest.mark.parametrize("dtype,n", ((np.complex128, 22), (np.complex64, 23)))
def test_streaming_variant(O, dtype, n):
    """64 MiB, the smallest vector at which the read-once kernels use non-temporal accesses: a dense 5-qubit op, every row
    against the oracle"""
    rng = np.random.default_rng(470)
    x = vector(rng, 1 << n, dtype)
    d_in, d_out = Buf(x), Buf(np.zeros(1 << n, dtype=dtype))
    op = MatrixOp.new_matrix([n - 7, 2, n - 1, 9, 4], table(rng, 5))
    want = np.zeros(1 << n, dtype=dtype)
    O.apply_op_overwrite(n, op, x, want)
    q.apply_op_device(n, op, d_in.slice(), d_out.slice(), accumulate=False)
    assert same(d_out.get(), want), op
    d_in.close(), d_out.close()
