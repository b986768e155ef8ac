"""apply_op / apply_op_overwrite on DEVICE slices of Complex<f64> / Complex<f32> (qip_hip_apply_op_device, the form all of the
reference's benches call: qip/benches/state_bench.rs:141-155).  A dense op on <= 3 qubits or a Swap, k_all <= 4 indices with
the controls: the table travels in the kernel arguments and the call is ONE launch on the caller's stream — k_cplx_groups for
the whole vector (each input read once), k_gather_cplx for windows.  Bar: bit-equal to the oracle and to the literal kernel
(k_gather_generic, option force_generic); the call can be recorded into a hipGraph."""
import ctypes

import numpy as np
import pytest

import rustqip_amd as q
from rustqip_amd import _ffi
from rustqip_amd.ops import MatrixOp
from test_gpu_a_generic_p import WINDOWS, Buf, device_sync, vector

pytestmark = pytest.mark.gpu

COMPLEX_TYPES = (np.complex128, np.complex64)
S2 = np.sqrt(0.5)
H, X, Y, S = [S2, S2, S2, -S2], [0, 1, 1, 0], [0, -1j, 1j, 0], [1, 0, 0, 1j]


def floats(a):
    return a.view(np.float64 if a.dtype == np.complex128 else np.float32)


def same(got, want):
    """equal viewed as floats: every value, NaN = NaN, and every sign (so -0 is not +0)"""
    g, w = floats(got), floats(want)
    return np.array_equal(g, w, equal_nan=True) and np.array_equal(np.signbit(g), np.signbit(w))


def nan_signs(*arrays):
    """for a failure message: the sign bits of the NaNs of each array (the values themselves are compared by same())"""
    return [np.signbit(floats(a)[np.isnan(floats(a))]).astype(int).tolist() for a in arrays]


def cvals(rng, count):
    return rng.standard_normal(count) + 1j * rng.standard_normal(count)


def run(n, op, x, y0, acc, io=0, oo=0):
    d_in, d_out = Buf(x), Buf(y0)
    try:
        q.apply_op_device(n, op, d_in.slice(), d_out.slice(), io, oo, accumulate=acc)
        return d_out.get()
    finally:
        d_in.close(), d_out.close()


def whole_vector_shapes(n, rng):
    shapes = []
    for low in (n - 1, n - 2, n - 4):  # qubit index of the lowest index bit: position 0, 1, 3
        others = [int(v) for v in rng.permutation(n - 4)]
        for k_all in (1, 2, 3, 4):
            idx = others[:k_all - 1] + [low]
            rng.shuffle(idx)
            for nc in range(k_all):
                k_op = k_all - nc
                if k_op <= 3:  # (a dense 4-qubit table does not fit the kernel arguments: below, on the old route)
                    inner = MatrixOp.new_matrix(idx[nc:], cvals(rng, 4 ** k_op))
                    shapes.append(inner if nc == 0 else MatrixOp.new_control(idx[:nc], idx[nc:], inner))
                if k_op % 2 == 0:
                    sw = MatrixOp.new_swap(idx[nc:nc + k_op // 2], idx[nc + k_op // 2:])
                    shapes.append(sw if nc == 0 else MatrixOp.new_control(idx[:nc], idx[nc:], sw))
    # both of the two lowest positions in the op (Complex<f32>: no pairs), in either order, plain / controlled / swapped
    for a_, b_ in ((n - 1, n - 2), (n - 2, n - 1)):
        shapes += [MatrixOp.new_matrix([a_, b_], cvals(rng, 16)), MatrixOp.new_swap([a_], [b_]), MatrixOp.new_matrix([a_, 1, b_], cvals(rng, 64)),
                   MatrixOp.new_control([a_], [b_], MatrixOp.new_matrix([b_], cvals(rng, 4))),
                   MatrixOp.new_control([2], [a_, b_], MatrixOp.new_swap([a_], [b_])),
                   MatrixOp.new_control([a_, 3], [b_], MatrixOp.new_matrix([b_], cvals(rng, 4)))]
    for g in (H, X, Y, S):
        shapes += [MatrixOp.new_matrix([0], g), MatrixOp.new_matrix([4], g), MatrixOp.new_matrix([n - 1], g)]
    shapes += [MatrixOp.new_control([1], [n - 1], MatrixOp.new_matrix([n - 1], X)), MatrixOp.new_control([n - 1], [2], MatrixOp.new_matrix([2], X)),  # CNOT
               MatrixOp.new_control([0, 5], [3], MatrixOp.new_matrix([3], X)), MatrixOp.new_control([n - 1, 2], [n - 2], MatrixOp.new_matrix([n - 2], X)),  # Toffoli
               MatrixOp.new_control([6], [1, 4], MatrixOp.new_swap([1], [4])), MatrixOp.new_control([3], [n - 1, 0], MatrixOp.new_swap([n - 1], [0]))]  # CSWAP
    # entries that are zero in both parts (skipped), purely imaginary ones, one with a zero real part only, and a zero row
    shapes.append(MatrixOp.new_matrix([2, 5], [1, 0, 2j, 0, 0, 0, 0, 3j, 0, 0, 0, 0, -1j, 0, 0.5 - 0j, 0]))
    shapes.append(MatrixOp.new_matrix([n - 1, 3], [0, 1j, 0, 0, -2j, 0, 0, 1 + 1j, 0, 0, 0, 0, 0, 0, 3, -1j]))
    shapes.append(MatrixOp.new_matrix([1, 6, 3, n - 2], cvals(rng, 256)))  # dense k = 4: today's route (the literal kernel through a handle)
    return shapes


@pytest.mark.parametrize("dtype", COMPLEX_TYPES)
def test_whole_vector_group_kernel_every_shape(O, dtype):
    """both windows = the whole vector: every (indices, controls, kind) shape the group kernels admit with the lowest index bit at
    position 0, 1 and 3, the named gates, zero / imaginary entries, and a dense 4-qubit op on the old route — accumulate and
    overwrite, with a -0.0 and an inf in the input; the oracle, the group kernel and the literal kernel (force_generic) agree
    bit for bit"""
    n = 8
    N = 1 << n
    rng = np.random.default_rng(31)
    for op in whole_vector_shapes(n, rng):
        x, y0 = vector(rng, N, dtype), vector(rng, N, dtype)
        x[3], x[N - 1] = complex(-0.0, 1.5), complex(np.inf, -0.25)
        for acc in (True, False):
            want = y0.copy()
            O.apply_op(n, op, x, want, accumulate=acc)
            outs = []
            for generic in (0, 1):
                q.set_global_option("force_generic", generic)
                try:
                    outs.append(run(n, op, x, y0, acc))
                finally:
                    q.set_global_option("force_generic", 0)
            assert same(outs[0], want) and same(outs[1], want) and same(outs[0], outs[1]), (op, dtype, acc, nan_signs(outs[0], outs[1], want))


def window_ops(n, rng, vals):
    pick = lambda k: [int(v) for v in rng.permutation(n)[:k]]  # noqa: E731
    ops = [MatrixOp.new_matrix(pick(k), vals(4 ** k)) for k in (1, 2, 3)]
    ab = pick(4)
    ops.append(MatrixOp.new_swap(ab[:2], ab[2:]))
    c = pick(4)
    ops.append(MatrixOp.new_control(c[:2], c[2:], MatrixOp.new_matrix(c[2:], vals(16))))
    c = pick(4)
    ops.append(MatrixOp.new_control(c[:1], c[1:], MatrixOp.new_matrix(c[1:], vals(64))))
    c = pick(3)
    ops.append(MatrixOp.new_control(c[:1], c[1:], MatrixOp.new_swap(c[1:2], c[2:])))
    ops.append(MatrixOp.new_control([n - 1], [0], MatrixOp.new_matrix([0], vals(4))))
    return ops


@pytest.mark.parametrize("dtype", COMPLEX_TYPES)
def test_windows_are_one_launch_of_the_literal_fold(O, dtype):
    """every window shape (ragged, empty input, the input's tail, empty output, shifted by one element) with ops whose table fits
    the kernel arguments: k_gather_cplx, bit-equal to the oracle"""
    n = 9
    N = 1 << n
    rng = np.random.default_rng(32)
    for op in window_ops(n, rng, lambda c: cvals(rng, c)):
        x, y0 = vector(rng, N, dtype), vector(rng, N, dtype)
        for (io, il, oo, ol) in WINDOWS(N):
            xin = np.ascontiguousarray(x[io:io + il])
            for acc in (True, False):
                want = y0[:ol].copy()
                O.apply_op(n, op, xin, want, io, oo, accumulate=acc)
                assert same(run(n, op, xin, y0[:ol], acc, io, oo), want), (op, dtype, io, il, oo, ol, acc)


def test_input_windows_accumulate_to_the_whole_vector(O):
    """the reference's provision for several devices (matrix_ops.rs:96-97) on Complex<f64> device slices: accumulate calls over
    four input windows into each of two output windows rebuild the whole product — exactly, with integer-valued data and
    matrices — and equal the oracle's whole-vector result"""
    n = 9
    N = 1 << n
    rng = np.random.default_rng(33)
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
        assert np.array_equal(got, want), op


def odd_buf(arr, odd):
    """a device slice holding `arr` that starts `odd` elements past a 16-byte boundary"""
    b = Buf(np.concatenate([np.zeros(odd, dtype=arr.dtype), arr]))
    s = b.st.as_slice(arr.dtype, odd, arr.size)
    assert s.ptr % 16 == odd * arr.dtype.itemsize
    return b, s


def test_complex64_slices_off_a_16_byte_boundary(O):
    """Complex<f32> slices that start at an odd element are 8-byte aligned only: single amplitudes per lane instead of pairs
    (the whole vector) and the literal fold (windows), bit-equal to the oracle"""
    n = 9
    N = 1 << n
    rng = np.random.default_rng(34)
    dtype = np.complex64
    ops = [MatrixOp.new_matrix([4], cvals(rng, 4)), MatrixOp.new_matrix([n - 1, 2], cvals(rng, 16)), MatrixOp.new_swap([1], [6]),
           MatrixOp.new_control([3], [0, 7, 5], MatrixOp.new_matrix([0, 7, 5], cvals(rng, 64)))]
    for op in ops:
        x, y0 = vector(rng, N, dtype), vector(rng, N, dtype)
        for (io, il, oo, ol) in ((0, N, 0, N), (N // 8, N // 2 + 5, N // 16, N - N // 4)):
            xin = np.ascontiguousarray(x[io:io + il])
            for odd_in, odd_out in ((1, 1), (1, 0), (0, 1)):
                for acc in (True, False):
                    want = y0[:ol].copy()
                    O.apply_op(n, op, xin, want, io, oo, accumulate=acc)
                    (d_in, si), (d_out, so) = odd_buf(xin, odd_in), odd_buf(y0[:ol], odd_out)
                    q.apply_op_device(n, op, si, so, io, oo, accumulate=acc)
                    got = d_out.get()[odd_out:]
                    d_in.close(), d_out.close()
                    assert same(got, want), (op, io, odd_in, odd_out, acc)


class Hip:
    """the few runtime calls of a stream capture, every status checked"""

    def __init__(self):
        self.lib = ctypes.CDLL("libamdhip64.so")

    def __call__(self, name, *args):
        fn = getattr(self.lib, name)
        fn.restype = ctypes.c_int
        status = fn(*args)
        assert status == 0, f"{name} failed with hipError_t {status}"


def test_the_call_is_only_a_launch(O):
    """the reference's bench shape (n = 12, ones in, zeros out, accumulate) recorded into a hipGraph under the strictest capture
    mode (global: an allocation, a copy from pageable memory or a synchronisation inside the capture fails it): three calls =
    three kernel nodes; two launches of the graph = the oracle applied six times, bit for bit"""
    n = 12
    N = 1 << n
    rng = np.random.default_rng(35)
    ops = [MatrixOp.new_matrix([0], H), MatrixOp.new_control([3], [9], MatrixOp.new_matrix([9], X)),
           MatrixOp.new_control([n - 1], [5, 1], MatrixOp.new_matrix([5, 1], cvals(rng, 16)))]
    x = np.ones(N, dtype=np.complex128)
    want = np.zeros(N, dtype=np.complex128)
    for _ in range(2):
        for op in ops:
            O.apply_op(n, op, x, want)
    cops = [op.to_c(_ffi.QIP_C64) for op in ops]  # (built before the capture: nothing but the three calls happens inside it)
    hip = Hip()
    d_in, d_out = Buf(x), Buf(np.zeros(N, dtype=np.complex128))
    si, so = d_in.slice(), d_out.slice()
    device_sync()
    stream, graph, gexec = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    hip("hipStreamCreate", ctypes.byref(stream))
    try:
        hip("hipStreamBeginCapture", stream, ctypes.c_int(0))  # hipStreamCaptureModeGlobal
        try:
            for cop in cops:
                q.apply_op_device(n, cop, si, so, stream=stream.value)
        finally:
            end = hip.lib.hipStreamEndCapture(stream, ctypes.byref(graph))
        assert end == 0 and graph.value, f"hipStreamEndCapture failed with hipError_t {end}"
        try:
            count = ctypes.c_size_t(0)
            hip("hipGraphGetNodes", graph, None, ctypes.byref(count))
            assert count.value == 3
            hip("hipGraphInstantiate", ctypes.byref(gexec), graph, None, None, ctypes.c_size_t(0))
            try:
                hip("hipGraphLaunch", gexec, stream)
                hip("hipGraphLaunch", gexec, stream)
                hip("hipStreamSynchronize", stream)
            finally:
                hip("hipGraphExecDestroy", gexec)
        finally:
            hip("hipGraphDestroy", graph)
    finally:
        hip("hipStreamDestroy", stream)
    got = d_out.get()
    d_in.close(), d_out.close()
    assert same(got, want) and want[0] != 0


@pytest.mark.slow
@pytest.mark.parametrize("dtype,n", ((np.complex128, 22), (np.complex64, 23)))
def test_streaming_variant(O, dtype, n):
    """64 MiB, the smallest vector at which the group kernels use non-temporal accesses (no index within the low three element
    positions): every row against the oracle"""
    rng = np.random.default_rng(36)
    x = vector(rng, 1 << n, dtype)
    d_in, d_out = Buf(x), Buf(np.zeros(1 << n, dtype=dtype))
    for op in (MatrixOp.new_matrix([n - 7, 2], cvals(rng, 16)),
               MatrixOp.new_control([5], [n - 8, 0], MatrixOp.new_matrix([n - 8, 0], cvals(rng, 16)))):
        want = np.zeros(1 << n, dtype=dtype)
        O.apply_op_overwrite(n, op, x, want)
        q.apply_op_device(n, op, d_in.slice(), d_out.slice(), accumulate=False)
        assert same(d_out.get(), want), op
    d_in.close(), d_out.close()
