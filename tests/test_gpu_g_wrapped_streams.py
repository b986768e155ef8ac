"""A wrapped handle issues every kernel, table upload and memset on the CALLER's stream (qip_hip_state_wrap's `stream`).

Forms (tests/wrapped_common.py): W1 (guarded torch tensors, a torch side stream S) and W2 (a guarded tensor, the HIP null
stream, which is torch's default stream) at n = 15, Complex<f64> and Complex<f32>.  On the stream, with no host synchronisation
in between:

    1. the tensor holds a stale state a                         4. the library call under test
    2. a chain of 4096 x 4096 float32 matmuls (the delay)       5. a clone of the buffer at device_ptr()
    3. interior.copy_(b, non_blocking=True)                     6. S.synchronize()

The clone must be what the call makes of b.  A launch, a table upload or a recorded graph that went to another stream runs while
the matmuls still hold S back and sees a: the result would be the one of a (the test checks that the two differ).  The delay is
measured by the test itself, with events, on the machine it runs on, as is the library call's own duration on a warm handle; the
chain is made long enough for delay >= 20 x call, and both figures are in the assertion messages.  torch's side streams are
non-blocking, so the null stream does not wait for them either.

Reference: the owned twin (HipState(n, dtype), upload(b), the same call, download()), which the existing tests of each call hold
to its own reference; the comparison is array_equal — the same kernels on the same values.  Calls that return a value to the
host synchronise it and prove nothing here: they are left out."""
import math

from gpu_common import *  # noqa: F401,F403

from fuzz_ops import fuzz_circuit
from wrapped_common import Form, assert_guards_intact, torch

pytestmark = pytest.mark.gpu

N = 15
DTYPES = (np.complex128, np.complex64)
_IDS = ("c128", "c64")
MIN_RATIO = 20.0
_CHAIN = {}


def _chain(reps):
    """`reps` dependent 4096 x 4096 float32 products on torch's current stream (the factor's entries are scaled to stay finite)"""
    if not _CHAIN:
        g = torch.Generator(device="cuda").manual_seed(5)
        _CHAIN["m"] = torch.randn(4096, 4096, device="cuda", dtype=torch.float32, generator=g) / 64.0
        _CHAIN["v"] = torch.randn(4096, 4096, device="cuda", dtype=torch.float32, generator=g)
        _CHAIN["out"] = torch.empty_like(_CHAIN["v"])
        torch.cuda.synchronize()
    src, dst = _CHAIN["v"], _CHAIN["out"]
    for _ in range(reps):
        torch.matmul(_CHAIN["m"], src, out=dst)
        src, dst = dst, _CHAIN["out"] if dst is not _CHAIN["out"] else _CHAIN["v"]


def _timed(stream, fn):
    """milliseconds of fn()'s work on `stream`, by events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record()
        fn()
        e1.record()
    stream.synchronize()
    return e0.elapsed_time(e1)


def _view(form, ptr):
    """the torch view of the caller's tensor at `ptr`"""
    for buf in form.buffers():
        if buf.ptr == ptr:
            return buf.interior
    return None


def _owned(dtype, x, prepare, call):
    with q.HipState(N, dtype) as st:
        ctx = prepare(st)
        st.upload(x)
        call(st, ctx)
        return st.download()


def _ordered(form_name, dtype, prepare, call):
    """the sequence of the module docstring for one call; `prepare(st)` makes what the call needs beforehand (options, a
    program) and returns it, `call(st, ctx)` is the library call under test"""
    dt = np.dtype(dtype)
    a, b = rand_state(N, 301, dtype), rand_state(N, 302, dtype)
    want, stale = _owned(dtype, b, prepare, call), _owned(dtype, a, prepare, call)
    assert not np.array_equal(want, stale)  # premise: a result made from the stale state is told apart
    a_dev, b_dev = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    form = Form(form_name, N, dtype, a)
    stream = form.stream if form_name == "W1" else torch.cuda.default_stream()
    assert (form_name == "W1") == (stream.cuda_stream != 0)
    st = form.st
    try:
        ctx = prepare(st)
        call(st, ctx)  # warm: every allocation, table buffer and compilation of the call happens here
        st.sync()
        call_ms = _timed(stream, lambda: call(st, ctx))
        _timed(stream, lambda: _chain(2))  # (warm: the BLAS library's own start-up is no part of a product's time)
        per_product = _timed(stream, lambda: _chain(8)) / 8.0
        reps = max(20, int(math.ceil(MIN_RATIO * 1.25 * call_ms / per_product)))
        assert reps <= 400, f"{reps} products for a call of {call_ms:.3f} ms: the call is too slow for this test"
        start = st.device_ptr()
        cur = _view(form, start)
        if cur is None:  # W2 after an odd number of exchanges: the state is in the library's buffer; bring it home
            st.swap_buffers()
            start = st.device_ptr()
            cur = _view(form, start)
        assert cur is not None and start == form.st.device_ptr()
        with torch.cuda.stream(stream):
            cur.copy_(a_dev)                                    # 1
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record()
            _chain(reps)                                        # 2
            e1.record()
            cur.copy_(b_dev, non_blocking=True)                 # 3
            call(st, ctx)                                       # 4
            end = st.device_ptr()
            out = _view(form, end)
            got_dev = out.clone() if out is not None else None  # 5
        stream.synchronize()                                    # 6
        # (W2 after an exchange: the result is in the library's buffer, which torch cannot name — read through the handle, whose
        # copy is queued on the same stream behind the call)
        got = got_dev.cpu().numpy() if got_dev is not None else st.download()
        delay_ms = e0.elapsed_time(e1)
        figures = f"delay {delay_ms:.2f} ms, call {call_ms:.3f} ms, {reps} products of {per_product:.3f} ms"
        print(f"{form_name} {dt.name}: {figures}")
        assert delay_ms >= MIN_RATIO * call_ms, f"the delay is not 20 x the call: {figures}"
        if np.array_equal(got, stale):
            raise AssertionError(f"the call ran ahead of the caller's stream: the result is the one of the stale state ({figures})")
        assert np.array_equal(got, want), f"max|d| = {np.max(np.abs(got - want)):.3e} from the owned twin ({figures})"
        assert np.array_equal(st.download(), want)
        assert_guards_intact(form, form_name)
        return ctx
    finally:
        form.close()


_FORMS = ("W1", "W2")


def _nothing(st):
    return None


@pytest.mark.parametrize("form", _FORMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_apply_op_waits_for_the_callers_stream(dtype, form):
    """W1 and W2, n = 15, both dtypes: apply_op with H on index bit 0 and on the top bit; reference: the owned twin, array_equal"""
    h0, htop = q.make_matrix_op([N - 1], circuits.H), q.make_matrix_op([0], circuits.H)

    def call(st, _):
        st.apply_op(h0)
        st.apply_op(htop)

    _ordered(form, dtype, _nothing, call)


@pytest.mark.parametrize("form", _FORMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_tile_sweeps_wait_for_the_callers_stream(dtype, form):
    """W1 and W2, n = 15, both dtypes: apply_ops with tile = 1 on a 40-gate fuzz_circuit (sweep tables are uploaded per call);
    reference: the owned twin under the same option, array_equal"""
    ops = fuzz_circuit(N, np.random.default_rng(77), 40)

    def prepare(st):
        st.set_option("tile", 1)

    _ordered(form, dtype, prepare, lambda st, _: st.apply_ops(ops))


@pytest.mark.parametrize("form", _FORMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_permute_bits_waits_for_the_callers_stream(dtype, form):
    """W1 and W2, n = 15, both dtypes: permute_bits by a rotation — out of place: the clone is taken from the scratch tensor (W1)
    or the state is downloaded from the library's buffer (W2); reference: the owned twin, array_equal"""
    pi = [(d + 1) % N for d in range(N)]
    _ordered(form, dtype, _nothing, lambda st, _: st.permute_bits(pi))


@pytest.mark.parametrize("form", _FORMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_pauli_rotations_wait_for_the_callers_stream(dtype, form):
    """W1 and W2, n = 15, both dtypes: apply_pauli_rotations with three terms of different X/Y masks (bit 0, the top bit, none);
    reference: the owned twin, array_equal"""
    terms = [{N - 1: "X", 3: "Z"}, {0: "Y", 7: "X", N - 1: "Z"}, {2: "Z", 9: "Z"}]
    _ordered(form, dtype, _nothing, lambda st, _: st.apply_pauli_rotations(terms, [0.3, -1.1, 0.7]))


@pytest.mark.parametrize("form", _FORMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_diagonal_tables_wait_for_the_callers_stream(dtype, form):
    """W1 and W2, n = 15, both dtypes: four consecutive apply_diagonal calls with four different tables — each table goes through
    one of two pinned host copies and one device buffer, so the third call reuses the first copy and every upload has to be
    ordered behind the previous call's kernel; reference: the owned twin, array_equal"""
    rng = np.random.default_rng(8)
    tables = []
    for t in range(4):
        terms = [{int(a): "Z", int(b): "Z"} for a, b in (rng.choice(N, 2, replace=False) for _ in range(5 + t))] + [{t: "Z"}, {N - 1 - t: "Z"}]
        tables.append((terms, rng.standard_normal(len(terms))))

    def call(st, _):
        for t, (terms, coeffs) in enumerate(tables):
            st.apply_diagonal(terms, coeffs, 0.4 + 0.1 * t)

    _ordered(form, dtype, _nothing, call)


@pytest.mark.parametrize("form", _FORMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_function_tables_wait_for_the_callers_stream(dtype, form):
    """W1 and W2, n = 15, both dtypes: two apply_function calls (an XOR with a value table, then an ADD with values and phases),
    each with its own table upload; reference: the owned twin, array_equal"""
    rng = np.random.default_rng(9)
    ins1, outs1 = [N - 1, 0, 9], [N - 2, 5, 1, 7]
    ins2, outs2 = [3, N - 1], [0, 8, N - 3]
    v1 = rng.integers(0, 2 ** len(outs1), size=2 ** len(ins1), dtype=np.uint64)
    v2 = rng.integers(0, 2 ** len(outs2), size=2 ** len(ins2), dtype=np.uint64)
    ph = rng.uniform(-3, 3, size=2 ** len(ins2))

    def call(st, _):
        st.apply_function(ins1, outs1, values=v1, mode="xor")
        st.apply_function(ins2, outs2, values=v2, phases=ph, mode="add")

    _ordered(form, dtype, _nothing, call)


@pytest.mark.parametrize("form", _FORMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_program_waits_for_the_callers_stream(dtype, form):
    """W1 and W2, n = 15, both dtypes: a compile_program recorded beforehand, run() in the sequence.  W1: the run is a graph launch
    on the caller's stream; W2: the null stream cannot be captured, is_graph is False and the eager run is ordered all the same.
    Reference: the owned twin's program, array_equal"""
    ops = fuzz_circuit(N, np.random.default_rng(78), 40)
    progs = []

    def prepare(st):
        progs.append(st.compile_program(ops))
        return progs[-1]

    try:
        prog = _ordered(form, dtype, prepare, lambda st, p: p.run())
        assert bool(prog.is_graph) == (form == "W1"), (form, prog.is_graph)
    finally:
        for p in progs:
            p.close()
