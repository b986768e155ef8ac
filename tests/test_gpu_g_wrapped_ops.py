"""Gates, sweeps and programs on handles that wrap caller memory and caller streams (qip_hip_state_wrap).

Handle forms (tests/wrapped_common.py): `owned` (the library's buffers and stream), W1 (guarded torch tensors for amplitudes
and scratch on a torch side stream) and W2 (a guarded torch tensor, no scratch, the HIP null stream); n in 1, 2, 3, 5, 6, 7
(a 64-lane row, a 16-byte pair or a guarded launch shape can run past 2^n), 11, 12 (either side of the tile width) and 15 (the
suite's size for a relabelled plan), Complex<f64> and Complex<f32>.

Every check has three parts:
  * the oracle, as gpu_common.check: one op launched alone from a known vector is IEEE-equal to it where the suite holds that
    route to bit equality (single-qubit gates, CNOT, Swap, permutations of the index bits and the `_special_gates` entries
    flagged bitwise in Complex<f64>; moves in Complex<f32>), and within TOL64 / TOL32 otherwise (matrix cores, k_dense_small,
    batches).  The bars are absolute for a normalised state; the fuzzed circuits hold gates that are not unitary, so a bar is
    scaled by max(1, |want|_2): an op is linear, its error scales with its input;
  * the owned twin that ran the same calls from the same upload: array_equal on the whole vector — same kernels and launch
    geometry, same bits — and, under profile = 1, the same launches per kernel class.  No route was found whose rounding differs:
    a program on W2 runs eagerly (the null stream cannot be captured), which the existing tests hold IEEE-equal to the graph;
  * all guard zones bit for bit, and the buffer contract: device_ptr() names the buffer download() reads, on W1 always one of the
    two interiors with scratch_ptr() the other."""
from gpu_common import *  # noqa: F401,F403
from gpu_common import _permuted, _special_gates  # noqa: F401

from fuzz_ops import EXACT_1Q, EXACT_DIAG, ROUNDED_1Q, ROUNDED_DIAG, fuzz_circuit, seeded_default_batch
from rustqip_amd import _ffi
from rustqip_amd.ops import CircuitError, validate_op
from wrapped_common import (Form, assert_buffer_contract, assert_guards_intact, assert_same_launches, assert_twins, close_forms,
                            make_forms, torch)

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 5, 6, 7, 11, 12, 15)
DTYPES = (np.complex128, np.complex64)
_IDS = ("c128", "c64")
MOVES = ("X", "cnot", "swap")  # exact in either precision: amplitudes are moved with their bits
# the `_special_gates` entries whose route test_gpu_a_ops.py holds IEEE-equal to the oracle at these sizes (single-qubit gates
# bare and controlled, swaps); the dense and sparse entries are flagged for n >= 26 only and keep the TOL64 bar here
BIT_EQUAL_SPECIAL = {"T_bit0", "H_bit0", "H_top", "Rz_top", "Rz_bit2", "cnot_lowctl", "cnot_lowtgt", "toffoli", "cphase", "cH",
                     "swap1", "swap2"}


def _tol(dtype, want):
    return (TOL64 if np.dtype(dtype) == np.complex128 else TOL32) * max(1.0, float(np.linalg.norm(want.astype(np.complex128))))


def _fits(n, op):
    """the op's indices are qubits of an n-qubit state (the shared generators are written for larger n)"""
    try:
        validate_op(n, op, _ffi.QIP_C64)
    except (CircuitError, ValueError, OverflowError):
        return False
    return True


def _palette(n):
    """(name, op, the suite holds it IEEE-equal to the oracle in Complex<f64>): n < 8 the hand palette, n >= 8 seeded circuits"""
    rng = np.random.default_rng(700 + n)
    out = []
    if n >= 8:
        out += [(f"fuzz{i}", op, False) for i, op in enumerate(fuzz_circuit(n, np.random.default_rng(9000 + n), 48))]
        if n >= 12:  # (the palette's edge bits reach index bit 12: at n = 12 some of its ops name a qubit that is not there)
            out += [(f"default{i}", op, False) for i, op in enumerate(seeded_default_batch(n, 0, gates=64)[0])]
        out += [(name, op, bitwise and name in BIT_EQUAL_SPECIAL) for name, op, bitwise in _special_gates(n, rng)]
        return [(name, op, flagged) for name, op, flagged in out if _fits(n, op)]
    kinds = {**EXACT_1Q, **EXACT_DIAG, **ROUNDED_1Q, **ROUNDED_DIAG}
    for t in range(n):
        for name, m in kinds.items():
            out.append((name if name == "X" else f"{name}_{t}", q.make_matrix_op([t], m), True))
    for a in range(n):
        for b in range(n):
            if a != b:
                out.append(("cnot", q.make_control_op([a], q.make_matrix_op([b], EXACT_1Q["X"])), True))
                out.append(("swap", q.make_swap_op([a], [b]), True))
    if n >= 2:
        out.append(("dense2", q.make_matrix_op([n - 1, 0], rand_unitary(2, rng).ravel()), False))
        out.append(("sparse2", q.make_sparse_matrix_op([n - 1, 0], [[(0, 0.6), (1, 0.8j)], [(1, 0.6), (0, 0.8j)], [(3, 1j)], [(2, -1)]]), False))
    if n >= 3:
        out.append(("dense3", q.make_matrix_op([n - 1, 0, n // 2], rand_unitary(3, rng).ravel()), False))
        out.append(("cdense2", q.make_control_op([n // 2], q.make_matrix_op([0, n - 1], rand_unitary(2, rng).ravel())), False))
    if n >= 4:
        out.append(("swap", q.make_swap_op([0, 1], [n - 1, n - 2]), True))
    return out


def _batch(n, rank1=True):
    """the palette as one batch; the rank-one gates (a zero row: they empty half the vector) go last, or are left out"""
    ops = _palette(n)
    first = [op for name, op, _ in ops if not name.startswith("rank1")]
    last = [op for name, op, _ in ops if name.startswith("rank1")]
    return first + (last if rank1 else [])


def _permutations(n):
    return [[(d + 1) % n for d in range(n)], list(range(n))[::-1]] if n >= 2 else []


def _inverse(pi):
    inv = [0] * len(pi)
    for d, p in enumerate(pi):
        inv[p] = d
    return inv


def _hold_oracle(got, want, dtype, bit, what):
    if bit:
        assert np.array_equal(got, want), f"{what}: not IEEE-equal to the oracle, max|d| = {np.max(np.abs(got - want)):.3e}"
    else:
        d, bar = float(np.max(np.abs(got - want))), _tol(dtype, want)
        assert d <= bar, f"{what}: max|d| = {d:.3e} against the oracle, bar {bar:.3e}"


def _bit_equal(name, flagged, dtype):
    return flagged if np.dtype(dtype) == np.complex128 else name in MOVES


# ---- 1. one op at a time -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("generic", (0, 1), ids=("fast", "force_generic"))
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_apply_op_one_at_a_time(O, dtype, n, generic):
    """owned, W1, W2 at every size of SIZES, both dtypes, the fast route and force_generic = 1 (the literal kernel, which writes
    the second buffer): each op of the palette from a fresh upload (n < 8) or from the running state (n >= 8), then permute_bits
    by a rotation and by a reversal.  Reference: the oracle on the vector the op started from (bit equality / TOL as in the
    module docstring; force_generic is the oracle's own fold: IEEE-equal in Complex<f64> for the flagged ops); every wrapped form
    array_equal to the owned twin with the same launches per kernel class; guards and buffer contract after every op."""
    x = rand_state(n, 40 + n, dtype)
    forms = make_forms(n, dtype, x, profile=1, force_generic=generic)
    try:
        cur = x
        for name, op, flagged in _palette(n):
            if n < 8:
                for f in forms:
                    f.upload(x)
                cur = x
            want = oracle_apply(O, n, op, cur)
            for f in forms:
                f.st.apply_op(op)
            what = f"n={n} {np.dtype(dtype).name} generic={generic} {name} {op!r}"
            cur = assert_twins(forms, what)
            _hold_oracle(cur, want, dtype, _bit_equal(name, flagged, dtype), what)
        for pi in _permutations(n):
            want = _permuted(n, pi, cur)
            for f in forms:
                f.st.permute_bits(pi)
            cur = assert_twins(forms, f"n={n} permute_bits {pi}")
            assert np.array_equal(cur, want), (n, pi)
        assert_same_launches(forms, f"n={n} generic={generic}")
    finally:
        close_forms(forms)


# ---- 2. batches ----------------------------------------------------------------------------------------------------------------
ROUTES = {
    "default": ({}, False),
    "tile1": ({"tile": 1}, False),
    "force_generic": ({"force_generic": 1}, False),
    "compiled": ({}, True),
    "compiled_tile1": ({"tile": 1}, True),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_apply_ops_batches(O, dtype, n, route):
    """owned, W1, W2 at every size of SIZES, both dtypes: the palette as ONE batch through apply_ops at defaults, with tile = 1,
    with force_generic = 1, and through compile_ops + apply_compiled (defaults and tile = 1), each batch twice in a row (the
    second starts on whichever buffer the first ended on).  Reference: the oracle's apply_ops_in_place on the vector the batch
    started from, TOL64 / TOL32 scaled by max(1, |want|_2) (batches fuse and hold matrix-core gates); wrapped forms array_equal
    to the owned twin with the same launches per kernel class; guards and buffer contract after every batch."""
    options, compiled = ROUTES[route]
    x = rand_state(n, 60 + n, dtype)
    ops = _batch(n)
    forms = make_forms(n, dtype, x, profile=1, **options)
    try:
        keep = [f.st.compile_ops(ops) for f in forms] if compiled else None
        cur = x
        for rep in range(2):
            want = O.apply_ops_in_place(n, ops, cur.copy())
            for i, f in enumerate(forms):
                if compiled:
                    f.st.apply_compiled(keep[i])
                else:
                    f.st.apply_ops(ops)
            what = f"n={n} {np.dtype(dtype).name} {route} batch {rep}"
            cur = assert_twins(forms, what)
            _hold_oracle(cur, want, dtype, False, what)
        assert_same_launches(forms, f"n={n} {route}")
    finally:
        close_forms(forms)


@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_relabelled_sweeps(O, dtype):
    """owned, W1, W2 at n = 15 with tile = 1 and tile_relabel = 3 (test_relabelled_state's recipe): apply_ops leaves the handle
    relabelled, the first call that needs the caller's order settles it with one k_permute_bits sweep — on W1 into the caller's
    scratch tensor.  Asserts that sweep in every profile, the oracle (TOL scaled as above), array_equal to the owned twin, the
    guards and the buffer contract; then a second relabelled batch from the buffer the first one ended on."""
    n = 15
    ops = circuits.c2_random_circuit(n, 80, seed=41)
    x = rand_state(n, 75, dtype)
    forms = make_forms(n, dtype, x, profile=1, tile=1, tile_relabel=3)
    try:
        cur = x
        for rep in range(2):
            want = O.apply_ops_in_place(n, ops, cur.copy())
            for f in forms:
                f.st.profile_reset()
                f.st.apply_ops(ops)
                assert f.launches().get("k_permute_bits", 0) == 0, (f.name, f.launches())  # premise: left relabelled
            if rep == 0:
                for f in forms:
                    f.st.device_ptr()  # the first call that needs the caller's order
                    assert f.launches().get("k_permute_bits", 0) == 1, (f.name, f.launches())
            cur = assert_twins(forms, f"relabelled batch {rep} {np.dtype(dtype).name}")
            for f in forms:
                assert f.launches().get("k_permute_bits", 0) == 1, (f.name, f.launches())
            _hold_oracle(cur, want, dtype, False, f"relabelled batch {rep}")
        assert_same_launches(forms, "relabelled")
    finally:
        close_forms(forms)


# ---- 3. where the result lives ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (2, 5, 7, 11, 12, 15))
@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_w1_result_alternates_between_the_callers_tensors(dtype, n):
    """W1 at n = 2, 5, 7 (k_permute_bits_small), 11, 12, 15 (the tiled sweeps), both dtypes: after one permute_bits device_ptr()
    is the scratch interior, after a second the amplitude interior again; scratch_ptr() is the other one each time; the torch
    view at device_ptr() is download(); the tensor the sweep only read keeps its content; guards intact.  Reference:
    gpu_common._permuted (a move: exact)."""
    x = rand_state(n, 80 + n, dtype)
    pi = [(d + 1) % n for d in range(n)]
    with Form("W1", n, dtype, x) as f:
        st = f.st
        assert st.device_ptr() == f.amps.ptr and st.scratch_ptr() == f.scratch.ptr
        st.permute_bits(pi)
        assert st.device_ptr() == f.scratch.ptr and st.scratch_ptr() == f.amps.ptr
        assert_buffer_contract(f, f"n={n} one sweep")
        once = _permuted(n, pi, x)
        assert np.array_equal(f.scratch.read(), once)
        assert np.array_equal(f.amps.read(), x)  # (the sweep's source)
        st.permute_bits(pi)
        assert st.device_ptr() == f.amps.ptr and st.scratch_ptr() == f.scratch.ptr
        assert_buffer_contract(f, f"n={n} two sweeps")
        assert np.array_equal(f.amps.read(), _permuted(n, pi, once))
        assert np.array_equal(st.download(), _permuted(n, pi, once))
        st.swap_buffers()  # the documented exchange: the scratch tensor, still holding the first sweep, becomes the state
        assert st.device_ptr() == f.scratch.ptr
        assert np.array_equal(st.download(), once)
        assert_buffer_contract(f, f"n={n} swap_buffers")


@pytest.mark.parametrize("n", (2, 7, 12, 15))
@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_w2_result_may_end_in_library_memory(dtype, n):
    """W2 at n = 2, 7, 12, 15, both dtypes: after an out-of-place op (permute_bits) device_ptr() is not the tensor and download()
    is right; the tensor still holds the sweep's source; after a second sweep the state is in the tensor again and the tensor is
    download().  After close() the tensor is readable through torch, torch.cuda.synchronize() succeeds and a second state created
    afterwards works (the handle freed exactly its own allocation, whichever role it ended in) — closed once with the state in
    library memory and once with it in the tensor.  Reference: gpu_common._permuted."""
    x = rand_state(n, 90 + n, dtype)
    pi = [(d + 1) % n for d in range(n)]
    once = _permuted(n, pi, x)
    for sweeps in (1, 2):
        f = Form("W2", n, dtype, x)
        st = f.st
        assert st.device_ptr() == f.amps.ptr
        st.permute_bits(pi)
        assert st.device_ptr() != f.amps.ptr
        assert np.array_equal(st.download(), once)
        assert np.array_equal(f.amps.read(), x)
        assert_buffer_contract(f, f"n={n} W2 one sweep")
        if sweeps == 2:
            st.permute_bits(pi)
            assert st.device_ptr() == f.amps.ptr
            assert np.array_equal(f.amps.read(), _permuted(n, pi, once))
            assert_buffer_contract(f, f"n={n} W2 two sweeps")
        st.sync()
        f.close()
        torch.cuda.synchronize()
        assert np.array_equal(f.amps.read(), x if sweeps == 1 else _permuted(n, pi, once))
        assert all(f.amps.guards_intact())
        with q.HipState(n, dtype) as fresh:
            fresh.upload(x)
            fresh.permute_bits(pi)
            assert np.array_equal(fresh.download(), once)
        with Form("W2", n, dtype, once) as again:  # the same kind of handle once more, on new memory
            again.st.permute_bits(_inverse(pi))
            assert np.array_equal(again.st.download(), x)
        torch.cuda.synchronize()


# ---- 4. programs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", (0, 1), ids=("default", "tile1"))
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_programs(O, dtype, n, tile):
    """owned, W1, W2 at every size of SIZES, both dtypes, default options and tile = 1: compile_program of the palette batch
    (without the rank-one gates, so that three runs keep a dense vector) and run() three times; then permute_bits and its
    inverse in two calls (the buffers are exchanged twice) and run(); then ONE permute_bits (the state now starts on the other
    buffer) and run().  On W1 every one of the first three runs is a graph launch on the caller's stream; on W2 none is (the
    null stream cannot be captured); after an exchange the run is right whatever is_graph reports.  Reference per run: the
    oracle's apply_ops_in_place on the vector the run started from (TOL scaled as above); array_equal to the owned twin;
    guards and buffer contract after every run."""
    x = rand_state(n, 110 + n, dtype)
    ops = _batch(n, rank1=False)
    forms = make_forms(n, dtype, x, tile=tile)
    progs = []
    try:
        progs = [f.st.compile_program(ops) for f in forms]
        cur = x

        def run_all(what, graphs=None):
            nonlocal cur
            want = O.apply_ops_in_place(n, ops, cur.copy())
            for p in progs:
                p.run()
            if graphs is not None:
                assert [bool(p.is_graph) for p in progs] == graphs, (what, [f.name for f in forms], [bool(p.is_graph) for p in progs])
            assert not progs[2].is_graph, what
            cur = assert_twins(forms, what)
            _hold_oracle(cur, want, dtype, False, what)

        for rep in range(3):
            run_all(f"n={n} {np.dtype(dtype).name} tile={tile} run {rep}", graphs=[True, True, False])
        for pi in _permutations(n)[:1]:
            for f in forms:
                f.st.permute_bits(pi)
            for f in forms:
                f.st.permute_bits(_inverse(pi))
            assert np.array_equal(assert_twins(forms, "there and back"), cur)
            run_all(f"n={n} tile={tile} run after two exchanges")
            for f in forms:
                f.st.permute_bits(pi)
            cur = _permuted(n, pi, cur)
            assert np.array_equal(assert_twins(forms, "one exchange"), cur)
            run_all(f"n={n} tile={tile} run after one exchange")
            run_all(f"n={n} tile={tile} run again")
    finally:
        for p in progs:
            p.close()
        close_forms(forms)


# ---- 5. the alignment rule of wrap ---------------------------------------------------------------------------------------------
def test_wrap_refuses_a_pointer_that_is_not_16_byte_aligned():
    """W1's tensors at n = 5, Complex<f32>: a view that starts at an odd element is 8-byte aligned, and the kernels read two
    amplitudes as one 16-byte element: wrap refuses it as the amplitude buffer and as the scratch buffer, naming the pointer,
    before any kernel runs; the aligned pair is accepted.  No reference: nothing is computed."""
    n = 5
    x = rand_state(n, 3, np.complex64)
    with Form("W1", n, np.complex64, x) as f:
        odd = f.amps.ptr + 8
        with pytest.raises(CircuitError, match="amplitude buffer .* not 16-byte aligned"):
            q.HipState(n, np.complex64, wrap_ptr=odd, scratch_ptr=f.scratch.ptr)
        with pytest.raises(CircuitError, match="scratch buffer .* not 16-byte aligned"):
            q.HipState(n, np.complex64, wrap_ptr=f.amps.ptr, scratch_ptr=f.scratch.ptr + 8)
        assert np.array_equal(f.st.download(), x)
        assert_guards_intact(f, "after the refusals")
