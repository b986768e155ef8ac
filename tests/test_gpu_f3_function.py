"""Classical functions between qubit registers on a device state (include/qip_hipx.h: qipx_state_apply_function;
HipState.apply_function, rustqip_amd.classical): k_function_tile (rustqip_amd/csrc/qip_function_kernels.h) at the short tiles of
n < 11, one and several tiles, every placement of the two registers relative to the wave row, two-pass XOR, ADD at its limit,
tables with one entry per wave and per lane, phases, and the stream order of the table's upload.

The reference is tests/function_ref.py (index arithmetic alone).  Without phases the result carries the input's bits: compared as
bytes.  With phases, for every amplitude |got_j - ref_j| <= 8 u |psi_j|, u = 2^-53 (Complex<f64>) or 2^-24 (Complex<f32>): the
table entry rounded to the state's precision is within 2 u (u per component, and the libm values it rounds), one complex product
adds at most sqrt(5) u, and the complex128 reference's own product and libm error are far below the remaining 3.7 u for f32 and
within it for f64.  Every phase test prints its worst ratio before it asserts."""
import ctypes as C

from gpu_common import *  # noqa: F401,F403

import function_ref as F
from rustqip_amd import _ffi, classical

pytestmark = pytest.mark.gpu

_IDS = ("c128", "c64")
_STATES = {}


def _state(n, dtype, special=False):
    """the case state of (n, dtype): shared, never written to; `special`: amplitude 0 is -0.0 - 0.0i and the last one has an inf"""
    key = (n, np.dtype(dtype), special)
    if key not in _STATES:
        x = F.make_state(n, 31 * n + (dtype == np.complex64), dtype)
        if special:
            x[0] = complex(-0.0, -0.0)
            x[-1] = complex(np.inf, -0.0)
        x.setflags(write=False)
        _STATES[key] = x
    return _STATES[key]


def _qubits(n, positions):
    """index positions -> qubits (qubit q is index bit n-1-q)"""
    return [n - 1 - p for p in positions]


def _table(rng, m, k):
    return rng.integers(0, 2 ** k, size=2 ** m, dtype=np.uint64)


def _same_bits(got, want):
    return got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def _moved(st, n, x, ins, outs, values, mode, what):
    st.upload(x)
    st.apply_function(ins, outs, values=values, mode=mode)
    got = st.download()
    assert _same_bits(got, F.apply_function_ref(n, x, ins, outs, values, None, mode)), what


def _hold_phase(got, ref, x_moved_abs, u, what):
    err = np.abs(got.astype(np.complex128) - ref)
    ratio = float(np.max(err / (u * x_moved_abs)))
    print(f"{what}: worst |got - ref| = {ratio:.3f} u |psi_j| (bar 8)")
    assert ratio <= 8.0, what


# ---- 1: every n = 1 .. 15 -------------------------------------------------------------------------------------------------------
def _small_cases(n):
    """(in positions, out positions): registers of 1 - 3 qubits at the low end, the high end, across index bits 5/6 and 0/1"""
    cases = [([], [0]), ([0], [])] if n == 1 else []
    if n >= 2:
        cases += [([1], [0]), ([0], [1]), ([n - 1], [0]), ([0], [n - 1])]
    if n >= 3:
        cases += [([2], [1, 0]), ([0, 2], [1]), ([n - 3], [n - 1, n - 2]), ([n - 1, n - 2], [n - 3])]
    if n >= 5:
        cases += [([4, 0], [2, 1, 3]), ([n - 1, n - 5], [n - 2, n - 4, n - 3]), ([1, 0], [n - 1, 2])]
    if n >= 7:
        cases += [([4], [5, 6]), ([6, 5], [4]), ([5], [6]), ([6], [5, 0])]
    if n >= 8:
        cases += [([4, 7], [6, 5]), ([5, 6], [7, 4, 0]), ([7, 1], [6, 0, 5])]
    return cases


@pytest.mark.parametrize("dtype", F.DTYPES, ids=_IDS)
def test_every_small_n_both_modes_bit_for_bit(dtype):
    rng = np.random.default_rng(11)
    count = 0
    for n in range(1, 16):
        x = _state(n, dtype, special=True)
        with q.HipState(n, dtype) as st:
            for ipos, opos in _small_cases(n):
                ins, outs = _qubits(n, ipos), _qubits(n, opos)
                if not outs:  # (a phase table of zeros: w = (1, 0), the state keeps its bits)
                    st.upload(x)
                    st.apply_function(ins, outs, phases=np.zeros(2 ** len(ins)))
                    assert _same_bits(st.download(), x), (n, ipos)
                    continue
                for mode in ("xor", "add"):
                    _moved(st, n, x, ins, outs, _table(rng, len(ins), len(outs)), mode, (n, ipos, opos, mode))
                    count += 1
    assert count >= 300


# ---- 2: the placement matrix at n = 14 -------------------------------------------------------------------------------------------
_IN_PLACES = {"in_row": [3, 0], "in_out": [12, 7, 9], "in_mixed": [8, 0, 13, 3], "in_none": []}  # (disjoint from every out place)
_OUT_PLACES = {"out_row": [2, 4, 1], "out_outside": [10, 6, 11], "out_mixed": [10, 2, 6, 5, 11], "out_none": []}


@pytest.mark.parametrize("dtype", F.DTYPES, ids=_IDS)
def test_placement_matrix_at_n14(dtype):
    n = 14
    x = _state(n, dtype)
    rng = np.random.default_rng(12)
    u = F.UNIT[dtype]
    with q.HipState(n, dtype) as st:
        for iname, ipos in _IN_PLACES.items():
            for oname, opos in _OUT_PLACES.items():
                ins, outs = _qubits(n, ipos), _qubits(n, opos)
                if not outs:
                    st.upload(x)
                    st.apply_function(ins, outs, phases=np.zeros(2 ** len(ins)))
                    assert _same_bits(st.download(), x), (iname, oname)
                    phases = rng.uniform(-7, 7, size=2 ** len(ins))
                    st.apply_function(ins, outs, phases=phases)
                    _hold_phase(st.download(), F.apply_function_ref(n, x, ins, outs, None, phases), np.abs(x.astype(np.complex128)), u,
                                f"{iname} {oname}")
                    continue
                for mode in ("xor", "add"):
                    _moved(st, n, x, ins, outs, _table(rng, len(ins), len(outs)), mode, (iname, oname, mode))


# ---- 3: two-pass XOR ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", F.DTYPES, ids=_IDS)
@pytest.mark.parametrize("high", (7, 9))
def test_two_pass_xor(dtype, high):
    n = 16
    opos = list(range(6, 6 + high))[::-1] + [3]
    ipos = [15, 0, 5]
    ins, outs = _qubits(n, ipos), _qubits(n, opos)
    assert q.function_passes(n, ins, outs, "xor") == 2
    with q.HipState(n, dtype) as st:
        assert st.function_passes(ins, outs) == 2
        _moved(st, n, _state(n, dtype), ins, outs, _table(np.random.default_rng(13 + high), len(ins), len(outs)), "xor", high)
        with pytest.raises(q.CircuitError, match="QIPX_FN_ADD with"):
            st.apply_function(ins, outs, values=np.zeros(2 ** len(ins), dtype=np.uint64), mode="add")


# ---- 4: ADD at the limit --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", F.DTYPES, ids=_IDS)
@pytest.mark.parametrize("in_row", ([], [4, 1], [5, 0, 3, 1, 4, 2]), ids=("row0", "row2", "row6"))
def test_add_with_six_positions_outside_the_row(dtype, in_row):
    n = 14
    opos = [9, 13, 6] + in_row + [11, 12, 7]
    k = len(opos)
    free = [p for p in range(n) if p not in opos]
    x = _state(n, dtype)
    rng = np.random.default_rng(14 + k)
    with q.HipState(n, dtype) as st:
        _moved(st, n, x, [], _qubits(n, opos), np.array([2 ** k - 1], dtype=np.uint64), "add", ("constant", k))
        ipos = free[:2]  # (row0: two lane bits; row6: the two positions left, both outside the tile)
        _moved(st, n, x, _qubits(n, ipos), _qubits(n, opos), _table(rng, len(ipos), k), "add", ("table", k))


# ---- 5: the largest table exercised ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", F.DTYPES, ids=_IDS)
@pytest.mark.parametrize("where", ("in_high", "in_low"))
def test_table_of_4096_entries(dtype, where):
    n, m = 16, 12
    ipos = list(range(4, 16)) if where == "in_high" else list(range(12))
    opos = [p for p in range(n) if p not in ipos]
    rng = np.random.default_rng(15)
    rng.shuffle(ipos)
    with q.HipState(n, dtype) as st:
        for mode in ("xor", "add"):
            _moved(st, n, _state(n, dtype), _qubits(n, ipos), _qubits(n, opos), _table(rng, m, len(opos)), mode, (where, mode))


# ---- 6: phases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", F.DTYPES, ids=_IDS)
def test_phases_within_eight_units(dtype):
    n = 14
    x = _state(n, dtype)
    u = F.UNIT[dtype]
    rng = np.random.default_rng(16)
    with q.HipState(n, dtype) as st:
        for ipos, opos, mode in (([13, 2, 7, 0], [9, 4, 6], "xor"), ([1, 5, 3], [12, 6, 0, 8], "add"), ([10, 11], [], "xor"),
                                 ([4, 2, 1], [6, 7, 8, 9, 10, 11, 13, 5, 3], "xor")):  # (the last: two passes, one phase)
            ins, outs = _qubits(n, ipos), _qubits(n, opos)
            values = _table(rng, len(ipos), len(opos)) if opos else None
            phases = rng.uniform(-20, 20, size=2 ** len(ipos))
            st.upload(x)
            st.apply_function(ins, outs, values=values, phases=phases, mode=mode)
            got = st.download()
            ref = F.apply_function_ref(n, x, ins, outs, values, phases, mode)
            moved = F.apply_function_ref(n, x, ins, outs, values, None, mode)
            _hold_phase(got, ref, np.abs(moved.astype(np.complex128)), u, f"{np.dtype(dtype).name} {ipos} -> {opos} {mode}")
            if opos:  # phases of zero: w = (1, 0) and the call is the move
                st.upload(x)
                st.apply_function(ins, outs, values=values, phases=np.zeros(2 ** len(ipos)), mode=mode)
                assert _same_bits(st.download(), moved), (ipos, opos)


# ---- 7: against the existing device routes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", F.DTYPES, ids=_IDS)
@pytest.mark.parametrize("m,k", ((3, 5), (5, 7)))
def test_equals_the_sparse_op_through_apply_op(dtype, m, k):
    n = 14
    rng = np.random.default_rng(17 + m)
    qubits = [int(v) for v in rng.permutation(n)[: m + k]]
    ins, outs = qubits[:m], qubits[m:]
    x = _state(n, dtype)
    with q.HipState(n, dtype) as st, q.HipState(n, dtype) as twin:
        for mode in ("xor", "add"):
            values = _table(rng, m, k)
            op = q.make_sparse_matrix_op(ins + outs, F.permutation_rows(m + k, m, k, values, mode))
            st.upload(x)
            st.apply_function(ins, outs, values=values, mode=mode)
            twin.upload(x)
            twin.apply_op(op)
            assert st.max_abs_diff(twin) == (0.0, 0), (m, k, mode)
            assert np.array_equal(st.download(), twin.download())


def _ripple_carry_adder(a, b, carry):
    """b <- a + b mod 2^len(b), the in-place ripple-carry adder of Cuccaro, Draper, Kutin and Moulton (2004) without its carry-out:
    MAJ on (c, b_i, a_i) upwards, UMA downwards, c = `carry` (zero before and after) and then a_{i-1}"""
    X = circuits.X
    cnot = lambda c, t: q.make_control_op([c], q.make_matrix_op([t], X))  # noqa: E731
    toffoli = lambda c1, c2, t: q.make_control_op([c1, c2], q.make_matrix_op([t], X))  # noqa: E731
    ops = []
    cs = [carry] + list(a[:-1])
    for c, bi, ai in zip(cs, b, a):  # MAJ
        ops += [cnot(ai, bi), cnot(ai, c), toffoli(c, bi, ai)]
    for c, bi, ai in reversed(list(zip(cs, b, a))):  # UMA
        ops += [toffoli(c, bi, ai), cnot(ai, c), cnot(c, bi)]
    return ops


@pytest.mark.parametrize("dtype", F.DTYPES, ids=_IDS)
def test_add_equals_a_ripple_carry_adder_of_toffolis(dtype):
    """8 + 8 register qubits, one carry qubit (qubit 0: the top index bit, so carry = 0 is the first half of the vector), two
    spectators; the registers interleaved and least significant bit first"""
    n = 19
    a = [1 + 2 * i for i in range(8)]
    b = [2 + 2 * i for i in range(8)]
    x = np.zeros(2 ** n, dtype=dtype)
    x[: 2 ** (n - 1)] = _state(n - 1, dtype)
    with q.HipState(n, dtype) as st, q.HipState(n, dtype) as twin:
        st.upload(x)
        classical.add(st, a, b)
        twin.upload(x)
        twin.apply_ops(_ripple_carry_adder(a, b, 0))
        assert st.max_abs_diff(twin) == (0.0, 0)
        got = st.download()
    assert np.array_equal(got, F.apply_function_ref(n, x, a, b, np.arange(256, dtype=np.uint64), None, "add"))
    assert not np.any(got[2 ** (n - 1):])


# ---- 8: ordering ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", F.DTYPES, ids=_IDS)
def test_unsynchronised_calls_with_rewritten_tables(dtype):
    n, m = 14, 10
    ipos, opos = list(range(2, 12)), [13, 0, 12, 1]
    ins, outs = _qubits(n, ipos), _qubits(n, opos)
    rng = np.random.default_rng(18)
    tables = [_table(rng, m, 4) for _ in range(3)]
    phases = rng.uniform(-3, 3, size=2 ** m)
    x = _state(n, dtype)
    with q.HipState(n, dtype) as st, q.HipState(n, dtype) as twin:
        st.upload(x)
        work, ph = np.empty(2 ** m, dtype=np.uint64), np.empty(2 ** m, dtype=np.float64)
        for i, mode in enumerate(("xor", "add", "xor")):
            work[:] = tables[i]
            ph[:] = phases * (i + 1)
            st.apply_function(ins, outs, values=work, phases=ph, mode=mode)  # no synchronise in between
            work[:] = 0  # the caller's arrays are the caller's again
            ph[:] = np.nan
        got = st.download()
        twin.upload(x)
        for i, mode in enumerate(("xor", "add", "xor")):
            twin.apply_function(ins, outs, values=tables[i], phases=phases * (i + 1), mode=mode)
            twin.download()  # (a download waits for the stream)
        want = twin.download()
    assert _same_bits(got, want)
    assert not _same_bits(got, x)


@pytest.mark.parametrize("dtype", F.DTYPES, ids=_IDS)
def test_relabelled_state(dtype):
    """tile = 1 with tile_relabel = 3 at n = 15 (the rotation tests' recipe): the batch leaves the qubits relabelled and the call
    restores the caller's order first"""
    n = 15
    ops = circuits.c2_random_circuit(n, 80, seed=41)
    ins, outs = [0, 9, 14], [3, 13, 7, 1]
    values = _table(np.random.default_rng(19), 3, 4)
    with q.HipState(n, dtype) as st, q.HipState(n, dtype) as twin:
        st.set_option("tile", 1)
        st.set_option("tile_relabel", 3)
        st.set_option("profile", 1)
        st.upload(_state(n, dtype))
        st.apply_ops(ops)
        twin.copy_from(st)  # (settles: a copy in the caller's order)
        st.upload(_state(n, dtype))
        st.apply_ops(ops)
        st.profile_reset()
        st.apply_function(ins, outs, values=values, mode="add")
        assert st.profile().get("k_permute_bits", {}).get("launches", 0) >= 1, "the batch left no layout to restore"
        y = twin.download()
        twin.apply_function(ins, outs, values=values, mode="add")
        assert st.max_abs_diff(twin) == (0.0, 0)
        assert _same_bits(twin.download(), F.apply_function_ref(n, y, ins, outs, values, None, "add"))


# ---- 9: rustqip_amd.classical ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", F.DTYPES, ids=_IDS)
def test_grover_amplifies_as_the_closed_form_says(dtype):
    n, item = 10, 0b1011001110
    reg = list(range(n))[::-1]  # (bit i of the register value = index bit i)
    h_layer = [q.make_matrix_op([t], circuits.H) for t in range(n)]
    x_layer = [q.make_matrix_op([t], circuits.X) for t in range(n)]
    cz = q.make_control_op(list(range(n - 1)), q.make_matrix_op([n - 1], [1, 0, 0, -1]))
    theta = math.asin(2.0 ** (-n / 2))
    tol = 1e-10 if dtype == np.complex128 else 2e-4
    with q.HipState(n, dtype) as st:
        st.init_basis(0)
        st.apply_ops(h_layer)
        for r in range(1, 26):
            classical.phase_oracle(st, reg, [item])
            st.apply_ops(h_layer + x_layer + [cz] + x_layer + h_layer)
            if r in (1, 8, 25):
                p = float(np.abs(st.download()[item]) ** 2)
                want = math.sin((2 * r + 1) * theta) ** 2
                print(f"r = {r}: p(marked) = {p:.12f}, closed form {want:.12f}")
                assert abs(p - want) <= tol
        assert p > 0.999


@pytest.mark.parametrize("dtype", F.DTYPES, ids=_IDS)
def test_exp_mod_into_shows_the_period(dtype):
    n = 9
    xreg, out = [3, 2, 1, 0], [8, 7, 6, 5]  # (qubit 4 is a spectator)
    with q.HipState(n, dtype) as st:
        st.init_basis(0)
        st.apply_ops([q.make_matrix_op([t], circuits.H) for t in xreg])
        classical.exp_mod_into(st, xreg, out, 7, 15)
        probs = st.measure_probs(out)
        got = st.download()
    # measure_probs: bit i of the outcome = qubit out[i]; 7^x mod 15 = 1, 7, 4, 13, 1, ..
    want = np.zeros(16)
    want[[1, 7, 4, 13]] = 0.25
    assert np.allclose(probs, want, rtol=0, atol=1e-6)
    j = np.arange(2 ** n, dtype=np.uint64)
    xs, ys = F.gather(n, j, xreg), F.gather(n, j, out)
    table = np.array([pow(7, int(v), 15) for v in range(16)], dtype=np.uint64)
    support = (ys == table[xs]) & (F.gather(n, j, [4]) == 0)
    assert np.all(np.abs(got[~support]) == 0) and np.allclose(np.abs(got[support]), 0.25, rtol=0, atol=1e-6)


@pytest.mark.parametrize("dtype", F.DTYPES, ids=_IDS)
def test_copy_and_controlled_constant(dtype):
    n = 12
    x = _state(n, dtype)
    a, b, ctl = [0, 5, 11], [7, 2, 9], [4, 10]
    with q.HipState(n, dtype) as st:
        st.upload(x)
        classical.copy(st, a, b)
        assert _same_bits(st.download(), F.apply_function_ref(n, x, a, b, np.arange(8, dtype=np.uint64), None, "xor"))
        st.upload(x)
        classical.add_const(st, b, 13, controls=ctl)
        assert _same_bits(st.download(), F.apply_function_ref(n, x, ctl, b, np.array([0, 0, 0, 5], dtype=np.uint64), None, "add"))


# ---- 10: what the call refuses once it has a handle ---------------------------------------------------------------------------------
def test_value_and_phase_refusals_leave_the_state_alone():
    n = 8
    x = _state(n, np.complex128)
    ins, outs = (C.c_uint64 * 2)(0, 1), (C.c_uint64 * 2)(6, 7)
    ok, big = (C.c_uint64 * 4)(0, 3, 1, 2), (C.c_uint64 * 4)(0, 3, 4, 2)
    ph, bad = (C.c_double * 4)(0.1, 0.2, 0.3, 0.4), (C.c_double * 4)(0.1, float("inf"), 0.3, 0.4)
    with q.HipState(n, np.complex128) as st:
        st.upload(x)

        def refused(*args):
            assert _ffi.lib.qipx_state_apply_function(st._h, *args) == _ffi.QIP_ERR_INVALID
            return _ffi.last_error()

        assert "values[2] = 4 does not fit the out register of 2 qubits" in refused(ins, 2, outs, 2, 0, big, None)
        assert "null value array" in refused(ins, 2, outs, 2, 1, None, ph)
        assert "an empty out register takes no values" in refused(ins, 2, outs, 0, 0, ok, ph)
        assert "an empty out register needs phases" in refused(ins, 2, outs, 0, 0, None, None)
        assert "the phase of entry 1 is not finite" in refused(ins, 2, outs, 2, 0, ok, bad)
        assert "unknown mode 5" in refused(ins, 2, outs, 2, 5, ok, None)
        assert "qubit 1 is in both registers" in refused(ins, 2, (C.c_uint64 * 2)(6, 1), 2, 0, ok, None)
        assert "out of range" in refused(ins, 2, (C.c_uint64 * 2)(6, 8), 2, 0, ok, None)
        with pytest.raises(q.CircuitError, match="a table of 3 entries"):
            st.apply_function([0, 1], [6, 7], values=[0, 1, 2])
        assert _same_bits(st.download(), x)
        st.apply_function([0, 1], [6, 7], values=lambda v: v ^ np.uint64(1), phases=lambda v: 0.5 * v.astype(np.float64), mode="add")
        got = st.download()
    ref = F.apply_function_ref(n, x, [0, 1], [6, 7], np.array([1, 0, 3, 2], dtype=np.uint64), 0.5 * np.arange(4), "add")
    _hold_phase(got, ref, np.abs(F.apply_function_ref(n, x, [0, 1], [6, 7], [1, 0, 3, 2], None, "add")), F.UNIT[np.complex128], "callables")
