"""Multiplexed gates on a device state (include/qip_hipx.h: qipx_state_apply_multiplexed; HipState.apply_multiplexed,
rustqip_amd.multiplex): k_multiplex (rustqip_amd/csrc/qip_multiplex_kernels.h) at the short rows of n < 6, every n up to 13, every
placement of the two registers relative to the wave row, launches of several blocks whose waves walk several steps, the largest
table, one matrix per lane and per wave, the stream order of the table's upload, identity halves, refusals, a relabelled state,
and the Python layer.

The reference is tests/multiplex_ref.py (index arithmetic alone).  Every comparison is BIT FOR BIT against
apply_multiplexed_spec, the header's arithmetic in the state's precision, unless a test says otherwise; the distance of that
arithmetic from an exact evaluation is held by tests/test_multiplex_cpu.py."""
import ctypes as C

from gpu_common import *  # noqa: F401,F403

import function_ref as F
import multiplex_ref as R
from rustqip_amd import _ffi, multiplex

pytestmark = pytest.mark.gpu

_IDS = ("c128", "c64")
_STATES = {}


def _state(n, dtype):
    """the case state of (n, dtype): shared, never written to"""
    key = (n, np.dtype(dtype))
    if key not in _STATES:
        x = R.make_state(n, 37 * n + (dtype == np.complex64), dtype)
        x.setflags(write=False)
        _STATES[key] = x
    return _STATES[key]


def _qubits(n, positions):
    """index positions -> qubits (qubit q is index bit n-1-q)"""
    return [n - 1 - p for p in positions]


def _same_bits(got, want):
    return got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def _with_specials(n, x, select, targets, table):
    """x with -0.0 and inf in some amplitudes whose matrix row is a unit row (nowhere else: they would spread NaN)"""
    j = np.arange(2 ** n, dtype=np.uint64)
    keep = R.unit_rows(np.asarray(table).astype(x.dtype))[R.gather(n, j, select).astype(np.int64), R.gather(n, j, targets).astype(np.int64)]
    # a special amplitude may only sit in a group ALL of whose rows are unit rows: any other row of the group would multiply it
    _, _, part = R._groups(n, select, targets)
    whole = np.all([keep[p] for p in part], axis=0)
    at = np.flatnonzero(whole)
    y = np.array(x)
    y[at[0::3]] = complex(-0.0, -0.0)
    y[at[1::3]] = complex(np.inf, -0.0)
    return y, len(at)


def _run(st, n, x, select, targets, table, what):
    st.upload(x)
    st.apply_multiplexed(select, targets, table)
    got = st.download()
    want = R.apply_multiplexed_spec(n, x, select, targets, table)
    if not _same_bits(got, want):
        bad = np.flatnonzero(np.any(got.view(np.uint8).reshape(len(got), -1) != want.view(np.uint8).reshape(len(got), -1), axis=1))
        raise AssertionError(f"{what}: {bad.size} amplitudes differ from the spec, first at index {bad[0] if bad.size else -1}: "
                             f"{got[bad[:1]]} against {want[bad[:1]]}")
    return got


# ---- 1: every n = 1 .. 13 ----------------------------------------------------------------------------------------------------------
def _small_cases(n):
    """(select positions, target positions): 0 - 3 select qubits and k = 1, 2 at the low end, the high end, across index bits 5/6
    and 0/1; n = k and m + k = n among them"""
    top = n - 1
    cases = [([], [0])]
    if n >= 2:
        cases += [([], [1, 0]), ([], [0, top]), ([1], [0]), ([0], [1]), ([top], [0]), ([0], [top])]
    if n == 2:
        cases += [([], [0, 1])]
    if n >= 3:
        cases += [([2], [1, 0]), ([0, 2], [1]), ([top - 2], [top, top - 1]), ([top, top - 1], [top - 2]), ([1], [0, top]), ([0], [top, 1])]
    if n == 3:
        cases += [([1, 0], [2])]
    if n >= 4:
        cases += [([3, 0], [1, 2]), ([top, 1, 0], [top - 1]), ([2, top, 0], [1]), ([top - 1, 0], [top, 1])]
    if n >= 5:
        cases += [([4, 0, 2], [1, 3]), ([top, top - 4, top - 2], [top - 1, top - 3]), ([1, 0, top], [2]), ([3, 1, 4], [0, 2])]
    if n == 4:
        cases += [([3, 1], [2, 0])]
    if n >= 7:
        cases += [([4], [5, 6]), ([6, 5], [4]), ([5], [6]), ([6], [5, 0]), ([5, 0, 6], [1]), ([0, 1], [6, 5]), ([6, 4, 5], [top, 0])]
    if n >= 8:
        cases += [([4, 7], [6, 5]), ([5, 6, 1], [7, 0]), ([7, 1], [6]), ([0], [7, 6]), ([6, 7, 5], [0, 1]), ([1, 7, 0], [5])]
    cases = [c for c in cases if len(set(c[0] + c[1])) == len(c[0] + c[1])]  # (where "top" meets a fixed position the case is another's)
    assert all(p < n for c in cases for p in c[0] + c[1])
    return cases


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_every_small_n_bit_for_bit(dtype):
    rng = np.random.default_rng(21)
    count = specials = 0
    for n in range(1, 14):
        x = _state(n, dtype)
        with q.HipState(n, dtype) as st:
            for spos, tpos in _small_cases(n):
                select, targets = _qubits(n, spos), _qubits(n, tpos)
                m, k = len(select), len(targets)
                for kind in ("unitary", "scaled", "identities"):
                    if kind == "identities":
                        table, _ = R.with_identities(rng, R.unitary_table(rng, m, k), share=0.5)
                        if m == 0:
                            table = np.eye(2 ** k, dtype=np.complex128)[None]
                        y, hit = _with_specials(n, x, select, targets, table)
                        specials += hit
                    else:
                        table, y = R.TABLES[kind](rng, m, k), x
                    _run(st, n, y, select, targets, table, (n, spos, tpos, kind))
                    count += 1
    assert count >= 300 and specials > 0


# ---- 2: the placement matrix at n = 14 -------------------------------------------------------------------------------------------
_SELECT_PLACES = {"sel_row": [2, 1], "sel_outside": [11, 7, 10], "sel_mixed": [8, 1, 11, 2], "sel_none": []}  # (disjoint from every target place)
_TARGET_PLACES = {"t0": [0], "t5": [5], "t6": [6], "t13": [13], "t0_9": [0, 9], "t9_0": [9, 0], "t5_6": [5, 6], "t6_5": [6, 5],
                  "t3_4": [3, 4], "t4_3": [4, 3], "t12_13": [12, 13], "t13_12": [13, 12]}


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_placement_matrix_at_n14(dtype):
    n = 14
    x = _state(n, dtype)
    rng = np.random.default_rng(22)
    with q.HipState(n, dtype) as st:
        for sname, spos in _SELECT_PLACES.items():
            for tname, tpos in _TARGET_PLACES.items():
                table = R.unitary_table(rng, len(spos), len(tpos))
                got = _run(st, n, x, _qubits(n, spos), _qubits(n, tpos), table, (sname, tname))
                assert not _same_bits(got, x)
    # the two orders of a target pair are different maps of the same matrix
    table = R.unitary_table(rng, 2, 2)
    a = R.apply_multiplexed_spec(n, x, _qubits(n, [2, 1]), _qubits(n, [5, 6]), table)
    b = R.apply_multiplexed_spec(n, x, _qubits(n, [2, 1]), _qubits(n, [6, 5]), table)
    assert not np.array_equal(a, b)


# ---- 3: several blocks, several steps ---------------------------------------------------------------------------------------------
def _steps_and_blocks(n, spos, tpos):
    """steps and blocks of the launch, by the plan header's rule (qip_multiplex_plan.h: kMxLoads = 4 amplitudes of a lane in flight,
    kMxWaves = 4 waves per block, kMxFillBlocks = 256 blocks before a wave walks a second step, kMxMaxSteps = 8)"""
    kh = sum(p >= 6 for p in tpos)
    outer = [p for p in range(6, n) if p not in tpos]
    free = [p for p in outer if p not in spos]
    items = 2 ** len(outer)
    U = 4 >> kh
    if 2 ** len(free) < U:
        U = 1
    waves = min(4, items // U)
    steps = max(1, min(8, items // (U * waves * 256)))
    return steps, items // (U * waves * steps), len(free), U


_BIG_CASES = [
    # (target positions, select positions): m = 10 with select bits below and above the walked (lowest free outer) positions
    ([0], [6, 7, 3, 18, 17, 16, 15, 14, 13, 12]),
    ([9], [6, 1, 8, 18, 17, 16, 15, 14, 13, 11]),
    ([3, 10], [7, 6, 0, 18, 17, 16, 15, 14, 13, 12]),
    ([11, 8], [6, 7, 2, 18, 17, 16, 15, 14, 13, 12]),
    ([5, 4], [7, 6, 9, 18, 17, 16, 15, 14, 13, 0]),
    # m = 12: one free outer position, so the walk reaches into the select positions and the rows are fetched again at every step
    ([0], [6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17]),
]


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
@pytest.mark.parametrize("n", (19, 20))
def test_several_blocks_of_several_steps(dtype, n):
    """n = 19 is the smallest n at which a launch has more than one block AND a wave walks more than one step: a second step needs
    kMxFillBlocks = 256 blocks of kMxWaves = 4 waves with kMxLoads = 4 amplitudes in flight per lane, 2 * 256 * 4 * 4 * 64 = 2^19
    amplitudes, whatever the target placement (a target outside the row halves the items and doubles the amplitudes of one).
    n = 20 walks four steps."""
    x = _state(n, dtype)
    rng = np.random.default_rng(23 + n)
    with q.HipState(n, dtype) as st:
        for tpos, spos in _BIG_CASES:
            steps, blocks, free, U = _steps_and_blocks(n, spos, tpos)
            assert steps >= 2 and blocks >= 256, (n, tpos, steps, blocks)
            if len(spos) == 12:
                assert steps * U > 2 ** free  # the walk changes x
            table = R.unitary_table(rng, len(spos), len(tpos))
            _run(st, n, x, _qubits(n, spos), _qubits(n, tpos), table, (n, tpos, spos))
    for k in (1, 2):  # below n = 19 no placement walks a second step
        assert _steps_and_blocks(18, [], list(range(k)))[0] == 1 and _steps_and_blocks(18, [], [17, 16][:k])[0] == 1


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
@pytest.mark.parametrize("k", (1, 2))
def test_largest_table(dtype, k):
    """m + 2k = 20 at n = 20: 2^20 table entries, select bits inside the row, on walked positions and above them"""
    n, m = 20, 20 - 2 * k
    tpos = [0, 6][:k]
    free = [7, 19][: n - m - k]
    spos = [p for p in range(n) if p not in tpos and p not in free]
    assert len(spos) == m
    assert q.multiplexed_table_bytes(n, _qubits(n, spos), _qubits(n, tpos), dtype) == (16 if dtype == np.complex128 else 8) << 20
    rng = np.random.default_rng(24 + k)
    table = R.unitary_table(rng, m, k)
    with q.HipState(n, dtype) as st:
        _run(st, n, _state(n, dtype), _qubits(n, spos), _qubits(n, tpos), table, ("largest", k))


# ---- 4: one matrix per lane, one per wave -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
@pytest.mark.parametrize("k", (1, 2))
def test_one_matrix_per_lane_and_per_wave(dtype, k):
    n = 12
    rng = np.random.default_rng(25 + k)
    row = [3, 0, 5, 1, 4, 2]
    with q.HipState(n, dtype) as st:
        # per lane: the registers fill the row, every group of a wave has a matrix of its own
        tpos, spos = row[:k], row[k:]
        _run(st, n, _state(n, dtype), _qubits(n, spos), _qubits(n, tpos), R.unitary_table(rng, 6 - k, k), ("lane", k))
        tpos, spos = [7, 10][:k], row
        _run(st, n, _state(n, dtype), _qubits(n, spos), _qubits(n, tpos), R.unitary_table(rng, 6, k), ("lane, targets outside", k))
        # per wave: every position outside the row is a select position
        tpos = [2, 4][:k]
        spos = list(range(6, n))[::-1]
        _run(st, n, _state(n, dtype), _qubits(n, spos), _qubits(n, tpos), R.unitary_table(rng, n - 6, k), ("wave", k))
        tpos = [8, 2][:k]
        spos = [p for p in range(6, n) if p not in tpos]
        _run(st, n, _state(n, dtype), _qubits(n, spos), _qubits(n, tpos), R.unitary_table(rng, len(spos), k), ("wave, target outside", k))


# ---- 5: ordering -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_unsynchronised_calls_with_rewritten_tables(dtype):
    n, m = 14, 10
    spos, tpos = list(range(2, 12)), [13, 0]
    select, targets = _qubits(n, spos), _qubits(n, tpos)
    rng = np.random.default_rng(26)
    tables = [R.unitary_table(rng, m, 2) for _ in range(3)]
    x = _state(n, dtype)
    with q.HipState(n, dtype) as st:
        st.upload(x)
        work = np.empty((2 ** m, 4, 4), dtype=np.complex128)
        for t in tables:
            work[:] = t
            st.apply_multiplexed(select, targets, work)  # no synchronise in between
            work[:] = np.nan  # the caller's array is the caller's again
        got = st.download()
    want = x
    for t in tables:
        want = R.apply_multiplexed_spec(n, want, select, targets, t)
    assert _same_bits(got, want) and not _same_bits(got, x)


# ---- 6: identity halves --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_controlled_leaves_the_other_half_untouched(dtype):
    n = 12
    rng = np.random.default_rng(27)
    for controls, select, targets in (([0], [5, 11], [7]), ([9, 3], [0], [11, 2]), ([11], [], [10])):
        gates = R.unitary_table(rng, len(select), len(targets))
        j = np.arange(2 ** n, dtype=np.uint64)
        off = R.gather(n, j, controls) != 2 ** len(controls) - 1
        x = np.array(_state(n, dtype))
        x[np.flatnonzero(off)[0::5]] = complex(-0.0, np.inf)
        x[np.flatnonzero(off)[1::5]] = complex(-0.0, -0.0)
        with q.HipState(n, dtype) as st:
            st.upload(x)
            multiplex.controlled(st, controls, select, targets, gates)
            got = st.download()
        assert _same_bits(got[off], x[off])
        want = R.apply_multiplexed_spec(n, x, list(select) + list(controls), targets, multiplex.controlled_table(len(controls), gates))
        assert _same_bits(got, want) and not np.array_equal(got[~off], x[~off])


# ---- 7: refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_state_alone():
    n = 8
    x = _state(n, np.complex128)
    sel, tgt = (C.c_uint64 * 2)(0, 1), (C.c_uint64 * 2)(6, 7)
    ok = (C.c_double * 128)(*([0.5] * 128))
    bad = (C.c_double * 128)(*([0.5] * 77 + [float("nan")] + [0.5] * 50))
    inf = (C.c_double * 128)(*([0.5] * 8 + [float("inf")] + [0.5] * 119))
    many = (C.c_uint64 * 19)(*range(19))
    with q.HipState(n, np.complex128) as st:
        st.upload(x)

        def refused(*args):
            assert _ffi.lib.qipx_state_apply_multiplexed(st._h, *args) == _ffi.QIP_ERR_INVALID
            return _ffi.last_error()

        assert refused(sel, 2, (C.c_uint64 * 2)(6, 8), 2, ok) == "apply_multiplexed: qubit 8 out of range"
        assert refused((C.c_uint64 * 2)(0, 0), 2, tgt, 2, ok) == "apply_multiplexed: qubit 0 repeated"
        assert refused(sel, 2, (C.c_uint64 * 2)(6, 6), 2, ok) == "apply_multiplexed: qubit 6 repeated"
        assert refused(sel, 2, (C.c_uint64 * 2)(6, 1), 2, ok) == "apply_multiplexed: qubit 1 is in both registers"
        assert refused(sel, 2, tgt, 0, ok) == "apply_multiplexed: 0 target qubits, 1 or 2 are supported"
        assert refused(sel, 2, (C.c_uint64 * 3)(5, 6, 7), 3, ok) == "apply_multiplexed: 3 target qubits, 1 or 2 are supported"
        assert refused(many, 19, tgt, 1, ok) == "apply_multiplexed: 19 select and 1 target qubits, m + 2k is at most 20"
        assert refused(None, 2, tgt, 2, ok) == "apply_multiplexed: null qubit array"
        assert refused(sel, 2, None, 2, ok) == "apply_multiplexed: null qubit array"
        assert refused(sel, 2, tgt, 2, None) == "apply_multiplexed: null matrix array"
        assert refused(sel, 2, tgt, 2, bad) == "apply_multiplexed: entry 6 of matrix 2 is not finite"
        assert refused(sel, 2, tgt, 2, inf) == "apply_multiplexed: entry 4 of matrix 0 is not finite"
        with pytest.raises(q.CircuitError, match=r"matrices of shape \(3, 2, 2\)"):
            st.apply_multiplexed([0, 1], [6], np.zeros((3, 2, 2)))
        assert _same_bits(st.download(), x)


# ---- 8: a relabelled state -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_relabelled_state(dtype):
    """tile = 1 with tile_relabel = 3 at n = 15 (the function tests' recipe): the batch leaves the qubits relabelled and the call
    restores the caller's order first"""
    n = 15
    ops = circuits.c2_random_circuit(n, 80, seed=41)
    select, targets = [0, 9, 14], [3, 13]
    table = R.unitary_table(np.random.default_rng(28), 3, 2)
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
        st.apply_multiplexed(select, targets, table)
        assert st.profile().get("k_permute_bits", {}).get("launches", 0) >= 1, "the batch left no layout to restore"
        y = twin.download()
        twin.apply_multiplexed(select, targets, table)
        assert st.max_abs_diff(twin) == (0.0, 0)
        assert _same_bits(twin.download(), R.apply_multiplexed_spec(n, y, select, targets, table))


# ---- 9: rustqip_amd.multiplex ----------------------------------------------------------------------------------------------------------
def _controlled_route(st, select, target, gates):
    """the same map as 2^m controlled gates through apply_op, X-conjugated where a select bit reads 0"""
    for xv, g in enumerate(gates):
        flips = [q.make_matrix_op([s], circuits.X) for i, s in enumerate(select) if not (xv >> i) & 1]
        op = q.make_matrix_op([target], g)
        for f in flips:
            st.apply_op(f)
        st.apply_op(q.make_control_op(list(select), op) if select else op)
        for f in flips:
            st.apply_op(f)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_rotation_is_the_controlled_rotations(dtype):
    """per amplitude relative to its group's norm: (1.5 M + 3) u = 6 u of the call, and 6 u of the controlled route, whose
    one-qubit kernels form the same four products and two sums per term from the same rounded matrix (include/qip_hip.h: the
    reference's unfused arithmetic) — every amplitude meets ONE rotation on that route too, the X gates only move it"""
    n = 11
    u = R.UNIT[dtype]
    rng = np.random.default_rng(29)
    x = _state(n, dtype)
    for axis in "xyz":
        for select, target in (([], 10), ([10], 0), ([3, 9], 10), ([0, 10, 4], 6), ([7, 8, 9], 5)):
            angles = rng.uniform(-6, 6, size=2 ** len(select))
            with q.HipState(n, dtype) as st, q.HipState(n, dtype) as twin:
                st.upload(x)
                multiplex.rotation(st, axis, select, target, angles)
                twin.upload(x)
                _controlled_route(twin, select, target, multiplex.rotation_matrices(axis, angles))
                got, want = st.download(), twin.download()
            ratio = float(np.max(np.abs(got.astype(np.complex128) - want.astype(np.complex128)) / (u * R.group_norms(n, x, [target]))))
            print(f"R{axis} m={len(select)} target {target}: worst |call - controlled route| = {ratio:.2f} u |v| (bar 12)")
            assert ratio <= 12.0, (axis, select, target)
            assert not np.array_equal(got, x)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
def test_batch_of_parameter_sets_is_eight_separate_states(dtype):
    """n = 10 with 3 batch qubits on top: member b of the batch is rotated by angles[b], as a 7-qubit state of its own is through
    apply_op (the bar of the rotation test)"""
    n, nb = 10, 3
    u = R.UNIT[dtype]
    rng = np.random.default_rng(30)
    members = [R.make_state(n - nb, 60 + b, dtype) for b in range(2 ** nb)]
    batch_qubits = [2, 1, 0]  # bit i of the member number = qubit batch_qubits[i]: the member number is the top of the index
    angles = rng.uniform(-3, 3, size=(3, 2 ** nb))
    for layer, (axis, target) in enumerate((("y", 9), ("x", 3), ("z", 6))):
        with q.HipState(n, dtype) as st:
            st.upload(np.concatenate(members))
            multiplex.rotation(st, axis, batch_qubits, target, angles[layer])
            got = st.download().reshape(2 ** nb, -1)
        worst = 0.0
        for b, member in enumerate(members):
            with q.HipState(n - nb, dtype) as one:
                one.upload(member)
                one.apply_op(q.make_matrix_op([target - nb], multiplex.rotation_matrices(axis, [angles[layer][b]])[0]))
                want = one.download()
            err = np.abs(got[b].astype(np.complex128) - want.astype(np.complex128)) / (u * R.group_norms(n - nb, member, [target - nb]))
            worst = max(worst, float(err.max()))
            assert not np.array_equal(got[b], member)
        print(f"R{axis} on qubit {target}: worst |batch member - separate state| = {worst:.2f} u |v| (bar 12)")
        assert worst <= 12.0, (axis, worst)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_IDS)
@pytest.mark.parametrize("k", (1, 4, 8))
def test_prepare_register_embedded(dtype, k):
    """a register of k qubits among 3 others that hold a state of their own: after the Ry passes the download is bit-equal to the
    CPU chain of spec passes; the final state is within (9k + 8) u of (amplitudes on the register) x (the others' state)"""
    n = k + 3
    u = R.UNIT[dtype]
    rng = np.random.default_rng(31 + k)
    psi = R.random_amplitudes(rng, k, zero_branch=k >= 4)
    perm = rng.permutation(n)
    qubits, others = [int(v) for v in perm[:k]], [int(v) for v in perm[k:]]
    rest = R.make_state(3, 70 + k, np.complex128)
    j = np.arange(2 ** n, dtype=np.uint64)
    r, o = R.gather(n, j, qubits).astype(np.int64), R.gather(n, j, others).astype(np.int64)
    x0 = np.where(r == 0, rest[o], 0).astype(dtype)
    want = psi[r] * x0.astype(np.complex128)[(j & ~F.scatter(n, np.full_like(j, 2 ** k - 1), qubits)).astype(np.int64)]
    angles, phases = multiplex.prepare_tables(psi)
    with q.HipState(n, dtype) as st:
        st.upload(x0)
        chain = x0
        for i, th in enumerate(angles):
            multiplex.rotation(st, "y", qubits[:i], qubits[i], th)
            chain = R.apply_multiplexed_spec(n, chain, qubits[:i], [qubits[i]], multiplex.rotation_matrices("y", th))
        assert _same_bits(st.download(), chain)
        st.upload(x0)
        multiplex.prepare_register(st, qubits, psi)
        got = st.download()
    err = float(np.linalg.norm(got.astype(np.complex128) - want) / (u * np.linalg.norm(want)))
    print(f"k = {k}: |got - psi x rest|_2 = {err:.2f} u (bar {9 * k + 8})")
    assert err <= 9 * k + 8
