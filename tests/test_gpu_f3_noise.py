"""Noise channels on a device state by quantum trajectories (include/qip_hipx.h: qipx_state_apply_reduce,
qipx_state_apply_channels; HipState.apply_reduce / apply_channels; rustqip_amd.noise) against tests/noise_ref.py, on Complex<f64>
and Complex<f32> states.

Bars (the project's own statements, none taken from the code under test):
  rho_next   every entry within 1e-12 sqrt(rho[a][a] rho[a'][a']) of the reference density of the reference result (the bar of
             tests/test_gpu_f2_reduced_density.py); Complex<f32>: against the float64 density of the DOWNLOADED f32 result
  state      within 1e-12 |A| |psi| per amplitude (|A| the spectral norm), 1e-5 |A| |psi| for Complex<f32>
  exact      rho_next Hermitian bit for bit with +0.0 diagonal imaginary parts; equal calls give equal bits; the identity leaves the
             state's bits; a permuted index list gives the bit-exact row / column permutation
  channels   `chosen` equals the reference's choice, the uniforms being seeded so that in the reference every u * W lies at least
             1e-6 W away from every cumulative boundary (asserted); the final state within the state bar per channel applied;
             norm_sqr preserved to 1e-12 (1e-5) per channel.
             weights within 1e-12 N for every channel and both precisions, N = tr rho of the state the channel meets.  The
             reference for channel j is the float64 quantity of the DOWNLOADED state that channel j meets (the rule of rho_next
             above): w_i = Re Tr(K_i^H K_i rho) from reduced_density_ref on that download.  That state is observed by running the
             chain's first j channels followed by the identity as a plain gate on channel j's qubits: the step into it has the
             union and the route of the full chain's step, its one branch has weight tr rho exactly, so the scale is 1 and the
             identity moves nothing.  Nothing here asks the code under test for its plan.

Which size runs which regime of k_apply_density_small (positions in 16-byte elements; a packed Complex<f32> element is two
amplitudes, so its positions are one less and amplitude position 0 is the half of the element):
  n = 3    G = every qubit (k = n): one group per lane, idle lanes hold zeros
  n = 7    128 amplitudes: Complex<f64> two rows, Complex<f32> one row of 64 elements; sets with an opened high position leave fewer
           than 64 work items (nlane < 64)
  n = 14   several blocks and the block fold; all-high sets, one, two and three lane-id bits, bit 0, the 5 / 6 boundary
  n = 23   Complex<f64>, |G| <= 2: 2^16 / 2^15 rows on 4096 blocks of four waves, so a lane's loop runs twice (the accumulators are
           carried over, the second round of loads and stores runs); |G| = 3 at this size is one round.  Packed Complex<f32> has
           half the rows: its two-round case is n = 24.  The test derives the number of rounds from the geometry and asserts it."""
from gpu_common import *  # noqa: F401,F403

import noise_ref as NR
import reduced_density_ref as D
from rustqip_amd import noise

pytestmark = pytest.mark.gpu

_IDS = ("c128", "c64")
_STATES = {}


def _state(n, dtype):
    key = (n, np.dtype(dtype))
    if key not in _STATES:
        x = D.make_state(n, D.seed_of(n, dtype) + 77, dtype)
        x.setflags(write=False)
        _STATES[key] = x
    return _STATES[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _tol(dtype):
    return TOL64 if np.dtype(dtype) == np.complex128 else TOL32


def _matrix(kind, k, seed):
    m = 1 << k
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((m, m)) + 1j * rng.standard_normal((m, m))
    if kind == "diagonal":
        a = np.diag(np.diag(a))
    elif kind == "projector":  # a projector with a zero row (and column): |0><0| on the lowest bit
        a = np.kron(np.eye(m // 2), np.diag([1.0, 0.0])).astype(np.complex128)
    elif kind == "identity":
        a = np.eye(m, dtype=np.complex128)
    return a


KINDS = ("random", "diagonal", "projector", "identity")

# (positions acted on, positions reduced next): amplitude-index positions, in the order handed to the call
GEOMETRY = {
    3: [([0, 1], [1, 2]), ([2, 0], [1]), ([1], [0, 2]), ([2, 1], [2, 1]), ([0], [0]), ([1, 2], [2]), ([2], [0, 1]), ([1, 0], [0, 1]), ([2], [1])],
    7: [([6, 3], [3, 0]), ([6], [5, 4]), ([3, 1], [2]), ([0], [0]), ([6], [6]), ([6, 2], [2, 6]), ([5], [6]), ([0, 6], [3]),
        ([4, 5], [5]), ([1], [0, 1]), ([2, 0], [1, 0])],
    14: [([13, 9], [9, 7]),      # all high
         ([13], [8, 2]),         # one lane bit, disjoint 1 + 2
         ([12, 3], [1]),         # two lane bits
         ([5, 4], [4, 2]),       # three lane bits, overlapping pairs, reversed lists
         ([0, 13], [7]),         # bit 0 with high positions, disjoint 2 + 1
         ([1, 0], [0, 1, ][::-1]),  # A = B, the lists in opposite orders
         ([2], [0, 2]),          # A inside B
         ([6, 7], [6]),          # B inside A, the 5 / 6 boundary of both element sizes
         ([0], [0]), ([9], [9]), ([5], [6]), ([11], [3]),  # 1 + 1: equal and disjoint
         ([10, 0], [5, 10]), ([7, 12], [12, 7]), ([3, 9], [0])],
    23: [([22, 3], [3, 10])],
}


def _reduce_case(st, n, dtype, apos, bpos, kind, seed):
    x = _state(n, dtype)
    a, b = D.qubits(n, apos), D.qubits(n, bpos)
    m = _matrix(kind, len(a), seed)
    what = f"n={n} {np.dtype(dtype).name} A={apos} B={bpos} {kind}"
    st.upload(x)
    rho = st.apply_reduce(a, m, b)
    y = st.download()
    ref_y, ref_rho = NR.apply_reduce(n, a, m, b, x)
    norm_a, norm_x = float(np.linalg.norm(m, 2)), float(np.linalg.norm(x.astype(np.complex128)))
    err = float(np.max(np.abs(y.astype(np.complex128) - ref_y)))
    if np.dtype(dtype) == np.complex64:
        ref_rho = D.density_ref(n, b, y)  # the float64 density of the downloaded f32 result
    worst = D.worst_ratio(rho, ref_rho)
    print(f"{what}: state err / (|A||psi|) = {err / (norm_a * norm_x):.3e}, rho worst / bar = {worst:.3e}")
    assert err <= _tol(dtype) * norm_a * norm_x, what
    assert rho.dtype == np.complex128 and rho.shape == ref_rho.shape and worst <= 1.0, what
    assert D.exact_structure(rho), what
    if kind == "identity":
        assert np.array_equal(_bits(y), _bits(x)), what
    if kind == "projector":  # an entry all of whose products are zero is exactly zero
        assert np.all(y[np.abs(ref_y) == 0] == 0), what
    # equal calls, equal bits
    st.upload(x)
    rho2 = st.apply_reduce(a, m, b)
    y2 = st.download()
    assert np.array_equal(_bits(rho), _bits(rho2)) and np.array_equal(_bits(y), _bits(y2)), what
    # permuted lists: the bit-exact permutation, the same state
    if len(a) == 2 or len(b) == 2:
        pa, pb = ([1, 0] if len(a) == 2 else [0]), ([1, 0] if len(b) == 2 else [0])
        st.upload(x)
        rho3 = st.apply_reduce([a[i] for i in pa], D.permuted(m, pa), [b[i] for i in pb])
        assert np.array_equal(_bits(rho3), _bits(D.permuted(rho, pb))), what
        assert np.array_equal(_bits(st.download()), _bits(y)), what


@pytest.mark.parametrize("dtype", D.DTYPES, ids=_IDS)
@pytest.mark.parametrize("n", (3, 7, 14))
def test_apply_reduce_geometry(n, dtype):
    with q.HipState(n, dtype) as st:
        for i, (apos, bpos) in enumerate(GEOMETRY[n]):
            for kind in KINDS:
                _reduce_case(st, n, dtype, apos, bpos, kind, 100 * n + i)


@pytest.mark.parametrize("dtype", D.DTYPES, ids=_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_apply_reduce_every_kind_on_three_lane_bits_and_bit_zero(kind, dtype):
    """the largest groups (|G| = 3) with every matrix kind: lane bits only, and bit 0 with a lane bit and a walked position"""
    n = 14
    with q.HipState(n, dtype) as st:
        _reduce_case(st, n, dtype, [5, 4], [4, 2], kind, 7)
        _reduce_case(st, n, dtype, [0, 9], [3, 0], kind, 8)
        _reduce_case(st, n, dtype, [12, 10], [8], kind, 9)


def _rounds(n, dtype, positions):
    """how often a wave's loop runs for the union `positions` on an n-qubit state, from the geometry as include/qip_hipx.h and
    csrc/qip_kernels.h state it: rows of 64 work items, at most 4096 blocks of four waves, a wave takes 2^(lane-id positions) rows
    (at least four loads) per round"""
    packed = np.dtype(dtype) == np.complex64 and n >= 2
    pe = [p - 1 if packed else p for p in sorted(set(positions)) if not (packed and p == 0)]
    ke, kl = len(pe), sum(1 for p in pe if p < 6)
    items = 1 << ((n - 1 if packed else n) - (ke - kl))
    nrows = max(items >> 6, 1)
    per_round = (1 << kl) * (1 if (1 << ke) >= 4 else 4 >> ke)
    blocks = min(max(nrows // (per_round * 4), 1), 4096)
    return -(-nrows // (blocks * 4 * per_round))


@pytest.mark.parametrize("dtype,n", list(zip(D.DTYPES, (23, 24))), ids=_IDS)
def test_apply_reduce_many_rounds_per_lane(dtype, n):
    """the grid-stride loop: accumulators carried across rounds, the second round of loads and stores"""
    top = n - 1
    cases = [([top], [top], "random"), ([top], [10], "random"), ([3, top], [3], "diagonal"), ([0], [4], "random")]
    with q.HipState(n, dtype) as st:
        for apos, bpos, kind in cases:
            assert _rounds(n, dtype, apos + bpos) >= 2, (n, apos, bpos)
            _reduce_case(st, n, dtype, apos, bpos, kind, n)
        if n == 23:
            for apos, bpos in GEOMETRY[23]:  # |G| = 3: one round at this size
                _reduce_case(st, n, dtype, apos, bpos, "random", 23)


@pytest.mark.parametrize("dtype", D.DTYPES, ids=_IDS)
def test_apply_reduce_on_one_and_two_qubits(dtype):
    """n = 1: a Complex<f32> state of one qubit is a lone 8-byte element (the only unpacked one of the product build); n = 2: one
    packed element per value of position 1"""
    for n, cases in ((1, [([0], [0])]), (2, [([0], [1]), ([1, 0], [0]), ([1], [1, 0]), ([0, 1], [1, 0])])):
        with q.HipState(n, dtype) as st:
            for i, (apos, bpos) in enumerate(cases):
                for kind in KINDS:
                    _reduce_case(st, n, dtype, apos, bpos, kind, 10 * n + i)


# ---- chains ---------------------------------------------------------------------------------------------------------------------
def _h():
    return np.array([[1, 1], [1, -1]], dtype=np.complex128) / np.sqrt(2.0)


def _cz_like():
    return np.diag([1, 1j, -1, np.exp(0.3j)]).astype(np.complex128)


def chain(n, length):
    """(channels, uniforms): chains of 1, 2 and 6 channels that mix 1- and 2-qubit channels and count = 1 gates; the 6-chain
    'mixed' has one step whose union is four qubits (the unfused route); 'pairs' has unions of at most two qubits only"""
    top = n - 1
    if length == 1:
        chans = [noise.depolarizing([top, 0], 0.4)]
    elif length == 2:
        chans = [noise.amplitude_damping(top, 0.35), noise.depolarizing([0, top], 0.5)]
    elif length == 6:
        chans = [noise.amplitude_damping(0, 0.3), noise.gate([0, 1], _cz_like()), noise.depolarizing([1, 2], 0.45),
                 noise.phase_damping(top, 0.5), noise.gate([top], _h()), noise.generalized_amplitude_damping(top - 1, 0.4, 0.3)]
    elif length == "pairs":  # 7 channels, every union of at most two qubits: every step fuses in both precisions
        chans = [noise.amplitude_damping(0, 0.3), noise.depolarizing([0, 1], 0.45), noise.gate([1], _h()), noise.gate([top, 1], _cz_like()),
                 noise.phase_damping(top, 0.5), noise.generalized_amplitude_damping(top, 0.4, 0.3), noise.bit_flip(top, 0.2)]
    else:  # "mixed": 6 channels, the second and third cover four qubits together (the only such step)
        chans = [noise.bit_flip(top, 0.3), noise.depolarizing([top, 3], 0.5), noise.depolarizing([1, 2], 0.6),
                 noise.depolarizing([1, top], 0.5), noise.gate([0], _h()), noise.pauli_channel(2, 0.2, 0.3, 0.1)]
    us = np.random.default_rng(1000 * n + 10 * len(chans) + {"mixed": 5, "pairs": 2}.get(length, 0)).random(len(chans))
    return chans, us


def _incoming_states(n, dtype, chans, us, x, opts):
    """[the stored state that channel j of the chain meets], downloaded (the module docstring says how it is observed)"""
    out = [np.asarray(x)]
    with q.HipState(n, dtype) as st:
        for key, value in opts.items():
            st.set_option(key, value)
        for j in range(1, len(chans)):
            ident = noise.gate(chans[j].qubits, np.eye(1 << len(chans[j].qubits)))
            st.upload(x)
            chosen, ws = st.apply_channels(list(chans[:j]) + [ident], list(us[:j]) + [0.5])
            out.append(st.download())
            assert chosen[j] == 0 and len(ws[j]) == 1
    return out


def _run_chain(st, n, dtype, chans, us, x, what, opts=None):
    f32 = np.dtype(dtype) == np.complex64
    pairs = [(c.qubits, c.kraus) for c in chans]
    ref = NR.trajectory(n, pairs, x, us, store=np.complex64 if f32 else None)
    chosen_ref, ws_ref, y_ref = ref.chosen, ref.weights, ref.state
    print(f"{what}: smallest margin {ref.margin:.3e}")
    assert ref.margin >= NR.MARGIN, what  # (the uniforms were picked for this: no case may be skipped)
    n0 = st.norm_sqr()
    chosen, ws = st.apply_channels(chans, us)
    y = st.download()
    assert list(chosen) == chosen_ref, what
    for c, met in enumerate(_incoming_states(n, dtype, chans, us, x, opts or {})):
        rho = D.density_ref(n, chans[c].qubits, met)
        want, bar = NR.weights(chans[c].kraus, rho), 1e-12 * float(np.real(np.trace(rho)))
        print(f"  channel {c}: |w - ref| max {float(np.max(np.abs(ws[c] - want))):.3e}, bar {bar:.3e}")
        assert np.max(np.abs(ws[c] - want)) <= bar, (what, c)
    # the state bar per channel applied: channel c adds tol |A_c| |psi| and the later operators carry it on by at most their norms
    norms = [float(np.linalg.norm(op, 2)) for op in ref.applied]
    bar = sum(_tol(dtype) * float(np.prod([max(a, 1.0) for a in norms[c:]])) for c in range(len(chans))) * np.sqrt(n0)
    err = float(np.max(np.abs(y.astype(np.complex128) - y_ref)))
    print(f"  final state err {err:.3e}, bar {bar:.3e}")
    assert err <= bar, what
    assert abs(st.norm_sqr() - n0) <= _tol(dtype) * len(chans) * n0, what
    return chosen, ws, y


@pytest.mark.parametrize("dtype", D.DTYPES, ids=_IDS)
@pytest.mark.parametrize("length", (1, 2, 6, "mixed", "pairs"))
@pytest.mark.parametrize("n", (7, 14))
def test_apply_channels(n, length, dtype):
    chans, us = chain(n, length)
    x = _state(n, dtype)
    with q.HipState(n, dtype) as st:
        st.upload(x)
        chosen, ws, y = _run_chain(st, n, dtype, chans, us, x, f"n={n} {length} {np.dtype(dtype).name}")
        st.upload(x)
        chosen2, ws2 = st.apply_channels(chans, us)
        assert np.array_equal(chosen, chosen2) and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(ws, ws2))
        assert np.array_equal(_bits(st.download()), _bits(y))
    want = (len(chans) + 1, len(chans) - 1) if length != "mixed" else (len(chans) + 2, len(chans) - 2)
    assert q.channel_passes(n, chans) == want  # (the plan of a Complex<f64> state)


@pytest.mark.parametrize("dtype", D.DTYPES, ids=_IDS)
def test_apply_channels_on_a_relabelled_state(dtype):
    """tile_relabel = 3 leaves a layout after apply_ops; the call puts the caller's order back first"""
    n = 14
    ops = circuits.c2_random_circuit(n, 60, seed=43)
    chans, us = chain(n, 6)
    with q.HipState(n, dtype) as st:
        st.set_option("tile", 1)
        st.set_option("tile_relabel", 3)
        st.set_option("profile", 1)
        st.upload(_state(n, dtype))
        st.apply_ops(ops)
        with q.HipState(n, dtype) as twin:
            twin.upload(_state(n, dtype))
            twin.set_option("tile", 1)
            twin.set_option("tile_relabel", 3)
            twin.apply_ops(ops)
            x = twin.download()  # (a download restores the caller's order, and a restored layout moves amplitudes exactly)
        st.profile_reset()
        _run_chain(st, n, dtype, chans, us, x, f"relabelled {np.dtype(dtype).name}", opts={"tile": 1, "tile_relabel": 3})
        assert st.profile().get("k_permute_bits", {}).get("launches", 0) >= 1, "the batch left no layout to restore"


@pytest.mark.parametrize("dtype", D.DTYPES, ids=_IDS)
def test_zero_weight_branches_and_the_ends_of_the_unit_interval(dtype):
    n = 7
    decay = noise.amplitude_damping(2, 0.4)
    flipped = noise.Channel([2], decay.kraus[::-1])  # the decay operator first: weight exactly zero on |0>
    below_one = float(np.nextafter(1.0, 0.0))
    with q.HipState(n, dtype) as st:
        for ch, u, want in ((decay, below_one, 0), (decay, 1.0, 0), (flipped, 0.0, 1), (flipped, 0.5, 1)):
            st.init_basis(0)
            chosen, ws = st.apply_channels([ch, noise.gate([3], np.eye(2))], [u, 0.5])
            assert list(chosen) == [want, 0] and ws[0][1 - want] == 0.0 and ws[0][want] == 1.0, (u, want)
            y = st.download()
            assert y[0] == 1 and not np.any(y[1:])
        # |1> on qubit 2: both branches have weight; u = 0 takes the first, u just below 1 the last
        for u, want in ((0.0, 0), (below_one, 1)):
            st.init_basis(1 << (n - 1 - 2))
            chosen, ws = st.apply_channels([decay], [u])
            assert list(chosen) == [want] and abs(ws[0][0] - 0.6) < 1e-15 and abs(ws[0][1] - 0.4) < 1e-15
        # a channel that annihilates the state is refused and the state stays as the preceding channels left it
        st.init_basis(0)
        lower = noise.Channel([2], [[[0, 1], [0, 0]]])
        with pytest.raises(q.CircuitError, match="no branch"):
            st.apply_channels([noise.gate([0], [[0, 1], [1, 0]]), lower], [0.5, 0.5])
        y = st.download()
        assert y[1 << (n - 1)] == 1 and np.count_nonzero(y) == 1


@pytest.mark.parametrize("dtype", D.DTYPES, ids=_IDS)
def test_pass_count(dtype):
    """the profile agrees with the plan: Complex<f64> fuses every step of the 6-chain (5 launches of the new class, one density
    pass, one dense apply); Complex<f32> runs its two steps of three qubits composed (profiles/noise.md), so its fused path
    inside apply_channels runs on unions of at most two qubits: the chain 'pairs' has only those and fuses all six steps in
    both precisions"""
    n = 14
    f32 = np.dtype(dtype) == np.complex64
    for length, want in ((6, (9, 3) if f32 else (7, 5)), ("mixed", (10, 2) if f32 else (8, 4)), ("pairs", (8, 6))):
        chans, us = chain(n, length)
        with q.HipState(n, dtype) as st:
            st.upload(_state(n, dtype))
            st.set_option("profile", 1)
            st.profile_reset()
            st.apply_channels(chans, us)
            prof = st.profile()
            plan = st.channel_passes(chans)
        print(length, plan, prof)
        assert plan == want, (length, plan)
        passes, fused = plan
        unfused = len(chans) - 1 - fused
        assert prof.get("k_apply_density_small", {}).get("launches", 0) == fused, prof
        assert prof["reduced_density"]["launches"] == 1 + unfused, prof
        others = {k: v["launches"] for k, v in prof.items() if k not in ("k_apply_density_small", "reduced_density")}
        assert sum(others.values()) == 1 + unfused, prof  # the dense applies: the unfused steps and the last channel
        assert passes == fused + 2 * unfused + 2
    assert q.channel_passes(n, chain(n, 6)[0]) == (7, 5)


@pytest.mark.parametrize("dtype", D.DTYPES, ids=_IDS)
def test_amplitude_damping_of_all_ones_trajectory_by_trajectory(dtype):
    """n = 10, 64 seeded trajectories of a 10-channel amplitude-damping chain on |1...1>: every trajectory is a basis state, and
    it is the reference's, trajectory by trajectory (exact, not statistical)"""
    n, shots = 10, 64
    chans = [noise.amplitude_damping(qb, 0.1 + 0.08 * qb) for qb in range(n)]
    pairs = [(c.qubits, c.kraus) for c in chans]
    start = np.zeros(1 << n, dtype=np.complex128)
    start[-1] = 1.0
    seen = set()
    with q.HipState(n, dtype) as st:
        for t in range(shots):
            us = np.random.default_rng([2024, t]).random(n)
            ref = NR.trajectory(n, pairs, start, us)
            chosen_ref, y_ref = ref.chosen, ref.state
            assert ref.margin >= NR.MARGIN, t
            st.init_basis((1 << n) - 1)
            chosen, _ = noise.trajectory(st, chans, [2024, t])
            pops = st.measure_probs(list(range(n)))  # bit i of the outcome = qubit i
            at = int(np.argmax(np.abs(y_ref)))
            outcome = sum(((at >> (n - 1 - qb)) & 1) << qb for qb in range(n))
            assert list(chosen) == chosen_ref and np.count_nonzero(y_ref) == 1, t
            assert np.count_nonzero(pops) == 1 and abs(pops[outcome] - 1.0) <= _tol(dtype) * n, (t, outcome)
            assert outcome == sum((1 - i) << qb for qb, i in enumerate(chosen_ref)), t  # a decay (branch 1) empties its qubit
            seen.add(outcome)
    assert len(seen) > 16  # the trajectories differ


def test_average_over_trajectories_runs_one_state_at_a_time():
    n = 4
    chans = [noise.amplitude_damping(qb, 0.5) for qb in range(n)]

    def make():
        st = q.HipState(n, np.complex128)
        st.init_basis((1 << n) - 1)
        return st

    mean = noise.average(lambda st: st.measure_probs([0]), make, chans, shots=8, seed=5)
    assert mean.shape == (2,) and abs(float(np.sum(mean)) - 1.0) < 1e-12
    again = noise.average(lambda st: st.measure_probs([0]), make, chans, shots=8, seed=5)
    assert np.array_equal(mean, again)


@pytest.mark.parametrize("dtype", D.DTYPES, ids=_IDS)
def test_refusals(dtype):
    n = 7
    x = _state(n, dtype)
    eye2, eye4 = np.eye(2), np.eye(4)
    with q.HipState(n, dtype) as st:
        st.upload(x)
        with pytest.raises(q.QipHipError, match="status 4"):
            st.apply_reduce([0, 1, 2], np.eye(8), [0])  # k = 3
        with pytest.raises(q.QipHipError, match=r"status 4.*\[0, 1\].*\[2, 3\]"):
            st.apply_reduce([0, 1], eye4, [2, 3])  # a union of four: the message names both lists
        for a, m, b in (([1, 1], eye4, [0]), ([0], eye2, [2, 2]), ([7], eye2, [0]), ([], np.eye(1), [0]), ([0], eye2, [])):
            with pytest.raises(q.CircuitError):
                st.apply_reduce(a, m, b)
        with pytest.raises(q.CircuitError):
            st.apply_channels([([0], np.zeros((0, 2, 2)))], [0.5])  # count = 0
        with pytest.raises(q.CircuitError):
            st.apply_channels([([0], np.stack([eye2] * 17))], [0.5])  # count = 17
        with pytest.raises(q.CircuitError):
            st.apply_channels([([0], eye2), ([3, 3], eye4)], [0.5, 0.5])  # refused before the first channel runs
        with pytest.raises(q.CircuitError):
            st.apply_channels([([0], eye2)], [1.5])
        assert np.array_equal(_bits(st.download()), _bits(x))  # nothing was touched
