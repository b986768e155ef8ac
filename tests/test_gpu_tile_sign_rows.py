"""Dense 1-qubit gates whose second row is the first up to one sign per column (H, H.X after an absorbed X, Ry(pi/2)) in the
interpreter's tile sweeps: k_tile_passes forms both rows of such a gate of real entries from row 0's products (pass_dense_signs;
marked on the host by tile_mark_sign_rows).  The results are what they were, bit for bit: against the CPU oracle applying the ops
one by one, and against one launch per gate (pair_floor = 0, tile = 0).  The host half: tests/test_tile_sign_rows_cpu.py."""
import cmath

from gpu_common import *  # noqa: F401,F403

from oracle import window_parity as W

pytestmark = pytest.mark.gpu

N = 13
X, H = circuits.X, circuits.H
A, B = 0.6, 0.8
CA, CB = 0.3 + 0.4j, 0.5 - 0.2j
RZ = [cmath.rect(1, -0.35), 0, 0, cmath.rect(1, 0.35)]
SIGNED = [[A, B, A, -B], [A, B, -A, B], [A, B, -A, -B], [A, B, A, B], [CA, CB, -CA, CB]]


def _m(bit, mat, n=N):
    return q.make_matrix_op([n - 1 - bit], mat)


def _c(cbits, op, n=N):
    return q.make_control_op([n - 1 - b for b in cbits], op)


CIRCUITS = {
    "h_on_three_pass_bits": [_m(7, H), _m(9, H), _m(12, H)],  # one pass, J = 0, 1, 2
    "h_on_rows": [_m(0, H), _m(3, H), _m(5, H)],
    "x_rz_h": [_m(8, X), _m(3, RZ), _m(8, H)],  # H.X: first column negated
    "sign_patterns_low_and_high": [_m(b, m) for m in SIGNED for b in (2, 10)],
    "control_on_a_pass_bit": [_m(9, H), _c([9], _m(10, H)), _m(10, H), _c([9], _m(11, X)), _m(9, H)],  # cm != 0: the generic body
    "random40": circuits.c2_random_circuit(N, 40, seed=28, single_only=True),
}


def _run(ops, dtype, **options):
    with q.HipState(N, dtype) as st:
        for k, v in options.items():
            st.set_option(k, v)
        st.init_basis(0)
        st.apply_ops(W.product_state_ops(N, seed=N)[0])  # distinct, non-uniform amplitudes
        start = st.download()
        st.set_option("profile", 1)
        st.profile_reset()
        st.apply_ops(ops)
        prof = st.profile()
        return start, st.download(), prof


@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_tile_sweep_is_bit_equal_to_the_oracle_and_to_gate_by_gate(O, name, dtype):
    ops = CIRCUITS[name]
    start, got, prof = _run(ops, dtype, tile=1)
    assert prof.get("k_tile_passes", {}).get("launches", 0) >= 1, prof
    assert got.dtype == dtype and np.array_equal(got, O.apply_ops_in_place(N, ops, start.copy()))
    start0, gbg, _ = _run(ops, dtype, pair_floor=0, tile=0)
    assert np.array_equal(start0, start) and np.array_equal(got, gbg)


def test_default_route_is_bit_equal_to_gate_by_gate():
    n = 22
    ops = circuits.c2_random_circuit(n, 256, seed=28, single_only=True)[:64]  # the first 64 gates of bench.py's headline
    states = []
    for floor in (None, 0):
        st = q.HipState(n, np.complex128)
        if floor is not None:
            st.set_option("pair_floor", floor)
        st.init_basis(0)
        st.apply_ops(W.product_state_ops(n, seed=n)[0])
        st.set_option("profile", 1)
        st.profile_reset()
        st.apply_ops(ops)
        states.append((st, st.profile()))
    (fused, prof), (gbg, _) = states
    try:
        assert prof.get("k_tile_passes", {}).get("launches", 0) >= 2, prof  # default options: the default fused route
        assert np.array_equal(fused.download(), gbg.download())
    finally:
        fused.close()
        gbg.close()
