"""The multiplexed gate (include/qip_hipx.h: qipx_state_apply_multiplexed) on handles that wrap caller memory and caller streams.

Handle forms (tests/wrapped_common.py): owned, W1 and W2, at n = 15 and at n = 1, Complex<f64> and Complex<f32>.  The call is held
  * bit for bit to tests/multiplex_ref.py's apply_multiplexed_spec, applied to the owned twin;
  * bit for bit to the owned twin on W1 and W2: the route does not depend on who owns the buffers or the stream;
  * to intact guard zones and the buffer contract (device_ptr() names the buffer download() reads) after the calls: the pass is in
    place, the caller's scratch tensor is never written;
  * to the caller's stream: the sequence of tests/test_gpu_g_wrapped_streams.py (a delay on the stream, then a copy into the tensor,
    then the calls) must see the copied state, table uploads included;
  * from a handle that apply_ops left relabelled (tile = 1, tile_relabel = 3), the call settles it first on every form."""
from gpu_common import *  # noqa: F401,F403

import multiplex_ref as R
from test_gpu_g_wrapped_streams import _FORMS, _nothing, _ordered
from wrapped_common import assert_twins, close_forms, make_forms

pytestmark = pytest.mark.gpu

DTYPES = (np.complex128, np.complex64)
_IDS = ("c128", "c64")
BIG = 15


def _cases(n):
    """(select, targets) as qubits: targets inside and outside the row, index bit 0 (qubit n - 1) among them"""
    if n == 1:
        return [([], [0])]
    return [([n - 1, 0, 9], [n - 2]), ([3, n - 3], [0, n - 1]), ([5, 6, 7, 8, 10, 11, 12], [2, 1]), ([], [n - 6, n - 7])]


@pytest.mark.parametrize("n", (1, BIG))
@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_forms_are_twins_of_the_spec(dtype, n):
    rng = np.random.default_rng(90 + n)
    x = R.make_state(n, 80 + n, dtype)
    calls = [(s, t, R.unitary_table(rng, len(s), len(t))) for s, t in _cases(n)]
    forms = make_forms(n, dtype, x)
    try:
        for f in forms:
            for s, t, table in calls:
                f.st.apply_multiplexed(s, t, table)  # (no synchronisation in between)
        got = assert_twins(forms, f"apply_multiplexed n={n}")
        for f in forms[1:]:  # in place: the state is still in the caller's tensor
            assert f.st.device_ptr() == f.amps.ptr
    finally:
        close_forms(forms)
    want = x
    for s, t, table in calls:
        want = R.apply_multiplexed_spec(n, want, s, t, table)
    assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))
    assert not np.array_equal(got, x)


@pytest.mark.parametrize("form", _FORMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_tables_wait_for_the_callers_stream(dtype, form):
    """W1 and W2, n = 15, both dtypes: three apply_multiplexed calls with three tables — each goes through one of two pinned host
    copies and one device buffer, so the third call reuses the first copy and every upload has to be ordered behind the previous
    call's kernel; reference: the owned twin, array_equal"""
    rng = np.random.default_rng(91)
    calls = [(s, t, R.unitary_table(rng, len(s), len(t))) for s, t in _cases(BIG)[:3]]

    def call(st, _):
        for s, t, table in calls:
            st.apply_multiplexed(s, t, table)

    _ordered(form, dtype, _nothing, call)


@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_relabelled_forms(dtype):
    n = BIG
    ops = circuits.c2_random_circuit(n, 80, seed=41)
    x = R.make_state(n, 85, dtype)
    select, targets = [0, 9, 14], [3, 13]
    table = R.unitary_table(np.random.default_rng(92), 3, 2)
    forms = make_forms(n, dtype, x, tile=1, tile_relabel=3, profile=1)
    try:
        for f in forms:
            f.st.apply_ops(ops)
            f.st.profile_reset()
            f.st.apply_multiplexed(select, targets, table)
            assert f.st.profile().get("k_permute_bits", {}).get("launches", 0) >= 1, f"{f.name}: the batch left no layout to restore"
        got = assert_twins(forms, "relabelled apply_multiplexed")
    finally:
        close_forms(forms)
    with q.HipState(n, dtype) as plain:
        plain.upload(x)
        plain.set_option("tile", 1)
        plain.set_option("tile_relabel", 3)
        plain.apply_ops(ops)
        y = plain.download()  # (settles)
    want = R.apply_multiplexed_spec(n, y, select, targets, table)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
