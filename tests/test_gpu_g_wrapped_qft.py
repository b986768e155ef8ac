"""The quantum Fourier transform of a register (include/qip_hipx.h: qipx_state_apply_qft) on handles that wrap caller memory and
caller streams.

Handle forms (tests/wrapped_common.py): owned, W1 and W2, at n = 15 and at n = 1, Complex<f64> and Complex<f32>.  The call is held
  * on the owned twin to tests/qft_ref.py: 8 m u per fibre for every call of the sequence by itself;
  * bit for bit to the owned twin on W1 and W2: the route does not depend on who owns the buffers or the stream;
  * to intact guard zones and the buffer contract (device_ptr() names the buffer download() reads) after one-pass calls, after
    reversed calls of several passes (in place: the state is still in the caller's tensor, the scratch tensor is never written)
    and after a natural-order call of several passes, whose closing bit reversal writes the scratch buffer and makes it current;
  * to the caller's stream: the sequence of tests/test_gpu_g_wrapped_streams.py (a delay on the stream, then a copy into the tensor,
    then the calls, then a clone on that stream, no host wait in between) must see the copied state, table uploads included."""
from gpu_common import *  # noqa: F401,F403

import qft_ref as R
from test_gpu_g_wrapped_streams import _FORMS, _nothing, _ordered
from wrapped_common import assert_twins, close_forms, make_forms

pytestmark = pytest.mark.gpu

DTYPES = (np.complex128, np.complex64)
_IDS = ("c128", "c64")
BIG = R.WRAPPED_N
ONE_PASS, REVERSED_PASSES, NATURAL_PASSES = R.WRAPPED_ONE_PASS, R.WRAPPED_REVERSED_PASSES, R.WRAPPED_NATURAL_PASSES  # (tests/qft_ref.py)


def _want(n, x, calls, dtype):
    """every call by itself meets the bar from the state the owned twin had before it; returns nothing: the forms are compared
    with the twin bit for bit"""
    with q.HipState(n, dtype) as st:
        st.upload(x)
        for qubits, inverse, reversed in calls:
            before = st.download()
            st.apply_qft(qubits, inverse=inverse, reversed=reversed)
            ratio = R.worst_ratio(n, st.download(), R.qft_exact(n, before, qubits, inverse, reversed), before, qubits, dtype)
            assert ratio <= R.BAR, (qubits, inverse, reversed, ratio)


@pytest.mark.parametrize("kind", ("one_pass", "reversed_passes", "natural_passes", "n1"))
@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_forms_are_twins_and_guards_stay_intact(dtype, kind):
    n = 1 if kind == "n1" else BIG
    calls = {"one_pass": ONE_PASS, "reversed_passes": REVERSED_PASSES, "natural_passes": NATURAL_PASSES,
             "n1": [([0], False, False), ([0], True, True)]}[kind]
    x = R.make_state(n, 80 + n, dtype)
    _want(n, x, calls, dtype)
    forms = make_forms(n, dtype, x)
    try:
        for f in forms:
            for qubits, inverse, reversed in calls:
                assert f.st.qft_passes(qubits, inverse, reversed) == R.pass_count(n, qubits, reversed)
                f.st.apply_qft(qubits, inverse=inverse, reversed=reversed)  # (no synchronisation in between)
        got = assert_twins(forms, f"apply_qft {kind}")
        for f in forms[1:]:
            if kind == "natural_passes":  # one closing sweep: the state is in the scratch buffer (W1: the caller's, guards checked)
                assert f.st.device_ptr() != f.amps.ptr
                if f.scratch is not None:
                    assert f.st.device_ptr() == f.scratch.ptr
            else:                         # in place: the state is still in the caller's tensor
                assert f.st.device_ptr() == f.amps.ptr
    finally:
        close_forms(forms)
    assert not np.array_equal(got, x)


@pytest.mark.parametrize("form", _FORMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_passes_and_tables_wait_for_the_callers_stream(dtype, form):
    """W1 and W2, n = 15, both dtypes: a one-pass call, a reversed call of two passes and a natural-order call of two passes and
    the closing sweep — three twiddle uploads through the two pinned host copies, every one ordered behind the previous call's
    kernels; reference: the owned twin, array_equal"""
    calls = [ONE_PASS[1], REVERSED_PASSES[0], NATURAL_PASSES[0]]

    def call(st, _):
        for qubits, inverse, reversed in calls:
            st.apply_qft(qubits, inverse=inverse, reversed=reversed)

    _ordered(form, dtype, _nothing, call)
