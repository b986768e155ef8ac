"""Classical functions between qubit registers (include/qip_hipx.h: qipx_state_apply_function, qipx_function_passes) without a GPU.

tests/function_ref.py agrees with the existing CPU route: the same map spelled as a SparseMatrix op goes through the oracle.
The pass planner (rustqip_amd/csrc/qip_function_plan.h) is plain C++: a stand-alone program (tests/cpp/test_function_plan.cpp)
walks every block, wave, row and lane as the kernel does and compares with the definition, under the host sanitizers.
qipx_function_passes counts passes and refuses malformed registers with the call's own messages, and the call itself refuses a
null handle: there is no CPU fall-back."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import function_ref as F
import rustqip_amd as q
from rustqip_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("mode", ("xor", "add"))
@pytest.mark.parametrize("n,ins,outs", [
    (10, [0, 9, 4], [2, 7, 5, 1, 8]),  # m + k = 8, scrambled
    (9, [3], [8, 0]),
    (7, [], [6, 2, 4]),                # a constant
    (10, [9, 8, 7, 6], [0, 1, 2, 3]),
    (5, [4, 0], [2, 1]),
])
def test_reference_is_the_sparse_op_through_the_oracle(oracle, n, ins, outs, mode):
    rng = np.random.default_rng(1000 * n + len(ins))
    values = rng.integers(0, 2 ** len(outs), size=2 ** len(ins), dtype=np.uint64)
    op = q.make_sparse_matrix_op(ins + outs, F.permutation_rows(len(ins) + len(outs), len(ins), len(outs), values, mode))
    for dtype in F.DTYPES:
        x = F.make_state(n, 7 + n, dtype)
        want = np.zeros_like(x)
        oracle.apply_op_overwrite(n, op, x, want)
        got = F.apply_function_ref(n, x, ins, outs, values, None, mode)
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (n, ins, outs, mode)
        assert not np.array_equal(got, x)


def test_reference_with_phases_is_the_diagonal_times_the_move():
    n, ins, outs = 8, [1, 6, 3], [0, 7]
    rng = np.random.default_rng(5)
    values = rng.integers(0, 4, size=8, dtype=np.uint64)
    phases = rng.uniform(-4, 4, size=8)
    x = F.make_state(n, 3, np.complex128)
    moved = F.apply_function_ref(n, x, ins, outs, values, None, "add")
    got = F.apply_function_ref(n, x, ins, outs, values, phases, "add")
    xs = F.gather(n, np.arange(2 ** n, dtype=np.uint64), ins)
    assert np.allclose(got, np.exp(1j * phases)[xs] * moved, rtol=0, atol=1e-15)
    only = F.apply_function_ref(n, x, ins, [], None, phases)
    assert np.allclose(only, np.exp(1j * phases)[xs] * x, rtol=0, atol=1e-15)


def test_plan_header_is_plain_cpp_and_moves_every_amplitude_by_brute_force_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "test_function_plan")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "rustqip_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "test_function_plan.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, " ".join(cmd) + "\n" + res.stdout + res.stderr
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and "function plan ok" in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]


def test_function_passes_counts_out_positions_outside_the_low_six():
    n = 20  # qubit q is index bit 19 - q: qubits 13 and below sit outside the six low index bits
    six, seven = list(range(8, 14)), list(range(7, 14))
    assert q.function_passes(n, [0, 1, 2], six, "xor") == 1
    assert q.function_passes(n, [0, 1, 2], seven, "xor") == 2
    assert q.function_passes(n, [0, 1, 2], six + [14, 19, 17, 15, 16, 18], "xor") == 1  # (out bits inside the low six do not count)
    assert q.function_passes(n, [0], list(range(1, 14)), "xor") == 3
    assert q.function_passes(n, [0, 1, 2], six + [19, 18], "add") == 1
    assert q.function_passes(n, [5, 6], [], "xor") == 1 and q.function_passes(n, [], [3], "add") == 1
    assert q.function_passes(3, [0], [1, 2], "add") == 1
    with pytest.raises(q.CircuitError, match="QIPX_FN_ADD with 7 out positions outside the six low index bits, at most 6"):
        q.function_passes(n, [0, 1, 2], seven, "add")


def _passes(n, ins, outs, mode):
    a, b = (C.c_uint64 * max(1, len(ins)))(*ins), (C.c_uint64 * max(1, len(outs)))(*outs)
    out = C.c_uint32(77)
    rc = _ffi.lib.qipx_function_passes(n, a, len(ins), b, len(outs), mode, C.byref(out))
    return rc, _ffi.last_error(), out.value


@pytest.mark.parametrize("args,message", [
    ((12, [12], [0], 0), "qubit 12 out of range"),
    ((12, [1], [0, 40], 0), "qubit 40 out of range"),
    ((12, [1, 2, 1], [0], 0), "qubit 1 repeated"),
    ((12, [1], [3, 4, 3], 1), "qubit 3 repeated"),
    ((12, [1, 2], [0, 2], 0), "qubit 2 is in both registers"),
    ((12, [1], [0], 2), "unknown mode 2"),
    ((12, [1], [0], -1), "unknown mode -1"),
    ((30, list(range(25)), [29], 0), "an in register of 25 qubits, at most 24"),
    ((40, [39], list(range(33)), 0), "an out register of 33 qubits, at most 32"),
    ((20, [19], list(range(7)), 1), "QIPX_FN_ADD with 7 out positions outside the six low index bits"),
    ((0, [], [], 0), "0 qubits"),
])
def test_malformed_registers_are_refused_by_message(args, message):
    rc, err, out = _passes(*args)
    assert rc == _ffi.QIP_ERR_INVALID and message in err and err.startswith("apply_function:"), err
    assert out == 0


def test_null_arrays_and_output():
    assert _ffi.lib.qipx_function_passes(8, None, 2, None, 0, 0, C.byref(C.c_uint32())) == _ffi.QIP_ERR_INVALID
    assert "null qubit array" in _ffi.last_error()
    assert _ffi.lib.qipx_function_passes(8, None, 0, None, 0, 0, None) == _ffi.QIP_ERR_INVALID
    assert "null output" in _ffi.last_error()
    out = C.c_uint32()
    assert _ffi.lib.qipx_function_passes(8, None, 0, None, 0, 0, C.byref(out)) == _ffi.QIP_OK and out.value == 1


def test_the_call_refuses_a_null_handle():
    """no CPU fall-back: without a device there is no handle, and a null handle is refused"""
    ins, outs, values = (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(1), (C.c_uint64 * 2)(0, 1)
    assert _ffi.lib.qipx_state_apply_function(None, ins, 1, outs, 1, 0, values, None) == _ffi.QIP_ERR_INVALID
    assert "null state handle" in _ffi.last_error()


def test_python_side_refusals():
    with pytest.raises(q.CircuitError, match="neither 'xor' nor 'add'"):
        q.function_passes(8, [0], [1], "sub")
    with pytest.raises(q.CircuitError, match="at most 24"):
        q.function_passes(40, list(range(25)), [30])
