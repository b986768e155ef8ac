"""The quantum Fourier transform of a register (include/qip_hipx.h: qipx_state_apply_qft, qipx_qft_passes) without a GPU.

Convention: rustqip_amd.fourier.qft_ops, the lowered circuit, through the CPU oracle equals tests/qft_ref.py for every flag
combination, and circuits.c3_qft(n) is the flags = 0 transform of [n-1, .., 0]: the tie to the reference's qfft.
Bar: a numpy emulation of the planned flow in the state's precision meets 8 m u per fibre on every shape the GPU tests use, by
correct arithmetic alone, and misses it by more than 1000 times with one wrong twiddle exponent.
Plan: rustqip_amd/csrc/qip_qft_plan.h is plain C++; a stand-alone program (tests/cpp/test_qft_plan.cpp) walks every block, thread,
step and element as the kernel does, in long double, under the host sanitizers.
Entry checks: qipx_qft_passes counts passes and refuses malformed calls with the call's own messages, and the call itself refuses a
null handle: there is no CPU fall-back.  Declarations: ctypes and Rust match the header."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import qft_ref as R
import rustqip_amd as q
from rustqip_amd import _ffi, circuits, fourier

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _through_oracle(oracle, n, ops, x):
    return oracle.apply_ops_in_place(n, ops, x.copy())


@pytest.mark.parametrize("n,qubits", [
    (1, [0]), (2, [1, 0]), (3, [2, 1, 0]), (3, [0, 2]), (4, [1]), (5, [4, 3, 2, 1, 0]), (5, [0, 3, 1]), (6, [5, 4, 3, 2, 1, 0]),
    (6, [2, 5, 0, 3]), (6, [0, 1, 2, 3, 4, 5]), (6, [4, 1]),
])
def test_the_lowered_circuit_through_the_oracle_is_the_reference(oracle, n, qubits):
    x = R.make_state(n, 10 + n, np.complex128, binades=4)
    exact = R.qft_exact_all(n, x, qubits)
    for inverse, reversed in R.FLAGS:
        got = _through_oracle(oracle, n, fourier.qft_ops(qubits, inverse=inverse, reversed=reversed), x)
        err = np.max(np.abs(got - exact[(inverse, reversed)].astype(np.complex128)))
        assert err <= 1e-13 * np.max(np.abs(x)), (n, qubits, inverse, reversed, err)
    if len(qubits) >= 2:
        assert not np.allclose(exact[(False, False)].astype(np.complex128), exact[(True, False)].astype(np.complex128))


@pytest.mark.parametrize("n", (1, 2, 3, 5, 6))
def test_c3_qft_is_the_forward_transform_of_the_whole_register_qubit_0_most_significant(oracle, n):
    x = R.make_state(n, 20 + n, np.complex128, binades=4)
    want = R.qft_exact(n, x, list(range(n))[::-1]).astype(np.complex128)
    got = _through_oracle(oracle, n, circuits.c3_qft(n), x)
    assert np.max(np.abs(got - want)) <= 1e-13 * np.max(np.abs(x))
    # the definition itself, by the DFT matrix on the index (qubit 0 = the top index bit = the register's top bit)
    size = 2 ** n
    dft = np.exp(2j * np.pi * np.outer(np.arange(size), np.arange(size)) / size) / np.sqrt(size)
    assert np.max(np.abs(dft @ x - want)) <= 1e-12 * np.max(np.abs(x))


def test_the_emulated_flow_meets_the_bar_on_every_gpu_shape_by_arithmetic_alone():
    worst = {np.dtype(d).name: (0.0, None) for d in R.DTYPES}
    for n, qubits in R.all_gpu_shapes():
        for dtype in R.DTYPES:
            x = R.make_state(n, 7 * n + len(qubits), dtype)
            exact = R.qft_exact_all(n, x, qubits)
            for inverse, reversed in R.FLAGS:
                got = R.emulate_flow(n, x, qubits, inverse, reversed)
                ratio = R.worst_ratio(n, got, exact[(inverse, reversed)], x, qubits, dtype)
                if ratio > worst[np.dtype(dtype).name][0]:
                    worst[np.dtype(dtype).name] = (ratio, (n, qubits, inverse, reversed))
    print("worst |error| / (m u |fibre|):", worst)
    for name, (ratio, where) in worst.items():
        assert ratio <= R.BAR, (name, ratio, where)  # (seen: 2.1 m u at m = 1, where a fibre is one rounded sum; under 1 from m = 4 on)


@pytest.mark.parametrize("n,qubits,wrong", [
    (13, R.qubits_at(13, [6, 7, 8, 9, 10, 11, 12]), (0, 6)),   # the top stage of the first pass
    (13, R.qubits_at(13, [6, 7, 8, 9, 10, 11, 12]), (0, 3)),   # a middle stage
    (13, R.qubits_at(13, [6, 7, 8, 9, 10, 11, 12]), (1, 0)),   # the one stage of the second pass
    (9, R.qubits_at(9, [0, 1, 2, 3, 4, 5, 6, 7, 8]), (0, 1)),  # the smallest twiddled stage of all
])
def test_one_wrong_twiddle_exponent_misses_the_bar_a_thousandfold(n, qubits, wrong):
    for dtype in R.DTYPES:
        x = R.make_state(n, 31, dtype)
        for inverse, reversed in R.FLAGS:
            exact = R.qft_exact(n, x, qubits, inverse, reversed)
            good = R.worst_ratio(n, R.emulate_flow(n, x, qubits, inverse, reversed), exact, x, qubits, dtype)
            bad = R.worst_ratio(n, R.emulate_flow(n, x, qubits, inverse, reversed, wrong=wrong), exact, x, qubits, dtype)
            assert good <= R.BAR and bad >= 1000 * R.BAR, (np.dtype(dtype).name, inverse, reversed, good, bad)


def test_plan_header_is_plain_cpp_and_its_flow_is_the_dft_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "test_qft_plan")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "rustqip_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "test_qft_plan.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, " ".join(cmd) + "\n" + res.stdout + res.stderr
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and "qft plan ok" in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]


def test_the_host_walk_of_the_large_gpu_shapes_stays_in_bounds(tmp_path):
    """the same program's `big` mode: the n = 19 pass-boundary registers and an n = 15 register of the GPU tests, all four flag
    combinations, every slot, table index and vector index checked against its bound; optimised and without sanitizers (seconds)"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "test_qft_plan_big")
    cmd = [cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "rustqip_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "test_qft_plan.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, " ".join(cmd) + "\n" + res.stdout + res.stderr
    res = subprocess.run([exe, "big"], capture_output=True, text=True)
    assert res.returncode == 0 and "qft plan ok (big)" in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]


def test_qft_passes_follows_the_rule():
    n = 30
    low12, high12, high16 = R.qubits_at(n, range(12)), R.qubits_at(n, range(18, 30)), R.qubits_at(n, range(14, 30))
    for dtype in R.DTYPES:
        assert q.qft_passes(n, low12, dtype=dtype) == 1 and q.qft_passes(n, low12, reversed=True, dtype=dtype) == 1
        assert q.qft_passes(n, high12, dtype=dtype) == 3 and q.qft_passes(n, high12, reversed=True, dtype=dtype) == 2
        assert q.qft_passes(n, high16, inverse=True, dtype=dtype) == 4 and q.qft_passes(n, high16, True, True, dtype=dtype) == 3
        assert q.qft_passes(n, list(range(n)), dtype=dtype) == 5 and q.qft_passes(n, list(range(n)), reversed=True, dtype=dtype) == 4
        assert q.qft_passes(n, [], dtype=dtype) == 0 and q.qft_passes(n, [], reversed=True, dtype=dtype) == 0
    for n, qubits, natural, reversed in R.boundary_cases():
        assert q.qft_passes(n, qubits) == natural == R.pass_count(n, qubits, False)
        assert q.qft_passes(n, qubits, reversed=True) == reversed == R.pass_count(n, qubits, True)
    for n, qubits in R.small_cases() + R.placement_cases():
        for rv in (False, True):
            assert q.qft_passes(n, qubits, reversed=rv) == R.pass_count(n, qubits, rv)


def _passes(dtype, n, qubits, flags, null=False):
    arr = (C.c_uint64 * max(1, len(qubits)))(*qubits)
    out = C.c_uint32(77)
    rc = _ffi.lib.qipx_qft_passes(dtype, n, None if null else arr, len(qubits), flags, C.byref(out))
    return rc, _ffi.last_error(), out.value


@pytest.mark.parametrize("args,message", [
    ((_ffi.QIP_C64, 12, [12], 0), "qubit 12 out of range"),
    ((_ffi.QIP_C32, 12, [1, 40], 2), "qubit 40 out of range"),
    ((_ffi.QIP_C64, 12, [1, 2, 1], 0), "qubit 1 repeated"),
    ((_ffi.QIP_C64, 12, [3, 4, 5], 4), "unknown flag bits"),
    ((_ffi.QIP_C64, 12, [3], 0x80000001), "unknown flag bits"),
    ((_ffi.QIP_C64, 0, [], 0), "0 qubits"),
    ((99, 12, [3], 0), "dtype 99 is not a state precision"),
])
def test_malformed_calls_are_refused_by_message(args, message):
    rc, err, out = _passes(*args)
    assert rc == _ffi.QIP_ERR_INVALID and message in err and err.startswith("apply_qft:"), err
    assert out == 0


def test_null_arrays_and_output():
    rc, err, out = _passes(_ffi.QIP_C64, 8, [1, 2], 0, null=True)
    assert rc == _ffi.QIP_ERR_INVALID and "null qubit array" in err and out == 0
    assert _ffi.lib.qipx_qft_passes(_ffi.QIP_C64, 8, None, 0, 0, None) == _ffi.QIP_ERR_INVALID
    assert "null output" in _ffi.last_error()
    out = C.c_uint32(5)
    assert _ffi.lib.qipx_qft_passes(_ffi.QIP_C64, 8, None, 0, 0, C.byref(out)) == _ffi.QIP_OK and out.value == 0


def test_the_call_refuses_a_null_handle():
    """no CPU fall-back: without a device there is no handle, and a null handle is refused"""
    arr = (C.c_uint64 * 2)(0, 1)
    assert _ffi.lib.qipx_state_apply_qft(None, arr, 2, 0) == _ffi.QIP_ERR_INVALID
    assert "null state handle" in _ffi.last_error()


def test_qft_ops_refuses_a_repeated_qubit_and_counts_its_gates():
    with pytest.raises(q.CircuitError, match="repeated"):
        fourier.qft_ops([1, 2, 1])
    m = 7
    assert len(fourier.qft_ops(range(m))) == m + m * (m - 1) // 2 + m // 2
    assert len(fourier.qft_ops(range(m), reversed=True)) == m + m * (m - 1) // 2
    assert len(fourier.qft_ops(range(30)[::-1])) == len(circuits.c3_qft(30)) == 480


def test_declarations_match_the_header():
    header = open(os.path.join(ROOT, "include", "qip_hipx.h")).read()
    assert "int qipx_state_apply_qft(qip_hip_state* s, const uint64_t* qubits, uint32_t m, uint32_t flags);" in header
    assert "int qipx_qft_passes(int dtype, uint32_t n, const uint64_t* qubits, uint32_t m, uint32_t flags, uint32_t* passes);" in header
    assert re.search(r"#define QIPX_QFT_INVERSE 1u\n#define QIPX_QFT_REVERSED 2u\n", header)
    u64p, u32 = C.POINTER(C.c_uint64), C.c_uint32
    f = _ffi.lib.qipx_state_apply_qft
    assert f.restype is C.c_int and list(f.argtypes) == [C.c_void_p, u64p, u32, u32]
    f = _ffi.lib.qipx_qft_passes
    assert f.restype is C.c_int and list(f.argtypes) == [C.c_int, u32, u64p, u32, u32, C.POINTER(u32)]
    rust = re.sub(r"\s+", " ", open(os.path.join(ROOT, "bindings", "rust", "qip-hip", "src", "sys_ext.rs")).read())
    assert "pub const QIPX_QFT_INVERSE: u32 = 1;" in rust and "pub const QIPX_QFT_REVERSED: u32 = 2;" in rust
    assert "pub fn qipx_state_apply_qft( s: *mut qip_hip_state, qubits: *const u64, m: u32, flags: u32, ) -> c_int;" in rust
    assert ("pub fn qipx_qft_passes( dtype: c_int, n: u32, qubits: *const u64, m: u32, flags: u32, passes: *mut u32, ) -> c_int;"
            in rust)
    assert _ffi.lib.qipx_abi_version() == 1
