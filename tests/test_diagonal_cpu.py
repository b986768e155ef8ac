"""The diagonal Pauli sums (include/qip_hipx.h: qipx_state_apply_diagonal, qipx_state_expect_diagonal) without a GPU.

The host side (rustqip_amd/csrc/qip_diag_plan.h) is plain C++: a stand-alone program (tests/cpp/test_diag_plan.cpp) includes it
alone and checks by brute force, for n = 1 .. 16 and both element packings: every amplitude belongs to exactly one tile row, the
groups partition the terms and keep their order, and the host reference of the energy equals the term-by-term sum to the stated
bound — exactly for dyadic coefficients — on random lists with repeated masks, empty terms, terms only below and only above the
tile boundary, long groups and more distinct low masks than a block has lanes.  It is built with the address and
undefined-behaviour sanitizers on the host compiler and run directly.

tests/diagonal_ref.py: the two forms of the reference agree, the stated arithmetic restated in numpy meets the bars the GPU tests
use, and the library exports the two calls and refuses a null handle."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import diagonal_ref as D
from rustqip_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_diag_plan.cpp")
INC = os.path.join(ROOT, "rustqip_amd", "csrc")


def test_plan_header_is_plain_cpp_and_holds_by_brute_force_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "test_diag_plan")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I" + INC, SRC, "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, " ".join(cmd) + "\n" + res.stdout + res.stderr
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and "diag plan ok" in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]


def test_the_two_forms_of_the_reference_agree():
    for n in (1, 5, 10):
        zs, cs = D.random_case(n, 25, 70 + n)
        a, b = D.energies_ref(n, zs, cs), D.energies_brute(n, zs, cs)
        weight = float(np.sum(np.abs(cs)))
        assert float(np.max(np.abs(a - b))) <= (25 + n) * 2.0 ** -63 * weight
        dy = np.round(cs * 64) / 64
        assert np.array_equal(D.energies_ref(n, zs, dy), D.energies_brute(n, zs, dy))
        assert np.array_equal(D.energy_spec(n, zs, dy).astype(np.longdouble), D.energies_brute(n, zs, dy))


@pytest.mark.parametrize("n", (10, 13))
@pytest.mark.parametrize("dtype", D.DTYPES, ids=("c128", "c64"))
def test_the_stated_arithmetic_meets_the_bars(dtype, n):
    x = D.make_state(n, D.seed_of(n, dtype), dtype)
    for count, scale, gamma in ((1, 1.0, 0.7), (40, 1.0, -1.9), (300, 100.0, 0.7)):
        zs, cs = D.random_case(n, count, 900 + n + count, scale)
        ok, worst = D.within_phase_bar(n, count, abs(gamma) * float(np.sum(np.abs(cs))), D.phase_spec(n, zs, cs, gamma, x),
                                       D.phase_ref(n, zs, cs, gamma, x), x)
        print(f"n={n} T={count}: phase worst {worst:.3f} of the bar")
        assert ok, (n, count)
        m1, m2 = D.moments_spec(n, zs, cs, x)
        r1, r2 = D.moments_ref(n, zs, cs, x)
        b1, b2 = D.moment_bars(n, count, float(np.sum(np.abs(cs))), x)
        print(f"n={n} T={count}: m1 {abs(m1 - r1) / b1:.3f}, m2 {abs(m2 - r2) / b2:.3f} of their bars")
        assert abs(m1 - r1) <= b1 and abs(m2 - r2) <= b2, (n, count)
    assert np.array_equal(D.phase_spec(n, [3], [0.5], 0.0, x).view(np.uint8), x.view(np.uint8))


def test_the_chain_length_is_the_headers():
    assert D.chain_length(30) == 1024 + 6 + 4 + 4096 and D.chain_length(13) == 28 and D.chain_length(5) == 12


def test_the_two_symbols_exist_and_refuse_a_null_handle():
    """no CPU fall-back: without a device there is no handle, and a null handle is refused"""
    start, qubits, paulis, coeffs = (C.c_uint64 * 2)(0, 1), (C.c_uint64 * 1)(0), (C.c_uint8 * 1)(3), (C.c_double * 1)(0.5)
    out = (C.c_double * 2)()
    assert _ffi.lib.qipx_state_apply_diagonal(None, start, qubits, paulis, coeffs, 1, 0.3) == _ffi.QIP_ERR_INVALID
    assert "null state handle" in _ffi.last_error()
    assert _ffi.lib.qipx_state_expect_diagonal(None, start, qubits, paulis, coeffs, 1, out) == _ffi.QIP_ERR_INVALID
    assert "null state handle" in _ffi.last_error()
