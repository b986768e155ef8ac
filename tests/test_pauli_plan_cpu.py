"""The host side of a Pauli-string pass (csrc/qip_pauli_plan.h) without a GPU: the header is plain C++, so a stand-alone program
(tests/cpp/test_pauli_plan.cpp) includes it alone and checks by brute force, for n = 1 .. 12, both element packings, x masks of
every class and z masks in slots 0, 5 and 31: the transposed z masks give the parity of popcount(j & z) at every work index, the
work indices reach every amplitude exactly once, a pair's partner lies above it; the geometry of a pass (alone also at n = 13 .. 30: several
blocks of whole spans, and at n = 26 a block first holds two spans); and both planners on term lists with repeated and interleaved x masks under groups 1, 2, 16 and 32.
It is built with the address and undefined-behaviour sanitizers on the host compiler and run directly."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_pauli_plan.cpp")
INC = os.path.join(ROOT, "rustqip_amd", "csrc")


def test_plan_header_is_plain_cpp_and_holds_by_brute_force_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "test_pauli_plan")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I" + INC, SRC, "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, " ".join(cmd) + "\n" + res.stdout + res.stderr
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and "pauli plan ok" in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]
