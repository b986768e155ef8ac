"""The interpreter's device-side list format (csrc/qip_tile_wire.h) without a GPU: the packer and the accessors the kernel reads the
blocks with are plain C++ as well, so a stand-alone program (tests/cpp/test_tile_wire_pack.cpp) packs descriptors with every field at
its smallest and largest legal value, unpacks them through those accessors, compares field by field in both precisions and checks
the pairing rule of run items on hand-made lists.  It is built with the address and undefined-behaviour sanitizers on the host
compiler and run directly."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_tile_wire_pack.cpp")
INC = os.path.join(ROOT, "rustqip_amd", "csrc")


def _build(tmp_path, *extra):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "test_tile_wire_pack")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *extra, "-I" + INC, SRC, "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, " ".join(cmd) + "\n" + res.stdout + res.stderr
    return exe


def test_wire_header_is_plain_cpp_and_round_trips_every_field_under_sanitizers(tmp_path):
    exe = _build(tmp_path, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer")
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and "wire pack ok" in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]
    for what in ("gates<double>", "gates<float>", "items<double>", "items<float>"):
        assert what in res.stdout, res.stdout


def test_wire_blocks_are_64_bytes_and_naturally_aligned(tmp_path):
    """one scalar load per list entry: the sizes and alignments the kernel's 16-word fetch relies on, read back from the header"""
    probe = tmp_path / "probe.cpp"
    probe.write_text(
        '#include <cstdio>\n#include "qip_tile_wire.h"\nusing namespace qipk;\n'
        'int main() { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(TileWireGate<double>), alignof(TileWireGate<double>), '
        "sizeof(TileWireGate<float>), alignof(TileWireGate<float>), sizeof(TileWireItem<double>), sizeof(TileWireItem<float>)); }\n")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    exe = str(tmp_path / "probe")
    subprocess.run([cxx, "-std=c++17", "-I" + INC, str(probe), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [128, 64, 64, 64, 64, 64], out
