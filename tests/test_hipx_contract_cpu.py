"""include/qip_hipx.h, the capabilities beyond the reference's interface — CPU only: the header, the ctypes table, the Rust
declarations and the library's exports are one set under their own version-script node, the header is plain C11, and the
exact reference the GPU tests of the batched soft_measure use (tests/sample_many_ref.py) leaves out few enough samples."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import measure_ref as R
import sample_many_ref as S
from rustqip_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    hdr = open(os.path.join(ROOT, "include", "qip_hipx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return set(re.findall(r"\b(qipx_[a-z0-9_]+)\s*\(", hdr))


def test_header_ffi_and_rust_declare_one_set():
    names = _declared()
    assert {"qipx_abi_version", "qipx_state_soft_measure_many"} <= names
    assert set(_ffi.EXT_SIGNATURES) == names
    sys_ext = open(os.path.join(ROOT, "bindings", "rust", "qip-hip", "src", "sys_ext.rs")).read()
    assert set(re.findall(r"pub fn (qipx_[a-z0-9_]+)\s*\(", sys_ext)) == names
    lib_rs = open(os.path.join(ROOT, "bindings", "rust", "qip-hip", "src", "lib.rs")).read()
    assert re.search(r"^pub mod sys_ext;", lib_rs, flags=re.M)
    # the binding contract does not grow: no qipx_ name in qip_hip.h or sys.rs
    assert "qipx_" not in open(os.path.join(ROOT, "include", "qip_hip.h")).read()
    assert "qipx_" not in open(os.path.join(ROOT, "bindings", "rust", "qip-hip", "src", "sys.rs")).read()


def test_library_exports_them_under_their_own_node():
    names = _declared()
    out = subprocess.run(["nm", "-D", "--defined-only", "--with-symbol-versions", _ffi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {}
    for line in out.splitlines():
        parts = line.split()
        if len(parts) >= 3 and parts[1] in "TW" and parts[2].startswith("qipx_"):
            sym, _, node = parts[2].partition("@@")
            exported[sym] = node
    assert set(exported) == names
    assert all(node == "QIP_HIPX" for node in exported.values()), exported
    for name in names:
        assert hasattr(_ffi.lib, name)
    assert _ffi.lib.qipx_abi_version() == 1
    assert _ffi.lib.qip_hip_abi_version() == 8


def test_header_is_plain_c11(tmp_path):
    src = tmp_path / "only_hipx.c"
    src.write_text('#include "qip_hipx.h"\nint only_hipx_version(void) { return QIPX_ABI_VERSION; }\n')
    res = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                          "-o", str(tmp_path / "only_hipx.o")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_many_samples_without_a_device_fail_loudly():
    """no CPU fall-back: without a device there is no handle, and a null handle is refused"""
    out = (C.c_uint64 * 1)()
    rs = (C.c_double * 1)(0.5)
    idx = (C.c_uint64 * 1)(0)
    assert _ffi.lib.qipx_state_soft_measure_many(None, idx, 1, rs, 1, out) == _ffi.QIP_ERR_INVALID


def test_crossing_many_is_crossing_ref():
    for dtype, n in ((np.complex128, 10), (np.complex64, 6)):
        x = R.make_state(n, R.seed_of(n, dtype), dtype)
        rs = np.concatenate([S.margin_samples(dtype, n, 24), [0.0, 1e-300, 1.5, float(R.norm_ref(x))]])
        at, dist = S.crossing_many(x, rs)
        for j, r in enumerate(rs):
            want_at, want_dist = R.crossing_ref(x, float(r))
            assert int(at[j]) == want_at and dist[j] == want_dist, (n, r)


@pytest.mark.parametrize("dtype,n,count,margin", S.MARGIN_CASES, ids=lambda v: getattr(v, "__name__", str(v)))
def test_reference_leaves_out_at_most_one_percent(dtype, n, count, margin):
    """the share of a margin case's samples that lie within the margin of a partial sum (no defined outcome there)"""
    x = R.make_state(n, R.seed_of(n, dtype), dtype)
    _, dist = S.crossing_many(x, S.margin_samples(dtype, n, count))
    left_out = int(np.sum(dist < margin))
    print(f"{np.dtype(dtype).name} n={n}: {left_out} of {count} left out")
    assert left_out <= count // 100
