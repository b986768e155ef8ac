"""The global option "slice_payload_cache_mb": the bound of the device-resident op payloads that qip_hip_apply_op_device keeps
(include/qip_hip.h).  Setting it needs no GPU: with nothing cached, 0 has nothing to synchronise or free."""
import os
import re

import pytest

import rustqip_amd as q
from rustqip_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slice_payload_cache_mb_values():
    try:
        for value in (0, 1, 256):
            q.set_global_option("slice_payload_cache_mb", value)
        with pytest.raises(q.CircuitError, match="slice_payload_cache_mb"):
            q.set_global_option("slice_payload_cache_mb", -1)
    finally:
        assert _ffi.lib.qip_hip_set_global_option(b"slice_payload_cache_mb", 256) in (0, 1)  # (1 = the key is unknown: reported above)


def test_the_option_is_documented_and_adds_no_entry_point():
    hdr = open(os.path.join(ROOT, "include", "qip_hip.h")).read()
    assert '"slice_payload_cache_mb"' in hdr
    assert len(set(re.findall(r"\b(qip_hip_[a-z0-9_]+)\s*\(", hdr))) == 66 and _ffi.lib.qip_hip_abi_version() == 8
