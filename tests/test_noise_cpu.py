"""Noise channels by quantum trajectories (include/qip_hipx.h: qipx_state_apply_reduce, qipx_state_apply_channels,
qipx_channel_passes; rustqip_amd/noise.py) without a GPU.

The header, the exports and the versions; the pass plan from pure host code; every refusal that needs no device (and the null
handle where a call needs one: there is no CPU fall-back); the Kraus families of rustqip_amd.noise; tests/noise_ref.py checked
against plain matrix application, a case worked by hand and the exact branch enumeration of a chain against the Kraus map; and
the host-only plan header (rustqip_amd/csrc/qip_channel_plan.h) against brute force through a stand-alone program."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import noise_ref as NR
import rustqip_amd as q
from rustqip_amd import _ffi, noise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("qipx_state_apply_reduce", "qipx_state_apply_channels", "qipx_channel_passes", "qipx_state_channel_passes")


def test_header_and_library_contract():
    hdr = open(os.path.join(ROOT, "include", "qip_hipx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert re.search(r"#define\s+QIPX_ABI_VERSION\s+1\b", hdr)
    out = subprocess.run(["nm", "-D", "--defined-only", "--with-symbol-versions", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r"\b%s@@QIP_HIPX\b" % name, out), name
    assert _ffi.lib.qipx_abi_version() == 1 and q.ext_abi_version() == 1
    assert len(_ffi.SIGNATURES) == 66  # include/qip_hip.h does not grow
    base = open(os.path.join(ROOT, "include", "qip_hip.h")).read()
    assert len(set(re.findall(r"\b(qip_hip_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", base, flags=re.S)))) == 66


def test_profile_classes_extend_the_binding_contracts_without_moving_them():
    lib = _ffi.lib
    base = lib.qip_hip_kernel_class_count()
    names = [lib.qipx_kernel_class_name(i).decode() for i in range(lib.qipx_kernel_class_count())]
    assert names[:base] == [lib.qip_hip_kernel_class_name(i).decode() for i in range(base)]
    assert names[base:] == ["k_apply_density_small", "reduced_density"]
    assert lib.qipx_kernel_class_name(len(names)) == b"" and lib.qip_hip_kernel_class_name(base) == b""
    assert lib.qipx_state_profile_get(None, base, None, None, None) == _ffi.QIP_ERR_INVALID


def _amp(qb, g=0.3):
    return noise.amplitude_damping(qb, g)


def test_channel_passes():
    assert q.channel_passes(5, [_amp(2)]) == (2, 0)
    for n in (1, 2, 7, 27):
        assert q.channel_passes(n, [_amp(qb) for qb in range(n)]) == (n + 1, n - 1)
    assert q.channel_passes(30, [_amp(qb) for qb in range(30)]) == (31 + 23, 29 - 23)  # (qubits 0 .. 23 are index bits 29 .. 6)
    two = noise.depolarizing([0, 1], 0.1), noise.depolarizing([2, 3], 0.1)
    assert q.channel_passes(4, two) == (4, 0)  # a union of four qubits: apply, then a density pass of its own
    assert q.channel_passes(4, [noise.depolarizing([0, 1], 0.1), noise.depolarizing([1, 2], 0.1), _amp(2)]) == (4, 2)
    assert q.channel_passes(4, [noise.depolarizing([3, 1], 0.1), noise.depolarizing([0, 2], 0.2), noise.gate([2], np.eye(2))]) == (5, 1)
    assert q.channel_passes(4, []) == (0, 0)
    # the measured routing (profiles/noise.md): on n >= 28 a step of one or two qubits with no index bit inside a wave row runs composed
    assert q.channel_passes(30, [_amp(0), _amp(1)]) == (4, 0) and q.channel_passes(27, [_amp(0), _amp(1)]) == (3, 1)
    assert q.channel_passes(30, [_amp(0), _amp(25)]) == (3, 1)   # qubit 25 is index bit 4
    assert q.channel_passes(30, [_amp(0), _amp(23)]) == (4, 0)   # qubit 23 is index bit 6
    assert q.channel_passes(30, [noise.depolarizing([0, 1], 0.1), _amp(2)]) == (3, 1)  # three qubits, Complex<f64>
    assert _ffi.lib.qipx_state_channel_passes(None, None, 0, None, None) == _ffi.QIP_ERR_INVALID


def _raw_channel(indices, k, kraus, count):
    idx = (C.c_uint64 * max(len(indices), 1))(*indices)
    ks = None if kraus is None else (C.c_double * len(kraus))(*kraus)
    ch = (_ffi.QipxChannel * 1)()
    ch[0].indices = idx if indices is not None else None
    ch[0].k, ch[0].kraus, ch[0].count = k, ks, count
    return ch, (idx, ks)


def test_refusals_without_a_device():
    lib = _ffi.lib
    passes, fused = C.c_uint64(9), C.c_uint64(9)
    eye = [1, 0, 0, 0, 0, 0, 1, 0]
    bad = [
        ([1], 0, eye, 1, "k = 0"), ([5], 1, eye, 1, "an index out of range"), ([1, 1], 2, eye * 4, 1, "a repeated index"),
        ([1], 1, eye, 0, "count = 0"), ([1], 1, eye, 17, "count = 17"), ([1], 1, None, 1, "null operators"),
    ]
    for indices, k, kraus, count, what in bad:
        ch, _keep = _raw_channel(indices, k, kraus, count)
        assert lib.qipx_channel_passes(5, ch, 1, C.byref(passes), C.byref(fused)) == _ffi.QIP_ERR_INVALID, what
        assert (passes.value, fused.value) == (0, 0) and _ffi.last_error(), what
    ch, _keep = _raw_channel([1], 1, eye, 1)
    ch[0].indices = None
    assert lib.qipx_channel_passes(5, ch, 1, C.byref(passes), C.byref(fused)) == _ffi.QIP_ERR_INVALID
    ch, _keep = _raw_channel([1], 1, eye, 1)
    assert lib.qipx_channel_passes(5, ch, 1, None, C.byref(fused)) == _ffi.QIP_ERR_INVALID
    assert lib.qipx_channel_passes(5, ch, 1, C.byref(passes), None) == _ffi.QIP_ERR_INVALID
    assert lib.qipx_channel_passes(5, None, 1, C.byref(passes), C.byref(fused)) == _ffi.QIP_ERR_INVALID
    assert lib.qipx_channel_passes(0, ch, 1, C.byref(passes), C.byref(fused)) == _ffi.QIP_ERR_INVALID
    assert lib.qipx_channel_passes(5, ch, 1, C.byref(passes), C.byref(fused)) == _ffi.QIP_OK and passes.value == 2
    three, _keep3 = _raw_channel([0, 1, 2], 3, [0.0] * 128, 1)
    assert lib.qipx_channel_passes(5, three, 1, C.byref(passes), C.byref(fused)) == _ffi.QIP_ERR_UNSUPPORTED
    # no CPU fall-back: the calls that work on a state refuse a null handle
    idx, m, rho = (C.c_uint64 * 1)(0), (C.c_double * 8)(*eye), (C.c_double * 8)()
    assert lib.qipx_state_apply_reduce(None, idx, 1, m, idx, 1, rho) == _ffi.QIP_ERR_INVALID
    r, chosen = (C.c_double * 1)(0.5), (C.c_uint32 * 1)()
    assert lib.qipx_state_apply_channels(None, ch, 1, r, chosen, None) == _ffi.QIP_ERR_INVALID
    with pytest.raises(q.CircuitError):
        q.channel_passes(5, [([0], np.eye(4))])  # the operator's shape does not fit its qubits


FAMILIES = [
    ("bit_flip", lambda p: noise.bit_flip(0, p)), ("phase_flip", lambda p: noise.phase_flip(1, p)),
    ("depolarizing1", lambda p: noise.depolarizing(2, p)), ("depolarizing2", lambda p: noise.depolarizing([0, 3], p)),
    ("pauli_channel", lambda p: noise.pauli_channel(0, p / 2, p / 3, p / 6)),
    ("amplitude_damping", lambda p: noise.amplitude_damping(1, p)),
    ("generalized_amplitude_damping", lambda p: noise.generalized_amplitude_damping(1, p, 0.3)),
    ("generalized_amplitude_damping_p", lambda p: noise.generalized_amplitude_damping(1, 0.4, p)),
    ("phase_damping", lambda p: noise.phase_damping(2, p)),
]


@pytest.mark.parametrize("name,make", FAMILIES, ids=[f[0] for f in FAMILIES])
@pytest.mark.parametrize("p", (0.0, 0.3, 1.0))
def test_every_family_is_complete(name, make, p):
    ch = make(p)
    total = sum(np.conj(K).T @ K for K in ch.kraus)
    assert np.max(np.abs(total - np.eye(total.shape[0]))) <= 1e-12
    assert ch.completeness_defect() <= 1e-12 and ch.check() is ch
    assert 1 <= len(ch.kraus) <= 16 and ch.kraus.shape[1] == 1 << len(ch.qubits)


def test_check_rejects_a_broken_set_and_constructors_reject_bad_parameters():
    with pytest.raises(q.CircuitError):
        noise.Channel([0], [np.eye(2), 0.1 * np.eye(2)]).check()
    with pytest.raises(q.CircuitError):
        noise.Channel([0, 1], [np.eye(2)])
    for make in (lambda: noise.bit_flip(0, 1.5), lambda: noise.amplitude_damping(0, -0.1), lambda: noise.pauli_channel(0, 0.5, 0.5, 0.5),
                 lambda: noise.depolarizing([0, 1, 2], 0.1)):
        with pytest.raises(q.CircuitError):
            make()
    g = noise.gate([1, 0], np.arange(16).reshape(4, 4))
    assert g.kraus.shape == (1, 4, 4) and g.qubits == [1, 0]
    # the two-qubit depolarizing channel is what its formula says: rho -> (1 - p) rho + p 1/4 tr rho
    ch, rho = noise.depolarizing([0, 1], 0.3), np.diag([0.5, 0.25, 0.25, 0.0]).astype(np.complex128)
    rho[0, 1] = rho[1, 0] = 0.1
    out = sum(K @ rho @ np.conj(K).T for K in ch.kraus)
    assert np.allclose(out, 0.7 * rho + 0.3 * np.eye(4) / 4, rtol=0, atol=1e-14)


def _state(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    return x / np.linalg.norm(x)


def test_reference_with_a_unitary_gate_is_plain_matrix_application():
    n = 4
    x = _state(n, 1)
    rng = np.random.default_rng(2)
    u, _ = np.linalg.qr(rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4)))
    for qubits in ([0, 2], [3, 1], [1, 0]):
        t = NR.trajectory(n, [(qubits, u[None])], x, [0.37])
        chosen, ws, y = t.chosen, t.weights, t.state
        # the definition, index by index: bit i of a row is index bit n - 1 - qubits[i]
        pos = [n - 1 - qb for qb in qubits]
        want = np.zeros(1 << n, dtype=np.complex128)
        for j in range(1 << n):
            a = sum(((j >> p) & 1) << i for i, p in enumerate(pos))
            for c in range(4):
                j2 = j
                for i, p in enumerate(pos):
                    j2 = (j2 & ~(1 << p)) | (((c >> i) & 1) << p)
                want[j] += u[a, c] * x[j2]
        assert chosen == [0] and np.allclose(y, want, rtol=0, atol=1e-14) and abs(ws[0][0] - 1.0) < 1e-14
    one = np.array([[0, 1], [1j, 0]])
    y = NR.apply_matrix(3, [1], one, np.eye(8)[:, 0b010])  # qubit 1 is index bit 1: |010> -> |000>
    assert np.array_equal(np.nonzero(y)[0], [0]) and y[0] == 1


def test_reference_amplitude_damping_on_one():
    g = 0.3
    ch = noise.amplitude_damping(0, g)
    one = np.array([0, 1], dtype=np.complex128)
    for u, want_branch, want_state in ((0.5, 0, [0, 1]), (0.9, 1, [1, 0]), (0.0, 0, [0, 1]), (0.7 + 1e-9, 1, [1, 0])):
        t = NR.trajectory(1, [(ch.qubits, ch.kraus)], one, [u])
        assert t.chosen == [want_branch] and np.allclose(t.weights[0], [1 - g, g], rtol=0, atol=1e-15)
        assert np.allclose(t.state, want_state, rtol=0, atol=1e-15)
    # on |0> the decay branch has weight exactly zero and is never taken, not even by u = 1
    t = NR.trajectory(1, [(ch.qubits, ch.kraus)], np.array([1, 0]), [1.0])
    assert t.chosen == [0] and t.weights[0][1] == 0.0 and np.array_equal(t.state, [1, 0])
    # a Complex<f32> device state stores every result rounded once: the reference can follow it
    x = _state(3, 11)
    chain = [([0], ch.kraus), ([1, 2], noise.depolarizing([1, 2], 0.4).kraus)]
    exact, stored = NR.trajectory(3, chain, x, [0.2, 0.6]), NR.trajectory(3, chain, x, [0.2, 0.6], store=np.complex64)
    assert np.array_equal(stored.states[0], exact.states[0].astype(np.complex64).astype(np.complex128))
    assert 0 < np.max(np.abs(stored.weights[1] - exact.weights[1])) < 1e-6 and stored.chosen == exact.chosen


def test_reference_branch_enumeration_is_the_kraus_map():
    n = 3
    x = _state(n, 7)
    chain = [noise.amplitude_damping(0, 0.3), noise.depolarizing([2, 0], 0.2), noise.phase_damping(1, 0.6)]
    chain = [(c.qubits, c.kraus) for c in chain]
    br = NR.branches(n, chain, x)
    assert abs(sum(p for p, _ in br) - 1.0) < 1e-12 and len(br) > 8
    mixed = sum(p * np.outer(y, np.conj(y)) for p, y in br)
    want = NR.kraus_map(n, chain, np.outer(x, np.conj(x)))
    assert np.max(np.abs(mixed - want)) <= 1e-12
    for _, y in br:
        assert abs(np.linalg.norm(y) - 1.0) < 1e-12  # every branch carries the norm through


def test_plan_header_is_plain_cpp_and_agrees_with_brute_force_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "test_channel_plan")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "rustqip_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "test_channel_plan.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, " ".join(cmd) + "\n" + res.stdout + res.stderr
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and "channel plan ok" in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]
