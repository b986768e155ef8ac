"""Handles on memory and streams the caller owns (qip_hip_state_wrap), for tests/test_gpu_g_wrapped_*.py.  A plain helper
module, no fixtures, beside gpu_common.py.

One host vector gives three handle forms:

    owned   HipState(n, dtype): the library's buffers and its own non-blocking stream — the twin every other form is held to
    W1      amplitudes and scratch are the interiors of two guarded torch tensors, the stream is a torch.cuda.Stream()
    W2      amplitudes in a guarded torch tensor, no scratch (the library allocates one when it needs to), stream None: torch's
            default stream, the HIP null stream

A guarded tensor has GUARD + 2^n + GUARD elements; the state is the interior view.  Both guard zones hold a sentinel, a fixed
bit pattern per element index that is no NaN (so array_equal can compare it) and that no amplitude of a test state has.  GUARD
is a multiple of 2, so a Complex<f32> interior starts 16-byte aligned, as the kernels' 16-byte element views need.
assert_guards_intact reads every zone back after the handle's stream has drained and compares it bit for bit."""
import ctypes
import re
import sys

import numpy as np

import rustqip_amd as q


def _import_torch():
    """torch on the HIP runtime the library already runs on.  A torch wheel ships its own copy of the runtime and asks the
    loader for it by the plain names below; libqip_hip.so asks for the versioned name.  With torch first (tools/bench_*.py) the
    library resolves to torch's copy.  In a test session the library is loaded long before this module, and torch would bring
    a SECOND runtime into the process, which finds no device: so the runtime that is loaded is opened once more under the plain
    names (the same file: the loader only notes the alias), and torch's libraries then bind to it."""
    if "torch" not in sys.modules:
        q.device_count()  # (the library and its runtime are loaded)
        for name in ("libamdhip64.so", "libhsa-runtime64.so"):
            try:
                ctypes.CDLL(name, mode=ctypes.RTLD_GLOBAL)
            except OSError:
                pass
    import torch

    with open("/proc/self/maps") as f:
        copies = set(re.findall(r"/\S*libamdhip64\S*", f.read()))
    if q.device_count() > 0:  # (without a device nothing here runs, and two idle copies do no harm)
        assert len(copies) == 1, f"two HIP runtimes in one process, the second one sees no device: {sorted(copies)}"
    return torch


torch = _import_torch()

GUARD = 4096
FORMS = ("owned", "W1", "W2")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def sentinel(count, dtype, salt):
    """element i of a guard zone: -(1000.5 + (37 i + 101 salt) mod 977) + i (0.25 + (7 i + salt) mod 1013) — exact in float32"""
    i = np.arange(count, dtype=np.int64)
    re = -(1000.5 + ((i * 37 + salt * 101) % 977))
    im = 0.25 + ((i * 7 + salt) % 1013)
    return (re + 1j * im).astype(dtype)


class GuardedBuffer:
    """a torch tensor of GUARD + 2^n + GUARD elements on the device; `ptr` is the address of the interior"""

    def __init__(self, n, dtype, salt, content=None):
        self.count = 1 << n
        host = np.empty(2 * GUARD + self.count, dtype=dtype)
        host[:GUARD] = sentinel(GUARD, dtype, salt)
        host[GUARD + self.count:] = sentinel(GUARD, dtype, salt + 1)
        host[GUARD:GUARD + self.count] = sentinel(self.count, dtype, salt + 2) if content is None else content
        self.low, self.high = host[:GUARD].copy(), host[GUARD + self.count:].copy()
        self.tensor = torch.from_numpy(host).cuda()
        self.interior = self.tensor[GUARD:GUARD + self.count]
        self.ptr = self.interior.data_ptr()
        assert self.ptr % 16 == 0 and self.interior.is_contiguous()

    def read(self):
        """the interior on the host (a copy on torch's current stream: the writer's stream has to be drained first)"""
        return self.interior.cpu().numpy()

    def guards_intact(self):
        host = self.tensor.cpu().numpy()
        return (np.array_equal(bits(host[:GUARD]), bits(self.low)),
                np.array_equal(bits(host[GUARD + self.count:]), bits(self.high)))


class Form:
    """one handle with the memory and the stream behind it; `amps` / `scratch` are GuardedBuffers or None"""

    def __init__(self, name, n, dtype, x, salt=0, stream=None):
        assert name in FORMS, name
        self.name, self.n, self.dtype = name, n, np.dtype(dtype)
        self.amps = self.scratch = self.stream = None
        if name == "owned":
            self.st = q.HipState(n, dtype)
            self.st.upload(x)
            return
        self.amps = GuardedBuffer(n, dtype, 10 * salt + 1, np.asarray(x, dtype=dtype))
        if name == "W1":
            self.scratch = GuardedBuffer(n, dtype, 10 * salt + 5)
            self.stream = stream if stream is not None else torch.cuda.Stream()
        torch.cuda.synchronize()  # the tensors are filled before the handle's stream touches them
        self.st = q.HipState(n, dtype, wrap_ptr=self.amps.ptr, scratch_ptr=self.scratch.ptr if self.scratch else None,
                             stream=self.stream.cuda_stream if self.stream is not None else None)

    def buffers(self):
        return [b for b in (self.amps, self.scratch) if b is not None]

    def set_options(self, **options):
        for k, v in options.items():
            self.st.set_option(k, v)

    def upload(self, x):
        """the state from the host through the handle: into whichever buffer is current"""
        self.st.upload(np.asarray(x, dtype=self.dtype))

    def launches(self):
        return {k: v["launches"] for k, v in self.st.profile().items()}

    def close(self):
        self.st.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def make_forms(n, dtype, x, names=FORMS, **options):
    """the forms `names`, each holding x, with the per-handle options set"""
    forms = [Form(name, n, dtype, x, salt=i) for i, name in enumerate(names)]
    for f in forms:
        f.set_options(**options)
    return forms


def close_forms(forms):
    for f in forms:
        f.close()


def assert_guards_intact(form, what=""):
    """all guard zones of the form's tensors, bit for bit, after the handle's stream has drained"""
    if not form.buffers():
        return
    form.st.sync()
    for role, buf in (("amplitude", form.amps), ("scratch", form.scratch)):
        if buf is None:
            continue
        low, high = buf.guards_intact()
        assert low, f"{what}: {form.name}: a kernel wrote in front of element 0 of the {role} tensor"
        assert high, f"{what}: {form.name}: a kernel wrote past element 2^n of the {role} tensor"


def assert_buffer_contract(form, what=""):
    """Where the state lives.  W1: device_ptr() is one of the two interiors, scratch_ptr() the other, and after sync() the torch
    view at device_ptr() is what download() returns.  W2: while device_ptr() is the tensor, the tensor's content is download().
    Guards are checked too.  device_ptr() settles a relabelled state, as the header says."""
    if form.name == "owned":
        return
    st = form.st
    cur = st.device_ptr()
    got = st.download()
    st.sync()
    if form.name == "W1":
        pair = {form.amps.ptr, form.scratch.ptr}
        other = st.scratch_ptr()
        assert cur in pair and other in pair and cur != other, (what, hex(cur), hex(other), [hex(p) for p in pair])
        assert st.device_ptr() == cur, what  # (asking for the scratch buffer moved nothing)
        view = (form.amps if cur == form.amps.ptr else form.scratch).read()
        assert np.array_equal(view, got), f"{what}: W1: the tensor at device_ptr() is not what download() returns"
    elif cur == form.amps.ptr:
        assert np.array_equal(form.amps.read(), got), f"{what}: W2: the wrapped tensor is not what download() returns"
    assert_guards_intact(form, what)


def assert_twins(forms, what="", contract=True):
    """every wrapped form holds, bit for bit, the vector of the owned twin (forms[0]); returns that vector"""
    assert forms[0].name == "owned"
    ref = forms[0].st.download()
    for f in forms[1:]:
        got = f.st.download()
        if not np.array_equal(got, ref):
            bad = np.flatnonzero(got != ref)
            raise AssertionError(f"{what}: {f.name} differs from the owned twin at {bad.size} amplitudes, first at index "
                                 f"{bad[0]}, max|d| = {np.max(np.abs(got - ref)):.3e}")
        if contract:
            assert_buffer_contract(f, what)
        else:
            assert_guards_intact(f, what)
    return ref


def assert_same_launches(forms, what=""):
    """with option profile = 1: the launches per kernel class of every form are those of the owned twin"""
    ref = forms[0].launches()
    for f in forms[1:]:
        assert f.launches() == ref, (what, f.name, f.launches(), ref)
    return ref
