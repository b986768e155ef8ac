"""The Pauli-string calls (csrc/qip_pauli.hip) against the bits an earlier commit left: expect_pauli, pauli_matrix_elements,
apply_pauli_sum and apply_pauli_rotations on hashed states, held to SHA-256 digests recorded on an MI355X
(tests/golden/pauli_digests.json names the commit).  The references of the other Pauli tests bound errors; this one says that a
change meant to leave the numerics alone left the last bit alone.  It compares for equality: there is no tolerance.

The state: amplitude j is an integer hash of j (splitmix64; 24 bits each for the real and the imaginary part, as a signed
integer times a power of two: exact in both precisions), computed with integer operations only, so that no random-number stream
can drift between versions.  No reference is computed.

The sizes: n = 14 is the smallest with a whole span per block in every class and precision; n = 26 (Complex<f64>) and n = 27
(Complex<f32>, packed) are the smallest with SEVERAL spans per block (a block's chunk exceeds one span only from 2^25 work items
on), which is where the sign word is carried from span to span.  The large cases hold 1 GiB per state, two states resident.

The terms: the classes of the expect tests' MANY_BLOCK_MASKS (x = 0, bit 0, the top bit, a mixed mask with n_Y = 2 and 5) and one
run of 20 terms of one x mask: passes of 16 and 4 under the default groups, one of 32 slots under group 32, singles — every
kernel capacity, and more than one pass.

    python tests/test_gpu_f2_pauli_digests.py --record [--commit ID] [--out FILE]    # on the GPU, at the commit to hold to"""
import hashlib
import json
import os
import struct
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import rustqip_amd as q  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "pauli_digests.json")
CASES = ((14, "complex128"), (14, "complex64"), (26, "complex128"), (27, "complex64"))
_M64 = (1 << 64) - 1


def _mix(z):
    """splitmix64's finalizer on a uint64 array, in place (the products wrap)"""
    z += np.uint64(0x9E3779B97F4A7C15)
    z ^= z >> np.uint64(30)
    z *= np.uint64(0xBF58476D1CE4E5B9)
    z ^= z >> np.uint64(27)
    z *= np.uint64(0x94D049BB133111EB)
    z ^= z >> np.uint64(31)
    return z


def _mix_int(v):
    z = (v + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def hashed_state(n, dtype, salt):
    """amplitude j = ((h >> 40) - 2^23, (h & 0xffffff) - 2^23) * 2^-(23 + n // 2), h = splitmix64(j + salt * 2^40)"""
    out = np.empty(1 << n, dtype=dtype)
    parts = out.view(np.float64 if out.dtype == np.complex128 else np.float32).reshape(-1, 2)
    scale = 2.0 ** -(23 + n // 2)
    step = 1 << min(n, 18)
    for lo in range(0, 1 << n, step):
        h = _mix(np.arange(lo, lo + step, dtype=np.uint64) + np.uint64(salt << 40))
        parts[lo:lo + step, 0] = ((h >> np.uint64(40)).astype(np.int64) - (1 << 23)) * scale
        parts[lo:lo + step, 1] = ((h & np.uint64(0xFFFFFF)).astype(np.int64) - (1 << 23)) * scale
    return out


def term_of_masks(n, x, z):
    """X on x & ~z, Z on z & ~x, Y on x & z (masks over amplitude-index bits; qubit q is bit n - 1 - q)"""
    term = {}
    for b in range(n):
        bx, bz = (x >> b) & 1, (z >> b) & 1
        if bx or bz:
            term[n - 1 - b] = "Y" if bx and bz else ("X" if bx else "Z")
    return term


def case_terms(n):
    full, top = (1 << n) - 1, 1 << (n - 1)
    odd, even = 0x5555555555555555 & full, 0xAAAAAAAAAAAAAAAB & full
    mixed = (1 << (n - 2)) | (1 << (n // 2)) | 0x812
    run = top | (1 << (n // 2 + 1)) | 0x104
    masks = [(0, 0), (0, 1), (0, odd), (0, top | 0x801),
             (1, 0), (1, 1), (1, even), (1, top | 0x801),
             (top, 0), (top, top | 1), (top, odd), (top, full),
             (mixed, 0), (mixed, (1 << (n - 2)) | 0x403), (mixed, mixed)]  # n_Y = 0, 2 and 5
    masks += [(run, _mix_int(k) >> (64 - n)) for k in range(20)]
    return [term_of_masks(n, x, z) for x, z in masks]


def _coefficients(count):
    k = np.arange(count)
    return ((k * 37) % 64 - 32) / 64.0 + 1j * (((k * 53) % 64 - 31) / 64.0)


def _angles(count):
    return ((np.arange(count) * 29) % 64 - 32) / 16.0


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def digests(n, dtype):
    """the digests of one case; the two states are built and uploaded once"""
    dtype = np.dtype(dtype)
    terms = case_terms(n)
    coeffs, angles = _coefficients(len(terms)), _angles(len(terms))
    where = np.array([0, (1 << n) - 1] + [_mix_int(k + (1 << 50)) >> (64 - n) for k in range(4094)], dtype=np.uint64)

    def sampled(st):
        return _sha(st.download_indices(where), struct.pack("<d", st.norm_sqr()))

    out = {}
    with q.HipState(n, dtype) as psi, q.HipState(n, dtype) as phi:
        psi.upload(hashed_state(n, dtype, 0))
        phi.upload(hashed_state(n, dtype, 1))
        out["expect"] = _sha(psi.expect_pauli(terms))
        out["expect_singles"] = _sha(np.array([psi.expect_pauli([t])[0] for t in terms]))
        psi.set_option("expect_group", 32)
        out["expect_group32"] = _sha(psi.expect_pauli(terms))
        psi.set_option("expect_group", 16)
        out["matrix_elements"] = _sha(phi.pauli_matrix_elements(psi, terms))
        phi.apply_pauli_sum(psi, terms, coeffs, accumulate=True)
        out["sum_accumulating"] = sampled(phi)
        phi.set_option("sum_group", 32)
        phi.apply_pauli_sum(psi, terms, coeffs, accumulate=True)
        out["sum_accumulating_group32"] = sampled(phi)
        phi.set_option("sum_group", 16)
        phi.apply_pauli_sum(psi, terms, coeffs)
        out["sum_storing"] = sampled(phi)
        phi.apply_pauli_sum(psi, terms[4:5], coeffs[4:5])
        out["sum_storing_single"] = sampled(phi)
        psi.apply_pauli_rotations(terms, angles)
        out["rotations"] = sampled(psi)
        psi.set_option("rotate_group", 1)
        psi.apply_pauli_rotations(terms[:15], angles[:15])
        out["rotations_singles"] = sampled(psi)
    return out


def _key(n, dtype):
    return f"n={n} {np.dtype(dtype).name}"


@pytest.mark.gpu
@pytest.mark.parametrize("n,dtype", CASES, ids=[_key(n, d).replace(" ", "-") for n, d in CASES])
def test_the_bits_of_the_recorded_commit(n, dtype):
    recorded = json.load(open(GOLDEN))
    t0 = time.perf_counter()
    got = digests(n, dtype)
    print(f"{_key(n, dtype)}: {time.perf_counter() - t0:.2f} s; recorded from {recorded['commit']}")
    want = recorded["digests"][_key(n, dtype)]
    differing = sorted(k for k in want if got.get(k) != want[k])
    print(f"{_key(n, dtype)}: differing parts: {differing or 'none'}")
    assert got == want


def _record(argv):
    import subprocess

    out, commit = GOLDEN, None
    if "--out" in argv:
        out = argv[argv.index("--out") + 1]
    if "--commit" in argv:
        commit = argv[argv.index("--commit") + 1]
    if commit is None:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    result = {"commit": commit, "device": "AMD Instinct MI355X (gfx950)", "digests": {}}
    for n, dtype in CASES:
        t0 = time.perf_counter()
        result["digests"][_key(n, dtype)] = digests(n, dtype)
        print(f"{_key(n, dtype)}: {time.perf_counter() - t0:.2f} s", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    if "--record" not in sys.argv:
        raise SystemExit(__doc__)
    _record(sys.argv[1:])
