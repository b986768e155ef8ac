"""Multiplexed gates (include/qip_hipx.h: qipx_state_apply_multiplexed, qipx_multiplexed_table_bytes) without a GPU.

tests/multiplex_ref.py agrees with the existing CPU route: the same map goes through the oracle as one block-diagonal dense op on
the select and target qubits, and one table entry as the X-conjugated controlled op.  The stated arithmetic stays within the
header's (1.5 M + 3) u of an exact evaluation, and unit rows pass signed zeros and infinities bit for bit.  The plan
(rustqip_amd/csrc/qip_multiplex_plan.h) is plain C++: a stand-alone program (tests/cpp/test_multiplex_plan.cpp) walks every block,
wave, step and lane as the kernel does and compares with the definition, under the host sanitizers.  qipx_multiplexed_table_bytes
sizes the table and refuses malformed registers with the call's own messages, and the call itself refuses a null handle: there is
no CPU fall-back.  The chain prepare_register issues reaches its target within (9k + 8) u."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import function_ref as F
import multiplex_ref as R
import rustqip_amd as q
from rustqip_amd import _ffi, multiplex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_ORACLE_CASES = [
    (8, [3, 0], [6]),            # m + k = 3
    (8, [], [7, 2]),             # a plain 2-qubit gate, scrambled
    (9, [8, 1, 4], [0, 6]),      # m + k = 5
    (10, [2, 9, 5, 0], [7, 3]),  # m + k = 6
    (10, [9, 8, 7, 6, 5], [0]),
    (6, [5, 0, 3, 1], [4, 2]),   # m + k = n
    (7, [4], [1]),
]


@pytest.mark.parametrize("n,select,targets", _ORACLE_CASES)
def test_reference_is_the_block_diagonal_dense_op_through_the_oracle(oracle, n, select, targets):
    """allclose at a few u of the group's norm product, not equality: the oracle also adds the zero products of the other blocks"""
    rng = np.random.default_rng(100 * n + len(select))
    table = R.unitary_table(rng, len(select), len(targets))
    op = q.make_matrix_op(R.index_order(select, targets), R.block_diagonal(table))
    for dtype in R.DTYPES:
        x = R.make_state(n, 5 + n, dtype)
        want = np.zeros_like(x)
        oracle.apply_op_overwrite(n, op, x, want)
        got = R.apply_multiplexed_spec(n, x, select, targets, table)
        scale = R.norm_products(n, x, select, targets, table)
        err = np.abs(got.astype(np.complex128) - want.astype(np.complex128)) / (R.UNIT[dtype] * scale)
        assert float(err.max()) <= 2 * R.BAR[len(targets)], (n, select, targets, float(err.max()))
        assert not np.allclose(got, x)


@pytest.mark.parametrize("n,select,targets,xv", [(7, [5, 1, 3], [2], 0b010), (8, [0, 6], [7, 3], 0b01), (6, [4], [0, 5], 0)])
def test_one_entry_is_the_x_conjugated_controlled_op(oracle, n, select, targets, xv):
    rng = np.random.default_rng(7 * n)
    M = 2 ** len(targets)
    table = np.tile(np.eye(M, dtype=np.complex128), (2 ** len(select), 1, 1))
    table[xv] = R.unitary_table(rng, 0, len(targets))[0]
    flips = [q.make_matrix_op([s], [0, 1, 1, 0]) for i, s in enumerate(select) if not (xv >> i) & 1]
    ctl = q.make_control_op(select, q.make_matrix_op(list(targets)[::-1], table[xv]))
    for dtype in R.DTYPES:
        x = R.make_state(n, 11 + n, dtype)
        cur = x.copy()
        for op in flips + [ctl] + flips:
            nxt = np.zeros_like(cur)
            oracle.apply_op_overwrite(n, op, cur, nxt)
            cur = nxt
        got = R.apply_multiplexed_spec(n, x, select, targets, table)
        scale = R.norm_products(n, x, select, targets, table)
        err = np.abs(got.astype(np.complex128) - cur.astype(np.complex128)) / (R.UNIT[dtype] * scale)
        assert float(err.max()) <= 2 * R.BAR[len(targets)], (n, float(err.max()))
        untouched = R.gather(n, np.arange(2 ** n, dtype=np.uint64), select) != xv
        assert np.array_equal(got[untouched].view(np.uint8), x[untouched].view(np.uint8))
        assert not np.array_equal(got[~untouched], x[~untouched])


@pytest.mark.parametrize("k", (1, 2))
@pytest.mark.parametrize("dtype", R.DTYPES, ids=("c128", "c64"))
def test_spec_arithmetic_is_within_the_stated_bound_of_exact(dtype, k):
    """|y_a - exact| <= (1.5 M + 3) u |U_x[a]|_2 |v|_2 on unitary, real and wildly scaled matrices"""
    n, m = 12, 6
    select, targets = [11, 0, 5, 7, 2, 9], [3, 8][:k]
    u = R.UNIT[dtype]
    for kind, make in R.TABLES.items():
        worst = 0.0
        for seed in range(4):
            rng = np.random.default_rng(1000 * k + seed)
            table = make(rng, m, k)
            x = R.make_state(n, 40 + seed, dtype)
            if kind == "scaled":
                x = (x * 10.0 ** rng.uniform(-6, 6, size=len(x))).astype(dtype)
            spec = R.apply_multiplexed_spec(n, x, select, targets, table)
            exact = R.apply_multiplexed_exact(n, x, select, targets, table)
            scale = R.norm_products(n, x, select, targets, table)
            ratio = float(np.max(np.abs(spec.astype(exact.dtype) - exact).astype(np.float64) / (u * scale)))
            worst = max(worst, ratio)
        print(f"{np.dtype(dtype).name} k={k} {kind}: worst |spec - exact| = {worst:.2f} u |U_x[a]| |v| (bar {R.BAR[k]})")
        assert worst <= R.BAR[k], (kind, worst)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=("c128", "c64"))
def test_identity_rows_keep_signed_zeros_and_infinities(dtype):
    n, select, targets = 8, [0, 5], [3, 6]
    rng = np.random.default_rng(3)
    table, ident = R.with_identities(rng, R.unitary_table(rng, 2, 2), share=0.5)
    ident[1] = True
    table[1] = np.eye(4)
    table[2] = np.diag([1, 1, 1j, 1])  # rows 0, 1 and 3 are unit rows, row 2 is not
    ident[2] = False
    x = np.array(R.make_state(n, 9, dtype))
    j = np.arange(2 ** n, dtype=np.uint64)
    xs, a = R.gather(n, j, select), R.gather(n, j, targets)
    special = np.flatnonzero(ident[xs] | ((xs == 2) & (a != 2)))
    x[special[0::4]] = complex(-0.0, -0.0)
    x[special[1::4]] = complex(np.inf, -0.0)
    x[special[2::4]] = complex(-0.0, -np.inf)
    got = R.apply_multiplexed_spec(n, x, select, targets, table)
    assert np.array_equal(got[special].view(np.uint8), x[special].view(np.uint8))
    rest = np.flatnonzero(~ident[xs] & (xs != 2))
    assert np.all(np.isfinite(got[rest])) and not np.array_equal(got[rest], x[rest])


def test_plan_header_is_plain_cpp_and_visits_every_index_once_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "test_multiplex_plan")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "rustqip_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "test_multiplex_plan.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, " ".join(cmd) + "\n" + res.stdout + res.stderr
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and "multiplex plan ok" in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]


def test_table_bytes():
    assert q.multiplexed_table_bytes(10, [0, 1, 2], [5]) == 8 * 4 * 16
    assert q.multiplexed_table_bytes(10, [0, 1, 2], [5, 6], np.complex64) == 8 * 16 * 8
    assert q.multiplexed_table_bytes(1, [], [0]) == 4 * 16
    assert q.multiplexed_table_bytes(30, list(range(16)), [20, 29]) == 16 << 20  # m + 2k = 20: the largest table
    assert q.multiplexed_table_bytes(30, list(range(18)), [29], np.complex64) == 8 << 20


_REFUSALS = [
    (8, [0, 8], [1], "qubit 8 out of range"),
    (8, [0], [9], "qubit 9 out of range"),
    (8, [0, 3, 0], [1], "qubit 0 repeated"),
    (8, [0], [1, 1], "qubit 1 repeated"),
    (8, [0, 2], [2], "qubit 2 is in both registers"),
    (8, [0], [], "0 target qubits, 1 or 2 are supported"),
    (8, [0], [1, 2, 3], "3 target qubits, 1 or 2 are supported"),
    (30, list(range(19)), [29], "19 select and 1 target qubits, m + 2k is at most 20"),
    (30, list(range(17)), [28, 29], "17 select and 2 target qubits, m + 2k is at most 20"),
]


@pytest.mark.parametrize("n,select,targets,message", _REFUSALS)
def test_table_bytes_refuses_with_the_calls_messages(n, select, targets, message):
    with pytest.raises(q.CircuitError) as e:
        q.multiplexed_table_bytes(n, select, targets)
    assert str(e.value) == "apply_multiplexed: " + message


def test_null_arrays_and_null_handle_are_refused():
    out = C.c_uint64(7)
    one = (C.c_uint64 * 1)(0)
    lib = _ffi.lib
    assert lib.qipx_multiplexed_table_bytes(_ffi.QIP_C64, 4, None, 1, one, 1, C.byref(out)) == _ffi.QIP_ERR_INVALID
    assert _ffi.last_error() == "apply_multiplexed: null qubit array" and out.value == 0
    assert lib.qipx_multiplexed_table_bytes(_ffi.QIP_C64, 4, one, 0, None, 1, C.byref(out)) == _ffi.QIP_ERR_INVALID
    assert _ffi.last_error() == "apply_multiplexed: null qubit array"
    assert lib.qipx_multiplexed_table_bytes(99, 4, None, 0, one, 1, C.byref(out)) == _ffi.QIP_ERR_INVALID
    assert lib.qipx_multiplexed_table_bytes(_ffi.QIP_C64, 4, None, 0, one, 1, None) == _ffi.QIP_ERR_INVALID
    # no CPU fall-back: without a device there is no handle, and a null handle is refused
    mats = (C.c_double * 8)(1, 0, 0, 0, 0, 0, 1, 0)
    assert lib.qipx_state_apply_multiplexed(None, None, 0, one, 1, mats) == _ffi.QIP_ERR_INVALID
    assert "null state handle" in _ffi.last_error()


def test_python_layer_checks_the_table_shape():
    class NoDevice:
        def apply_multiplexed(self, select, targets, matrices):
            self.got = (list(select), list(targets), np.asarray(matrices))

    st = NoDevice()
    multiplex.controlled(st, [7], [1, 2], [4], R.unitary_table(np.random.default_rng(0), 2, 1))
    sel, tgt, table = st.got
    assert sel == [1, 2, 7] and tgt == [4] and table.shape == (8, 2, 2)
    assert np.array_equal(table[:4], np.tile(np.eye(2), (4, 1, 1))) and not np.allclose(table[4:], np.eye(2))
    with pytest.raises(q.CircuitError):
        multiplex.select_gates(st, [1, 2], [4], np.zeros((3, 2, 2)))
    with pytest.raises(q.CircuitError):
        multiplex.rotation(st, "y", [1, 2], 4, [0.1, 0.2])
    with pytest.raises(q.CircuitError):
        multiplex.rotation(st, "w", [1], 4, [0.1, 0.2])
    with pytest.raises(q.CircuitError):
        multiplex.prepare_tables([1.0, 1.0])  # not normalised
    th = np.array([0.3, -1.1])
    for axis, gen in (("x", [[0, 1], [1, 0]]), ("y", [[0, -1j], [1j, 0]]), ("z", [[1, 0], [0, -1]])):
        want = [np.cos(t / 2) * np.eye(2) - 1j * np.sin(t / 2) * np.array(gen) for t in th]
        assert np.allclose(multiplex.rotation_matrices(axis, th), want, rtol=0, atol=1e-16)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=("c128", "c64"))
def test_prepare_register_chain_reaches_the_amplitudes(dtype):
    """k spec passes and the function reference's phase pass from |0..0>: |got - psi|_2 <= (9k + 8) u |psi|_2 for k = 1 .. 8 (6 u per
    pass, 3 u for the host's angles and trigonometry, 8 u for the phase pass)"""
    u = R.UNIT[dtype]
    for k in range(1, 9):
        worst = 0.0
        for seed, zero_branch in ((0, False), (1, True), (2, False)):
            psi = R.random_amplitudes(np.random.default_rng(50 * k + seed), k, zero_branch)
            tables, phases = R.ry_chain(psi)
            angles, phases2 = multiplex.prepare_tables(psi)
            assert np.array_equal(phases, phases2)
            qubits = list(range(k))[::-1] if seed else list(range(k))
            x = np.zeros(2 ** k, dtype=dtype)
            x[0] = 1
            for i, t in enumerate(tables):
                assert np.array_equal(t.view(np.uint8), multiplex.rotation_matrices("y", angles[i]).view(np.uint8))
                x = R.apply_multiplexed_spec(k, x, qubits[:i], [qubits[i]], t)
            got = F.apply_function_ref(k, x, qubits, [], None, phases)
            want = np.empty(2 ** k, dtype=np.complex128)
            want[F.scatter(k, np.arange(2 ** k, dtype=np.uint64), qubits).astype(np.int64)] = psi
            worst = max(worst, float(np.linalg.norm(got - want) / u))
        print(f"{np.dtype(dtype).name} k={k}: worst |got - psi|_2 = {worst:.2f} u (bar {9 * k + 8})")
        assert worst <= 9 * k + 8, (k, worst)
