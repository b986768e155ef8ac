//! Raw bindings of `include/qip_hipx.h`: capabilities beyond the reference's interface (prefix `qipx_`, versioned on their own:
//! `QIPX_ABI_VERSION`).  `sys.rs` stays the binding contract of `include/qip_hip.h`; `tests/test_hipx_contract_cpu.py` compares
//! this file with the header.
use crate::sys::qip_hip_state;
use std::os::raw::{c_char, c_double, c_int};

pub const QIPX_ABI_VERSION: c_int = 1;
/// `flags` of `qipx_state_apply_qft`: the inverse transform; the register's bits in reversed order on the transformed side.
pub const QIPX_QFT_INVERSE: u32 = 1;
pub const QIPX_QFT_REVERSED: u32 = 2;

/// `struct qipx_channel`: `count` Kraus operators of 2 * 4^k doubles each (row-major, bit i of a row = qubit `indices[i]`) on
/// the `k` qubits `indices`.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct qipx_channel {
    pub indices: *const u64,
    pub k: u32,
    pub kraus: *const c_double,
    pub count: u32,
}

extern "C" {
    pub fn qipx_abi_version() -> c_int;
    /// `measured[j]` = the outcome of the single-sample call for `rand_u01[j]`, `j < count`; the state is not changed.
    pub fn qipx_state_soft_measure_many(
        s: *mut qip_hip_state,
        indices: *const u64,
        k: u32,
        rand_u01: *const c_double,
        count: u64,
        measured: *mut u64,
    ) -> c_int;
    /// `values[t]` = <psi| P_t |psi>, `t < count`: term `t` is the product of `paulis[i]` (0 = I, 1 = X, 2 = Y, 3 = Z) on qubit
    /// `qubits[i]` for `term_start[t] <= i < term_start[t+1]`; the raw quadratic form, the state is not changed.
    pub fn qipx_state_expect_pauli(
        s: *mut qip_hip_state,
        term_start: *const u64,
        qubits: *const u64,
        paulis: *const u8,
        count: u64,
        values: *mut c_double,
    ) -> c_int;
    /// Host only: the passes over the vector the call above makes when at most `group` terms share one (0 = the default).
    pub fn qipx_expect_pauli_passes(
        n: u32,
        term_start: *const u64,
        qubits: *const u64,
        paulis: *const u8,
        count: u64,
        group: u32,
        passes: *mut u64,
    ) -> c_int;
    /// psi <- exp(-i * angles[t] * P_t) psi for `t < count`, in the order given; the terms as for `qipx_state_expect_pauli`.
    /// Queued on the handle's stream, returns without waiting.
    pub fn qipx_state_apply_pauli_rotations(
        s: *mut qip_hip_state,
        term_start: *const u64,
        qubits: *const u64,
        paulis: *const u8,
        angles: *const c_double,
        count: u64,
    ) -> c_int;
    /// Host only: the passes over the vector the call above makes when at most `group` consecutive terms of one X/Y mask
    /// share one (0 = the default).
    pub fn qipx_pauli_rotation_passes(
        n: u32,
        term_start: *const u64,
        qubits: *const u64,
        paulis: *const u8,
        count: u64,
        group: u32,
        passes: *mut u64,
    ) -> c_int;
    /// dst <- H src (or dst + H src when `accumulate` is non-zero), H = sum_t (coeffs[2t] + i coeffs[2t+1]) P_t; the terms as
    /// for `qipx_state_expect_pauli`.  dst != src, same n, precision and device.  Complete when it returns.
    pub fn qipx_state_apply_pauli_sum(
        dst: *mut qip_hip_state,
        src: *mut qip_hip_state,
        term_start: *const u64,
        qubits: *const u64,
        paulis: *const u8,
        coeffs: *const c_double,
        count: u64,
        accumulate: c_int,
    ) -> c_int;
    /// Host only: the passes the call above makes when at most `group` terms of one X/Y mask share one (0 = the default).
    pub fn qipx_pauli_sum_passes(
        n: u32,
        term_start: *const u64,
        qubits: *const u64,
        paulis: *const u8,
        count: u64,
        group: u32,
        passes: *mut u64,
    ) -> c_int;
    /// values[2t] + i values[2t+1] = <bra| P_t |ket>, raw, in double for both precisions; an empty term gives <bra|ket>.
    /// bra == ket is allowed.  Neither state is changed.
    pub fn qipx_state_pauli_matrix_elements(
        bra: *mut qip_hip_state,
        ket: *mut qip_hip_state,
        term_start: *const u64,
        qubits: *const u64,
        paulis: *const u8,
        count: u64,
        values: *mut c_double,
    ) -> c_int;
    /// rho[2 (a M + a')] + i rho[.. + 1] = sum_b psi[a,b] conj(psi[a',b]), M = 2^k, 1 <= k <= 6: the raw reduced density matrix of
    /// the qubits `indices` (bit i of a = qubit indices[i]), in double for both precisions.  The state is not changed.
    pub fn qipx_state_reduced_density(s: *mut qip_hip_state, indices: *const u64, k: u32, rho: *mut c_double) -> c_int;
    /// m[2 (a M + a')] + i m[.. + 1] = sum_b ket[a,b] conj(bra[a',b]), M = 2^k, 1 <= k <= 3: the raw reduced transition matrix
    /// Tr_rest |ket><bra| of the qubits `indices` (bit i of a = qubit indices[i]), in double for both precisions.  Neither state
    /// is changed.  Complete when it returns.
    pub fn qipx_state_transition_matrix(bra: *mut qip_hip_state, ket: *mut qip_hip_state, indices: *const u64, k: u32, m: *mut c_double) -> c_int;
    /// dst[j] <- sum_i (coeffs[2i] + i coeffs[2i+1]) srcs[i][j], 1 <= count <= 16 (0: dst <- 0), in the state's precision; dst may
    /// be any of the sources.  A non-null `norm_sqr` receives sum_j |dst[j]|^2 of the stored values from the same pass.  Complete
    /// when it returns.
    pub fn qipx_state_linear_combination(
        dst: *mut qip_hip_state,
        srcs: *const *mut qip_hip_state,
        coeffs: *const c_double,
        count: u32,
        norm_sqr: *mut c_double,
    ) -> c_int;
    /// values[2i] + i values[2i+1] = <bras[i]|ket>, 1 <= count <= 16, in double for both precisions, one pass over all of them; a
    /// batch equals its single-bra calls bit for bit.  No state is changed.
    pub fn qipx_state_inner_products(bras: *const *mut qip_hip_state, count: u32, ket: *mut qip_hip_state, values: *mut c_double) -> c_int;
    /// psi[j] <- exp(-i gamma D(j)) psi[j], D(j) = sum_t coeffs[t] (-1)^popcount(j & z_t): the terms as for `qipx_state_expect_pauli`,
    /// factors I and Z only.  ONE in-place pass whatever `count` is; queued on the handle's stream, returns without waiting.
    pub fn qipx_state_apply_diagonal(
        s: *mut qip_hip_state,
        term_start: *const u64,
        qubits: *const u64,
        paulis: *const u8,
        coeffs: *const c_double,
        count: u64,
        gamma: c_double,
    ) -> c_int;
    /// moments[0] = sum_j |psi_j|^2 D(j), moments[1] = sum_j |psi_j|^2 D(j)^2 for the same D: raw, in double for both precisions,
    /// one pass; the state is not changed.  Complete when it returns.
    pub fn qipx_state_expect_diagonal(
        s: *mut qip_hip_state,
        term_start: *const u64,
        qubits: *const u64,
        paulis: *const u8,
        coeffs: *const c_double,
        count: u64,
        moments: *mut c_double,
    ) -> c_int;
    /// |x>|y> -> w(x) |x>|y'>: y' = y ^ values[x] (`mode` 0, QIPX_FN_XOR) or (y + values[x]) mod 2^k (`mode` 1, QIPX_FN_ADD), bit i of
    /// x / y = qubit in_qubits[i] / out_qubits[i]; w = 1 (null `phases`: amplitudes are moved with their bits) or
    /// (cos phases[x], sin phases[x]).  2^m entries; k = 0: null `values`, a phase by table.  In place, one pass per six out
    /// positions outside the six low index bits (ADD: at most six); queued on the handle's stream, returns without waiting.
    pub fn qipx_state_apply_function(
        s: *mut qip_hip_state,
        in_qubits: *const u64,
        m: u32,
        out_qubits: *const u64,
        k: u32,
        mode: c_int,
        values: *const u64,
        phases: *const c_double,
    ) -> c_int;
    /// The number of passes over the vector that `qipx_state_apply_function` makes on `n` qubits, after the same checks of the
    /// registers and the mode.  Host-only.
    pub fn qipx_function_passes(
        n: u32,
        in_qubits: *const u64,
        m: u32,
        out_qubits: *const u64,
        k: u32,
        mode: c_int,
        passes: *mut u32,
    ) -> c_int;
    /// |x>|t> -> |x> (U_x |t>) for all 2^m values x of the `select` register in one in-place pass: `matrices` holds 2^m row-major
    /// 2^k x 2^k complex matrices (re, im interleaved), bit i of x = qubit select[i], bit i of a row or column = qubit targets[i].
    /// k in {1, 2}, m + 2k <= 20.  Queued on the handle's stream, returns without waiting.
    pub fn qipx_state_apply_multiplexed(
        s: *mut qip_hip_state,
        select: *const u64,
        m: u32,
        targets: *const u64,
        k: u32,
        matrices: *const c_double,
    ) -> c_int;
    /// The bytes of the device table `qipx_state_apply_multiplexed` uploads for a state of `dtype` on `n` qubits, after the same
    /// checks of the registers.  Host-only.
    pub fn qipx_multiplexed_table_bytes(
        dtype: c_int,
        n: u32,
        select: *const u64,
        m: u32,
        targets: *const u64,
        k: u32,
        bytes: *mut u64,
    ) -> c_int;
    /// The quantum Fourier transform of the register `qubits` (bit i of its value = qubit qubits[i]) for every setting of the other
    /// qubits, in place: new[y] = 2^(-m/2) sum_x exp(+-2 pi i x y / 2^m) old[x], the minus sign with `QIPX_QFT_INVERSE`;
    /// `QIPX_QFT_REVERSED` leaves the forward result bit-reversed and reads the inverse's input in that order.  FFT passes over LDS
    /// tiles, per fibre within 8 m u of the exact transform.  Queued on the handle's stream, returns without waiting.
    pub fn qipx_state_apply_qft(
        s: *mut qip_hip_state,
        qubits: *const u64,
        m: u32,
        flags: u32,
    ) -> c_int;
    /// The passes over the vector that `qipx_state_apply_qft` makes for a state of `dtype` on `n` qubits, after the same checks.
    /// Host-only.
    pub fn qipx_qft_passes(
        dtype: c_int,
        n: u32,
        qubits: *const u64,
        m: u32,
        flags: u32,
        passes: *mut u32,
    ) -> c_int;
    /// psi <- (the 2^k x 2^k `matrix` on `indices`) psi in place, unitary or not, and `rho_next` = the raw reduced density matrix
    /// of the RESULT on `next_indices` from the same pass (conventions of `qipx_state_reduced_density`).  k, k2 in {1, 2}; the
    /// lists may overlap; together at most three qubits.  Complete on return.
    pub fn qipx_state_apply_reduce(
        s: *mut qip_hip_state,
        indices: *const u64,
        k: u32,
        matrix: *const c_double,
        next_indices: *const u64,
        k2: u32,
        rho_next: *mut c_double,
    ) -> c_int;
    /// One trajectory step through `nch` channels in order: branch i of channel c is drawn by `rand_u01[c]` with weight
    /// Re Tr(K_i^H K_i rho) and psi <- K_i psi, rescaled to the norm it had.  `chosen[c]` = i; `weights` (nullable) gets every
    /// channel's weights one after another.
    pub fn qipx_state_apply_channels(
        s: *mut qip_hip_state,
        ch: *const qipx_channel,
        nch: u64,
        rand_u01: *const c_double,
        chosen: *mut u32,
        weights: *mut c_double,
    ) -> c_int;
    /// The passes over the vector that `qipx_state_apply_channels` makes for the list on `n` qubits and how many of them are
    /// fused apply-and-reduce passes (for a Complex<f64> state), after the same checks of the list.  Host-only.
    pub fn qipx_channel_passes(n: u32, ch: *const qipx_channel, nch: u64, passes: *mut u64, fused: *mut u64) -> c_int;
    /// The same for the state `s` (its n and precision): the plan `qipx_state_apply_channels` runs on it.  Host-only.
    pub fn qipx_state_channel_passes(s: *mut qip_hip_state, ch: *const qipx_channel, nch: u64, passes: *mut u64, fused: *mut u64) -> c_int;
    /// The kernel classes of the profile: those of `qip_hip_kernel_class_count` under their indices, then the classes of the
    /// calls of this header.
    pub fn qipx_kernel_class_count() -> c_int;
    pub fn qipx_kernel_class_name(cls: c_int) -> *const c_char;
    pub fn qipx_state_profile_get(
        s: *mut qip_hip_state,
        cls: c_int,
        launches: *mut u64,
        total_ms: *mut c_double,
        algorithmic_bytes: *mut c_double,
    ) -> c_int;
}
