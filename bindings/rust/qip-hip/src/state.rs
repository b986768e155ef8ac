//! `HipState`: the device-resident `2^n` amplitude vector (`state` + `arena` of `builder.rs:406-407`).
use crate::op::{marshal, HipPrecision};
use crate::sys;
use crate::sys_ext;
use num_complex::Complex;
use qip_iterators::iterators::MatrixOp;
use std::ffi::{CStr, CString};
use std::marker::PhantomData;

/// A non-zero status of the C ABI with the library's message (`qip_hip_last_error`).
#[derive(Debug, Clone)]
pub struct HipError {
    pub code: i32,
    pub message: String,
}
impl std::fmt::Display for HipError {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        write!(f, "qip_hip error {}: {}", self.code, self.message)
    }
}
impl std::error::Error for HipError {}

pub(crate) fn check(rc: i32) -> Result<(), HipError> {
    if rc == sys::QIP_OK {
        return Ok(());
    }
    let message = unsafe { CStr::from_ptr(sys::qip_hip_last_error()) }.to_string_lossy().into_owned();
    Err(HipError { code: rc, message })
}

/// The term arrays of `include/qip_hipx.h` for the diagonal calls: (term_start, qubits, paulis, coefficients), every array with one
/// spare element so that none is a dangling pointer for an empty list.
fn diagonal_arrays(terms: &[Vec<(u64, u8)>], coeffs: &[f64]) -> (Vec<u64>, Vec<u64>, Vec<u8>, Vec<f64>) {
    let mut start = vec![0u64];
    let (mut qubits, mut paulis) = (Vec::new(), Vec::new());
    for term in terms {
        for &(q, p) in term {
            qubits.push(q);
            paulis.push(p);
        }
        start.push(qubits.len() as u64);
    }
    qubits.push(0);
    paulis.push(0);
    let mut c = coeffs.to_vec();
    c.push(0.0);
    (start, qubits, paulis, c)
}

pub struct HipState<P: HipPrecision = f64> {
    n: usize,
    h: *mut sys::qip_hip_state,
    _p: PhantomData<P>,
}

// One host thread drives a handle at a time (the reference's run loop is sequential, builder.rs:423-517);
// moving it to another thread is fine, sharing it is not.
unsafe impl<P: HipPrecision> Send for HipState<P> {}

impl<P: HipPrecision> HipState<P> {
    /// `2^n` `Complex<P>` amplitudes (+ as much scratch) in the HBM of `device`.  Fails when no gfx950 device
    /// is visible: there is no CPU fallback.
    pub fn new(n: usize, device: i32) -> Result<Self, HipError> {
        let mut h = std::ptr::null_mut();
        check(unsafe { sys::qip_hip_state_create(n as u32, P::DTYPE, device, &mut h) })?;
        Ok(Self { n, h, _p: PhantomData })
    }
    pub fn n(&self) -> usize {
        self.n
    }
    pub fn set_option(&mut self, key: &str, value: i64) -> Result<(), HipError> {
        let k = CString::new(key).expect("option key without NUL");
        check(unsafe { sys::qip_hip_state_set_option(self.h, k.as_ptr(), value) })
    }
    /// new[j] = old[src(j)], bit pi[d] of src(j) = bit d of j: any permutation of the index bits in one sweep
    /// (what a run of `Swap` ops composes to, qip-iterators/src/iterators/qubit_iterators.rs:208-218).
    pub fn permute_bits(&mut self, pi: &[u32]) -> Result<(), HipError> {
        assert_eq!(pi.len(), self.n, "the permutation must list all n index bits");
        check(unsafe { sys::qip_hip_state_permute_bits(self.h, pi.as_ptr()) })
    }
    /// |index> (builder.rs:409-421).
    pub fn init_basis(&mut self, index: usize) -> Result<(), HipError> {
        check(unsafe { sys::qip_hip_state_init_basis(self.h, index as u64) })
    }
    pub fn upload(&mut self, amps: &[Complex<P>], offset: usize) -> Result<(), HipError> {
        check(unsafe { sys::qip_hip_state_upload(self.h, amps.as_ptr() as *const _, offset as u64, amps.len() as u64) })
    }
    pub fn download(&self) -> Result<Vec<Complex<P>>, HipError> {
        let mut out = vec![Complex::new(P::zero(), P::zero()); 1usize << self.n];
        check(unsafe { sys::qip_hip_state_download(self.h, out.as_mut_ptr() as *mut _, 0, out.len() as u64) })?;
        Ok(out)
    }
    /// `apply_op_overwrite` + buffer swap of the reference run loop (builder.rs:499,514), in place on the device.
    pub fn apply_op(&mut self, op: &MatrixOp<Complex<P>>) -> Result<(), HipError> {
        let c = marshal(op);
        check(unsafe { sys::qip_hip_state_apply_op(self.h, c.as_ptr()) })
    }
    /// A run of gates in one call, so the library may schedule them (options "tile", "fuse").
    pub fn apply_ops(&mut self, ops: &[MatrixOp<Complex<P>>]) -> Result<(), HipError> {
        let keep: Vec<_> = ops.iter().map(marshal).collect();
        let flat: Vec<sys::qip_op> = keep.iter().map(|c| unsafe { std::ptr::read(c.as_ptr()) }).collect();
        let rc = unsafe { sys::qip_hip_state_apply_ops(self.h, flat.as_ptr(), flat.len() as u64) };
        std::mem::forget(flat); // bitwise copies of descriptors that `keep` owns
        check(rc)
    }
    /// `self <- other`, device to device (same n, precision and device).
    pub fn copy_from(&mut self, other: &mut HipState<P>) -> Result<(), HipError> {
        check(unsafe { sys::qip_hip_state_copy_from(self.h, other.h) })
    }
    /// `(max_i |self_i - other_i|, number of amplitudes that are not IEEE-equal)` over the whole vector, on the device:
    /// what the parity checks use to hold a state against a reference copy.
    pub fn max_abs_diff(&mut self, other: &mut HipState<P>) -> Result<(f64, u64), HipError> {
        let (mut worst, mut differ) = (0.0f64, 0u64);
        check(unsafe { sys::qip_hip_state_max_abs_diff(self.h, other.h, &mut worst, &mut differ) })?;
        Ok((worst, differ))
    }
    /// Amplitudes at an explicit list of indices (one gather kernel): a logical window of a sharded / relabelled state.
    pub fn download_indices(&mut self, indices: &[u64]) -> Result<Vec<Complex<P>>, HipError> {
        let mut out = vec![Complex::new(P::zero(), P::zero()); indices.len()];
        check(unsafe { sys::qip_hip_state_download_indices(self.h, indices.as_ptr(), indices.len() as u64, out.as_mut_ptr() as *mut _) })?;
        Ok(out)
    }
    pub fn norm_sqr(&self) -> Result<f64, HipError> {
        let mut v = 0.0;
        check(unsafe { sys::qip_hip_state_norm_sqr(self.h, &mut v) })?;
        Ok(v)
    }
    /// `measure_probs` (measurement_ops.rs:115-127).
    pub fn measure_probs(&self, indices: &[usize]) -> Result<Vec<f64>, HipError> {
        let idx: Vec<u64> = indices.iter().map(|&i| i as u64).collect();
        let mut out = vec![0.0; 1usize << idx.len()];
        check(unsafe { sys::qip_hip_state_measure_probs(self.h, idx.as_ptr(), idx.len() as u32, out.as_mut_ptr()) })?;
        Ok(out)
    }
    /// `measure` (measurement_ops.rs:190-214): sample with `rand_u01` (or force `measured`), collapse, renormalise.
    pub fn measure(&mut self, indices: &[usize], forced: Option<usize>, rand_u01: f64) -> Result<(usize, f64), HipError> {
        let idx: Vec<u64> = indices.iter().map(|&i| i as u64).collect();
        let (mut m, mut p) = (0u64, 0f64);
        let f = forced.map(|v| v as i64).unwrap_or(-1);
        check(unsafe { sys::qip_hip_state_measure(self.h, idx.as_ptr(), idx.len() as u32, f, rand_u01, &mut m, &mut p) })?;
        Ok((m as usize, p))
    }
    /// Many samples of the state in one call (`include/qip_hipx.h`, beyond the reference's interface): element `j` is the
    /// outcome `soft_measure` (measurement_ops.rs:153-176) gives for `rand_u01[j]`, all of them for about the cost of two
    /// single samples.  The state is not changed.
    pub fn soft_measure_many(&self, indices: &[u64], rand_u01: &[f64]) -> Result<Vec<u64>, HipError> {
        let mut out = vec![0u64; rand_u01.len()];
        check(unsafe {
            sys_ext::qipx_state_soft_measure_many(self.h, indices.as_ptr(), indices.len() as u32, rand_u01.as_ptr(), rand_u01.len() as u64, out.as_mut_ptr())
        })?;
        Ok(out)
    }
    /// <psi| P |psi> of Pauli strings (`include/qip_hipx.h`, beyond the reference's interface): a term is a list of
    /// `(qubit, code)` with code 0 = I, 1 = X, 2 = Y, 3 = Z.  The raw quadratic form (not divided by the norm), in double for
    /// both precisions; terms that share their X/Y qubits share passes over the vector.  The state is not changed.
    pub fn expect_pauli(&self, terms: &[Vec<(u64, u8)>]) -> Result<Vec<f64>, HipError> {
        let mut start = vec![0u64];
        let (mut qubits, mut paulis) = (Vec::new(), Vec::new());
        for term in terms {
            for &(q, p) in term {
                qubits.push(q);
                paulis.push(p);
            }
            start.push(qubits.len() as u64);
        }
        // (never a dangling-but-null pointer question on the C side: the arrays hold at least one element)
        qubits.push(0);
        paulis.push(0);
        let mut out = vec![0f64; terms.len()];
        check(unsafe {
            sys_ext::qipx_state_expect_pauli(self.h, start.as_ptr(), qubits.as_ptr(), paulis.as_ptr(), terms.len() as u64, out.as_mut_ptr())
        })?;
        Ok(out)
    }
    /// psi <- exp(-i * angles[t] * P_t) psi for every term, in the order given (`include/qip_hipx.h`): terms as for
    /// `expect_pauli`.  One in-place pass per run of consecutive terms with the same X/Y qubits; queued on the stream, returns
    /// without waiting.
    pub fn apply_pauli_rotations(&mut self, terms: &[Vec<(u64, u8)>], angles: &[f64]) -> Result<(), HipError> {
        assert_eq!(terms.len(), angles.len(), "one angle per term");
        let mut start = vec![0u64];
        let (mut qubits, mut paulis) = (Vec::new(), Vec::new());
        for term in terms {
            for &(q, p) in term {
                qubits.push(q);
                paulis.push(p);
            }
            start.push(qubits.len() as u64);
        }
        qubits.push(0);
        paulis.push(0);
        check(unsafe {
            sys_ext::qipx_state_apply_pauli_rotations(self.h, start.as_ptr(), qubits.as_ptr(), paulis.as_ptr(), angles.as_ptr(), terms.len() as u64)
        })
    }
    /// psi[j] <- exp(-i gamma D(j)) psi[j] for the diagonal sum D = sum_t coeffs[t] P_t (`include/qip_hipx.h`): terms as for
    /// `expect_pauli` with factors I (0) and Z (3) only.  ONE in-place pass whatever the number of terms; queued on the stream,
    /// returns without waiting.
    pub fn apply_diagonal(&mut self, terms: &[Vec<(u64, u8)>], coeffs: &[f64], gamma: f64) -> Result<(), HipError> {
        assert_eq!(terms.len(), coeffs.len(), "one coefficient per term");
        let (start, qubits, paulis, c) = diagonal_arrays(terms, coeffs);
        check(unsafe {
            sys_ext::qipx_state_apply_diagonal(self.h, start.as_ptr(), qubits.as_ptr(), paulis.as_ptr(), c.as_ptr(), terms.len() as u64, gamma)
        })
    }
    /// (sum_j |psi_j|^2 D(j), sum_j |psi_j|^2 D(j)^2) for the same D: raw, in double for both precisions, one pass; the state is
    /// not changed.
    pub fn expect_diagonal(&self, terms: &[Vec<(u64, u8)>], coeffs: &[f64]) -> Result<(f64, f64), HipError> {
        assert_eq!(terms.len(), coeffs.len(), "one coefficient per term");
        let (start, qubits, paulis, c) = diagonal_arrays(terms, coeffs);
        let mut out = [0f64; 2];
        check(unsafe {
            sys_ext::qipx_state_expect_diagonal(self.h, start.as_ptr(), qubits.as_ptr(), paulis.as_ptr(), c.as_ptr(), terms.len() as u64, out.as_mut_ptr())
        })?;
        Ok((out[0], out[1]))
    }
    /// self <- H src, or self + H src when `accumulate`, for H = sum_t coeffs[t] P_t (`include/qip_hipx.h`): terms as for
    /// `expect_pauli`, coefficients as `(re, im)`; `src` is another state of the same size, precision and device and is not
    /// changed.  Complete when it returns.
    pub fn apply_pauli_sum(&mut self, src: &mut HipState<P>, terms: &[Vec<(u64, u8)>], coeffs: &[(f64, f64)], accumulate: bool) -> Result<(), HipError> {
        assert_eq!(terms.len(), coeffs.len(), "one coefficient per term");
        let mut start = vec![0u64];
        let (mut qubits, mut paulis) = (Vec::new(), Vec::new());
        for term in terms {
            for &(q, p) in term {
                qubits.push(q);
                paulis.push(p);
            }
            start.push(qubits.len() as u64);
        }
        qubits.push(0);
        paulis.push(0);
        let mut flat: Vec<f64> = coeffs.iter().flat_map(|&(re, im)| [re, im]).collect();
        flat.push(0.0);
        check(unsafe {
            sys_ext::qipx_state_apply_pauli_sum(self.h, src.h, start.as_ptr(), qubits.as_ptr(), paulis.as_ptr(), flat.as_ptr(), terms.len() as u64, accumulate as i32)
        })
    }
    /// `<self| P |ket>` of Pauli strings as `(re, im)` (`include/qip_hipx.h`): raw, in double for both precisions; an empty term
    /// gives `<self|ket>`.  Neither state is changed.  (For the Hermitian case `<psi| P |psi>` use `expect_pauli`: two `&mut` to
    /// one state cannot be had.)
    pub fn pauli_matrix_elements(&mut self, ket: &mut HipState<P>, terms: &[Vec<(u64, u8)>]) -> Result<Vec<(f64, f64)>, HipError> {
        let mut start = vec![0u64];
        let (mut qubits, mut paulis) = (Vec::new(), Vec::new());
        for term in terms {
            for &(q, p) in term {
                qubits.push(q);
                paulis.push(p);
            }
            start.push(qubits.len() as u64);
        }
        qubits.push(0);
        paulis.push(0);
        let mut flat = vec![0f64; 2 * terms.len()];
        check(unsafe {
            sys_ext::qipx_state_pauli_matrix_elements(self.h, ket.h, start.as_ptr(), qubits.as_ptr(), paulis.as_ptr(), terms.len() as u64, flat.as_mut_ptr())
        })?;
        Ok(flat.chunks(2).map(|c| (c[0], c[1])).collect())
    }
    /// `<self|other>` as `(re, im)`: `pauli_matrix_elements` with the empty term.
    pub fn inner(&mut self, other: &mut HipState<P>) -> Result<(f64, f64), HipError> {
        Ok(self.pauli_matrix_elements(other, &[Vec::new()])?[0])
    }
    /// The raw reduced density matrix of up to six qubits (`include/qip_hipx.h`): `2^k` rows of `2^k` entries `(re, im)`,
    /// `rho[a][a'] = sum_b psi[a,b] conj(psi[a',b])`, bit `i` of `a` = qubit `indices[i]`; not divided by the norm.  The lower
    /// triangle is the exact conjugate of the upper.  The state is not changed.
    pub fn reduced_density_matrix(&mut self, indices: &[u64]) -> Result<Vec<Vec<(f64, f64)>>, HipError> {
        let m = 1usize << indices.len().min(6);
        let mut flat = vec![0f64; 2 * m * m];
        check(unsafe { sys_ext::qipx_state_reduced_density(self.h, indices.as_ptr(), indices.len() as u32, flat.as_mut_ptr()) })?;
        Ok(flat.chunks(2 * m).map(|row| row.chunks(2).map(|c| (c[0], c[1])).collect()).collect())
    }
    /// The raw reduced transition matrix of up to three qubits (`include/qip_hipx.h`), `self` the bra: `2^k` rows of `2^k` entries
    /// `(re, im)`, `m[a][a'] = sum_b ket[a,b] conj(self[a',b])`, bit `i` of `a` = qubit `indices[i]`; `<self| A |ket> = Tr(A m)` for
    /// every operator `A` on those qubits.  Neither state is changed.
    pub fn transition_matrix(&mut self, ket: &mut HipState<P>, indices: &[u64]) -> Result<Vec<Vec<(f64, f64)>>, HipError> {
        let m = 1usize << indices.len().min(3);
        let mut flat = vec![0f64; 2 * m * m];
        check(unsafe { sys_ext::qipx_state_transition_matrix(self.h, ket.h, indices.as_ptr(), indices.len() as u32, flat.as_mut_ptr()) })?;
        Ok(flat.chunks(2 * m).map(|row| row.chunks(2).map(|c| (c[0], c[1])).collect()).collect())
    }
    /// `self[j] <- own * self[j] + sum_i coeffs[i] * others[i][j]` in one pass (`include/qip_hipx.h`), coefficients as
    /// `(re, im)`: `self` is the first source when `own` is given (two `&mut` to one state cannot be had, so the state itself
    /// is named this way), at most 16 sources in all, none: `self <- 0`.  With `want_norm` the pass also returns
    /// `sum_j |self[j]|^2` of the stored amplitudes.  Complete when it returns.
    pub fn linear_combination(&mut self, own: Option<(f64, f64)>, others: &mut [&mut HipState<P>], coeffs: &[(f64, f64)], want_norm: bool) -> Result<Option<f64>, HipError> {
        assert_eq!(others.len(), coeffs.len(), "one coefficient per source");
        let mut handles: Vec<*mut sys::qip_hip_state> = Vec::new();
        let mut flat: Vec<f64> = Vec::new();
        if let Some((re, im)) = own {
            handles.push(self.h);
            flat.extend_from_slice(&[re, im]);
        }
        for (s, &(re, im)) in others.iter().zip(coeffs) {
            handles.push(s.h);
            flat.extend_from_slice(&[re, im]);
        }
        let count = handles.len() as u32;
        handles.push(std::ptr::null_mut());
        flat.push(0.0);
        let mut norm = 0f64;
        check(unsafe {
            sys_ext::qipx_state_linear_combination(self.h, handles.as_ptr(), flat.as_ptr(), count, if want_norm { &mut norm } else { std::ptr::null_mut() })
        })?;
        Ok(if want_norm { Some(norm) } else { None })
    }
    /// `<bras[i]|self>` as `(re, im)` for up to 16 states in one pass over all of them (`include/qip_hipx.h`), in double for both
    /// precisions; a batch equals its single-bra calls bit for bit.  No state is changed.
    pub fn inner_products(&mut self, bras: &mut [&mut HipState<P>]) -> Result<Vec<(f64, f64)>, HipError> {
        let mut handles: Vec<*mut sys::qip_hip_state> = bras.iter().map(|b| b.h).collect();
        let count = handles.len() as u32;
        handles.push(std::ptr::null_mut());
        let mut flat = vec![0f64; 2 * bras.len() + 1];
        check(unsafe { sys_ext::qipx_state_inner_products(handles.as_ptr(), count, self.h, flat.as_mut_ptr()) })?;
        flat.truncate(2 * bras.len());
        Ok(flat.chunks(2).map(|c| (c[0], c[1])).collect())
    }
    pub fn raw(&mut self) -> *mut sys::qip_hip_state {
        self.h
    }
}

impl<P: HipPrecision> Drop for HipState<P> {
    fn drop(&mut self) {
        unsafe { sys::qip_hip_state_destroy(self.h) };
    }
}
