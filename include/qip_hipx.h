/*
 * qip_hipx.h — capabilities beyond the reference's interface.
 *
 * include/qip_hip.h is the binding contract: one entry point per function of the reference, nothing more.  What a device
 * state can do that the reference has no call for lives here, under the prefix `qipx_`, exported by libqip_hip.so under
 * the version-script node QIP_HIPX and versioned on its own (qipx_abi_version).  Handles, dtypes and error codes are
 * those of qip_hip.h; every function returns a QIP_* code and leaves its message in the library's last-error string.
 */
#ifndef QIP_HIPX_H
#define QIP_HIPX_H

#include "qip_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QIPX_ABI_VERSION 1

/* The version of THIS header the library was built from. */
int qipx_abi_version(void);

/* Many samples of one state in one call: measured[j], j < count, is the outcome the single-sample soft_measure call of
 * qip_hip.h returns for (s, indices, k, rand_u01[j]) on this state, in its default two-launch form — the same function of
 * the sample for Complex<f64> and Complex<f32>, for every double that call accepts: 0.0, samples at or above the norm
 * (amplitude index 0, measurement_ops.rs:166), samples of an unnormalised state.  What that call promises about the
 * reference's sample -> outcome map (exact for f64, the distribution for f32) therefore holds here too.  The result is in
 * input order; repeated and unsorted samples are fine.
 *
 * Cost: one pass over the vector for the chunk sums plus one read of every chunk a sample lands in, whatever `count` is;
 * the single call pays a whole pass per sample.
 *
 * The state is not changed.  The call is ordered after the work queued on the handle and complete when it returns.
 * count == 0 returns QIP_OK (null arrays allowed); with count > 0 a null `rand_u01` or `measured` is QIP_ERR_INVALID;
 * the index list is checked as for the single call.
 *
 * The samples are processed in slabs so that the device scratch (40 bytes per sample of a slab, owned by the handle, grown
 * on demand, freed with it) stays bounded: state option "sample_slab" (set through the set_option call of qip_hip.h) is the
 * number of samples per slab, default 1 << 22, at most 1 << 28 are used; values below 1 are refused with QIP_ERR_INVALID. */
int qipx_state_soft_measure_many(qip_hip_state* s, const uint64_t* indices, uint32_t k,
                                 const double* rand_u01, uint64_t count, uint64_t* measured);

/* Expectation values of Pauli strings.  (Added without a change of QIPX_ABI_VERSION: the addition is purely additive, every
 * earlier declaration is as it was.)
 *
 * values[t] = <psi| P_t |psi>, t < count.  Term t is the product of paulis[i] (0 = I, 1 = X, 2 = Y, 3 = Z) on qubit
 * qubits[i] for term_start[t] <= i < term_start[t+1]; qubit q is index bit n-1-q as everywhere in qip_hip.h.
 *
 * The value.  With x = the index bits under X or Y, z = those under Z or Y and n_Y the number of Y factors,
 *   values[t] = sum_j conj(psi[j ^ x]) * i^n_Y * (-1)^popcount(j & z) * psi[j],
 * the raw quadratic form: it is NOT divided by the norm, so an unnormalised state gives norm^2 times the value of the
 * normalised one.  An empty term (term_start[t] == term_start[t+1]), and a term made of I factors only, gives sum |psi_j|^2.
 *
 * Precision.  Products and sums are formed in double for Complex<f64> and for Complex<f32> states alike; f32 amplitudes are
 * widened before the first product.  (qip_hip.h's norm_sqr and measure_probs form |psi_j|^2 in the state's own precision: on a
 * Complex<f32> state they agree with this call to f32 rounding of the products only.)
 *
 * Determinism.  No atomics: every block writes its partial sums to the handle's reduction scratch (d_partial) and the host
 * adds them in block order, as norm_sqr does.  The same call on the same state returns the same bits.
 *
 * Reproducibility.  values[t] depends on the state and on term t only: not on which other terms are in the call, on their
 * order, or on option "expect_group".  A batch equals the single-term calls bit for bit.  (One grid geometry and one
 * accumulation order per n, precision and class of x mask — zero, bit 0 set, bit 0 clear — whatever the group.)
 *
 * Cost.  The terms are sorted by x mask (stably); the terms of one x mask share passes over the vector, at most
 * "expect_group" terms per pass: one kernel launch and one small copy per pass.  Strings of Z and I (x = 0) are a signed norm
 * pass.  An empty term is a term of x = 0 like any other and takes a slot of such a pass.
 *
 * The state is not changed.  The call is ordered after the work queued on the handle and complete when it returns.  A
 * relabelled state (option "tile_relabel" = 3) is put back in the caller's order on entry, as by the measurement calls.
 *
 * Arguments.  count == 0 returns QIP_OK (null arrays allowed).  With count > 0 each of these is QIP_ERR_INVALID, with a
 * message: a null array; term_start[0] != 0; a decreasing term_start; a qubit >= n; a qubit repeated inside one term; a code
 * > 3.  A null handle is QIP_ERR_INVALID: there is no host fall-back.
 *
 * State option "expect_group" (set_option of qip_hip.h): the most terms per pass, 1 to 32, anything else is refused with
 * QIP_ERR_INVALID.  Default 16: the largest kernel capacity (1, 4, 16, 32) whose pass stayed within 1.5x of the single-term
 * pass in the run recorded in profiles/expect_pauli.md (n = 30, both precisions). */
int qipx_state_expect_pauli(qip_hip_state* s, const uint64_t* term_start, const uint64_t* qubits,
                            const uint8_t* paulis, uint64_t count, double* values);

/* Host only, no device needed: the number of passes over the vector the call above makes for these terms on an n-qubit state
 * when at most `group` terms share a pass (group = 0: the default of "expect_group"; above 32: QIP_ERR_INVALID).  The terms
 * are checked as above; count == 0 gives 0 passes.  It runs the grouping code the call itself runs. */
int qipx_expect_pauli_passes(uint32_t n, const uint64_t* term_start, const uint64_t* qubits, const uint8_t* paulis,
                             uint64_t count, uint32_t group, uint64_t* passes);

/* Pauli-string rotations in place.  (Added without a change of QIPX_ABI_VERSION: purely additive again.)
 *
 * For t = 0 .. count-1, IN THE ORDER GIVEN, psi <- exp(-i * angles[t] * P_t) psi.  The terms are given exactly as for
 * qipx_state_expect_pauli above (the same arrays, the same codes, qubit q = index bit n-1-q) and are checked by the same code
 * with the same messages.  Nothing is reordered: the terms do not commute in general.
 *
 * The rotation.  exp(-i theta P) = cos theta * I - i sin theta * P, and with x, z, n_Y as above
 *   (P psi)[j] = i^n_Y * (-1)^popcount((j ^ x) & z) * psi[j ^ x],
 * so every amplitude mixes with one partner only: one in-place pass that reads and writes each amplitude once, whatever the
 * weight of the string.  An empty term, and a term of I factors only, is the global phase e^{-i theta}: a term of x = 0 like
 * any other (a Z string multiplies psi[j] by e^{-+ i theta}).
 *
 * Arithmetic.  c = cos theta and s = sin theta are evaluated in double on the host and rounded once to the state's precision.
 * The factor -i * i^n_Y * (+-1) is a swap or negation of components, which is exact.  Every new component is
 *   fl(fl(c * u) + fl(s * v))
 * in the state's precision, u the old component and v the signed component of the partner (of the amplitude itself when
 * x = 0); no fused multiply-add, and zero amplitudes get no special case.  Per component the error of one rotation is at most
 * 4u(|c||u| + |s||v|) with u the unit roundoff (2^-53, 2^-24): rounding of c and s, two products, one sum.
 *
 * Reproducibility.  A batch leaves the bits that the single-term calls leave when made one after the other, under any value
 * of option "rotate_group": a slot of a pass does the same operations on the same values whatever its company.
 *
 * Cost.  A pass takes a maximal run of CONSECUTIVE terms of equal x mask, cut at "rotate_group" terms: it loads each pair
 * (j, j ^ x) once, applies the run's rotations to it one after the other in registers, in term order, and stores it: one kernel
 * launch per pass, no synchronisation, no atomics.  The eight strings of a Jordan-Wigner double excitation share one x mask; a
 * whole QAOA cost layer is x = 0.  Terms of one x mask that are separated by a term of another do not share a pass.
 *
 * Calling contract.  The call is queued on the handle's stream behind earlier work and returns without waiting, like
 * qip_hip_state_apply_op.  A relabelled state (option "tile_relabel" = 3) is put back in the caller's order on entry.
 * count == 0 returns QIP_OK (null arrays allowed).  With count > 0 each of these is QIP_ERR_INVALID with a message, and leaves
 * the state untouched (everything is checked before the first launch): a null array; a non-finite angle (the message names the
 * term); any term error of qipx_state_expect_pauli.  A null handle is QIP_ERR_INVALID: there is no host fall-back.  More than
 * 2^32 - 1 terms is QIP_ERR_UNSUPPORTED.
 *
 * State option "rotate_group": the most terms per pass, 1 to 32, anything else is refused with QIP_ERR_INVALID.
 * Default 16: the largest of 1, 4, 16, 32 terms whose pass stayed within 1.5x of the single-term pass in the run recorded in
 * profiles/pauli_rotation.md (tools/bench_rotate.py, n = 30, both precisions: 16 terms 1.25x / 1.34x, 32 terms 2.27x / 2.47x; a
 * pass of more than a few terms is bound by vector issue, about 0.4 ms per term and pass in Complex<f64>, not by memory). */
int qipx_state_apply_pauli_rotations(qip_hip_state* s, const uint64_t* term_start, const uint64_t* qubits,
                                     const uint8_t* paulis, const double* angles, uint64_t count);

/* Host only, no device needed: the number of passes over the vector the call above makes for these terms on an n-qubit state
 * when at most `group` terms share a pass (group = 0: the default of "rotate_group"; above 32: QIP_ERR_INVALID).  The terms
 * are checked as above; count == 0 gives 0 passes.  It runs the grouping code the call itself runs. */
int qipx_pauli_rotation_passes(uint32_t n, const uint64_t* term_start, const uint64_t* qubits, const uint8_t* paulis,
                               uint64_t count, uint32_t group, uint64_t* passes);

/* A Pauli sum applied to a second state.  (Added without a change of QIPX_ABI_VERSION: purely additive again.)
 *
 * dst <- H src, or dst <- dst + H src when `accumulate` is non-zero, for H = sum_t c_t P_t with complex coefficients
 * c_t = coeffs[2t] + i coeffs[2t+1].  The terms are given exactly as for qipx_state_expect_pauli above (the same arrays, the same
 * codes, qubit q = index bit n-1-q) and are checked by the same code with the same messages.  With x, z, n_Y as there,
 *   dst[j] = (accumulate ? dst[j] : 0) + sum_t c_t * i^n_Y,t * (-1)^popcount((j ^ x_t) & z_t) * src[j ^ x_t].
 * H need not be Hermitian and nothing is normalised.  This is the step of the adjoint gradient (lambda = H psi), of Lanczos and
 * Krylov iterations, of an imaginary-time step and of <H^2>.
 *
 * Cost.  The terms are sorted by x mask (stably); the terms of one x mask share passes, at most "sum_group" terms per pass: one
 * kernel launch per pass, which reads `src` once and reads and writes `dst` once (the first pass of a call that does not
 * accumulate stores without reading `dst`).  No atomics.
 *
 * Arithmetic.  Everything is formed in the state's precision (u = 2^-53, 2^-24), without fused multiply-add.  k_t = c_t * i^n_Y,t
 * (a swap and sign flips, exact) is rounded once to that precision on the host.  Per amplitude a pass forms the signed
 * coefficient sum w = sum of (+-)k_t over its terms, in term order starting from +0, one addition per component and term; then the
 * complex product p = w * src[j ^ x] as re = fl(fl(wr sr) - fl(wi si)), im = fl(fl(wr si) + fl(wi sr)); then stores p (first pass
 * of a call that does not accumulate) or fl(dst[j] + p) per component.  To first order in u the error of an amplitude is within
 *   (m + 3) u * sum_t |c_t| |src[j ^ x_t]|  +  P u * (sum_t |c_t| |src[j ^ x_t]| + |dst_old[j]|)
 * for P passes of at most m terms each (m + P <= count + 1).  The result depends on the call only — same call, same bits — but
 * NOT only on the terms: another "sum_group", or another order of the terms, adds in another order and may differ by rounding.
 *
 * Calling contract.  Both handles are put in the caller's order on entry (option "tile_relabel" = 3), the work queued on `src` is
 * waited for, the passes run on `dst`'s stream, and THE CALL IS COMPLETE WHEN IT RETURNS, as qip_hip_state_copy_from is: the caller
 * may change `src` at once.  `src` is not changed.  count == 0 sets dst to zero, or leaves it as it is when accumulating (null
 * arrays allowed).  Each of these is refused with a message before anything is queued, `dst` untouched: a null handle
 * (QIP_ERR_INVALID, there is no host fall-back); a handle that is unusable after a failed relabelled batch (QIP_ERR_DEVICE);
 * dst == src (QIP_ERR_INVALID: later passes need the source intact); handles that differ in n or dtype (QIP_ERR_INVALID) or live
 * on different devices (QIP_ERR_UNSUPPORTED); with count > 0 a null array, a non-finite coefficient (the message names the term)
 * or any term error of qipx_state_expect_pauli (QIP_ERR_INVALID); more than 2^32 - 1 terms (QIP_ERR_UNSUPPORTED).
 *
 * State option "sum_group" (of `dst`): the most terms per pass, 1 to 32, anything else is refused with QIP_ERR_INVALID.
 * Default 16: the largest of 1, 4, 16, 32 terms whose pass stayed within 1.5x of the single-term pass in the run recorded in
 * profiles/adjoint_gradient.md (tools/bench_adjoint.py, n = 30, both precisions: 16 terms 1.11x / 1.08x, 32 terms 1.43x / 1.65x;
 * a storing pass of up to 16 terms costs what a rotation pass costs, an accumulating one 1.5x: three vectors against two). */
int qipx_state_apply_pauli_sum(qip_hip_state* dst, qip_hip_state* src, const uint64_t* term_start, const uint64_t* qubits,
                               const uint8_t* paulis, const double* coeffs, uint64_t count, int accumulate);

/* Host only, no device needed: the number of passes the call above makes for these terms on an n-qubit state when at most
 * `group` terms share a pass (group = 0: the default of "sum_group"; above 32: QIP_ERR_INVALID).  The terms are checked as
 * above; count == 0 gives 0 passes.  It runs the grouping code the call itself runs. */
int qipx_pauli_sum_passes(uint32_t n, const uint64_t* term_start, const uint64_t* qubits, const uint8_t* paulis,
                          uint64_t count, uint32_t group, uint64_t* passes);

/* Pauli matrix elements between two states.  (Purely additive again.)
 *
 * values[2t] + i values[2t+1] = <bra| P_t |ket>
 *                             = sum_j conj(bra[j]) * i^n_Y * (-1)^popcount((j ^ x) & z) * ket[j ^ x],     t < count,
 * the terms as for qipx_state_expect_pauli.  The value is raw: it is not divided by any norm.  An empty term (and a term of I
 * factors only) gives the inner product <bra|ket>.  bra == ket is allowed: the Hermitian case, whose real part is the value of
 * qipx_state_expect_pauli up to rounding (that call and its bits are untouched by this one: it has its own kernel).
 *
 * Precision.  Products and sums are formed in double for both precisions; f32 amplitudes are widened before the first product.
 * Determinism and reproducibility are those of qipx_state_expect_pauli: per-block partial sums in `ket`'s reduction scratch,
 * added on the host in block order, no atomics; values[2t], values[2t+1] depend on the two states and on term t only, so a batch
 * equals its single-term calls bit for bit under any "expect_group".
 *
 * Cost.  The terms are sorted by x mask (stably) and the terms of one x mask share passes over both vectors, at most
 * min("expect_group" of `ket`, 16) terms per pass (the kernel keeps two running sums per term).
 *
 * Neither state is changed.  Both handles are put in the caller's order on entry; the call is ordered after the work queued on
 * both handles and complete when it returns.  count == 0 returns QIP_OK (null arrays allowed).  The handles are checked as by the
 * call above (bra == ket excepted); with count > 0 a null array or any term error of qipx_state_expect_pauli is QIP_ERR_INVALID. */
int qipx_state_pauli_matrix_elements(qip_hip_state* bra, qip_hip_state* ket, const uint64_t* term_start, const uint64_t* qubits,
                                     const uint8_t* paulis, uint64_t count, double* values);

/* The reduced density matrix of up to six qubits.  (Purely additive again.)
 *
 * With the amplitudes seen as a 2^k x 2^(n-k) matrix Psi (row a = the bits of the k qubits, column b = all other bits),
 *   rho[a][a'] = sum_b psi[a,b] * conj(psi[a',b]),       rho = Psi Psi^H = Tr_rest |psi><psi|.
 * `rho` holds 2 * 4^k doubles, row-major with M = 2^k: rho[2 (a M + a')] and rho[2 (a M + a') + 1] are the real and imaginary part
 * of rho[a][a'].  Bit i of a and of a' is the bit of qubit indices[i], the outcome convention of qip_hip_state_measure_probs; qubit
 * q is index bit n-1-q.  The value is raw: it is NOT divided by the norm, so tr rho = sum |psi_j|^2 and the diagonal is what
 * measure_probs returns (to the rounding of the products on a Complex<f32> state, see below).
 *
 * Supported: 1 <= k <= 6, k = n included (one column: rho = psi psi^H).  k > 6 is QIP_ERR_UNSUPPORTED with a message that names
 * k.  The index list is checked as by the measurement calls, with their messages (k = 0, an index >= n, a repeated index:
 * QIP_ERR_INVALID).  A null `rho` and a null handle are QIP_ERR_INVALID: there is no host fall-back.  Everything is checked
 * before the first launch.
 *
 * Precision.  Products and sums are formed in double for Complex<f64> and Complex<f32> states alike; f32 amplitudes are widened
 * before the first product, as in qipx_state_expect_pauli.
 *
 * Arithmetic.  Re rho[a][a'] = sum_b (xr xr' + xi xi'), Im rho[a][a'] = sum_b (xi xr' - xr xi') with psi[a,b] = xr + i xi and
 * psi[a',b] = xr' + i xi'.  k <= 3: fused multiply-adds into one running sum per entry and lane.  k = 4 .. 6: the f64 matrix
 * instruction v_mfma_f64_16x16x4_f64 on 16 x 16 blocks I <= J of rho, four columns b per step; on a diagonal block the imaginary
 * part is T - T^T for the accumulated T = Xi Xr^T.
 *
 * Exact structure.  The library computes the entries a <= a' (in the sorted order below) once and mirrors them: rho[a'][a] is bit
 * for bit the conjugate of rho[a][a'], and every diagonal imaginary part is +0.0.
 *
 * Determinism.  No atomics.  Every block writes one partial matrix to the handle's reduction scratch; a second kernel adds the
 * partial matrices entry by entry in block order on the device, so that only 4^k entries cross PCIe.  The same call on the same
 * state returns the same bits.  The kernels work on the qubits' index positions in ascending order and the host permutes rows
 * and columns: the result for a permuted index list is the bit-exact row/column permutation of the result for the sorted list.
 *
 * Scratch.  k <= 3: at most 4096 blocks of 4^k doubles (2 MiB).  k = 4 .. 6: at most 1024 blocks of 512 / 1536 / 5120 doubles (the
 * blocks I <= J only): 4 / 12 / 40 MiB, plus one matrix for the fold.  It is the handle's reduction scratch, grown on demand and
 * freed with the handle.
 *
 * Error statement.  Let S = sum_b |psi[a,b]| |psi[a',b]| <= sqrt(rho[a][a] rho[a'][a']) (Cauchy-Schwarz) and u = 2^-53.  To first
 * order an entry is within c u * 2 S of the exact sum over the stored amplitudes (each part of an entry adds two products per
 * column), c the longest chain of additions a product passes through:
 *   k <= 3    lane chain: 2^(n-k-20) groups for n - k >= 20 (4096 blocks of 256 lanes; at most 512 at n = 30), two fused
 *             multiply-adds each; wave tree 6; the block's four waves 3; block fold 4096 / 64 = 64 in a lane, then a tree of 6;
 *             c <= 2 * 512 + 6 + 3 + 64 + 6 = 1103 at n = 30, k = 1.
 *   k >= 4    a wave's accumulators are added to a second set and cleared every 32 steps of four columns: inner chain 32 * 4 = 128
 *             columns; outer chain: a wave meets 2^(n-k) / 4096 columns (1024 blocks, 4 waves to a set of block pairs; 2 at k = 6),
 *             2^14 at n = 30, k = 4, that is 128 additions; the block's waves 3; block fold 1024 / 64 = 16, then a tree of 6;
 *             T - T^T one more; c <= 2 * 128 + 128 + 3 + 16 + 6 + 1 = 410 at n = 30, k = 4.
 * Both stay below 1e-12 S / (2 S u) = 4500: the result is within 1e-12 * sqrt(rho[a][a] rho[a'][a']) of the exact value for every
 * n <= 30 (tests/test_gpu_f2_reduced_density.py holds every entry to that bar).
 *
 * Calling contract.  The state is not changed.  A relabelled state (option "tile_relabel" = 3) is put back in the caller's order on
 * entry, as by the measurement calls.  The call is ordered after the work queued on the handle and complete when it returns. */
int qipx_state_reduced_density(qip_hip_state* s, const uint64_t* indices, uint32_t k, double* rho);

/* The two-state counterpart of the call above: the reduced TRANSITION matrix of up to three qubits.  (Purely additive again.)
 *
 *   M[a][a'] = sum_b ket[a,b] * conj(bra[a',b]) = Tr_rest |ket><bra|,
 * rows a and a' the bits of the k qubits, column b all other bits.  <bra| A |ket> = Tr(A M) for EVERY operator A on those qubits,
 * from one read of the two vectors: what the adjoint method needs for A = dW/dtheta W^H of a parametrised gate W.
 * `m` holds 2 * 4^k doubles, row-major with M = 2^k: m[2 (a M + a')] and m[2 (a M + a') + 1] are the real and imaginary part of
 * M[a][a'].  Bit i of a and of a' is the bit of qubit indices[i], the convention of qipx_state_reduced_density; qubit q is index
 * bit n-1-q.  The value is raw, divided by no norm: tr M = <bra|ket>.  bra == ket is allowed: M is then the reduced density matrix
 * (up to rounding: no promise is made that the result mirrors bit for bit, nor that it has qipx_state_reduced_density's bits).
 *
 * Supported: 1 <= k <= 3, k = n included.  k > 3 is QIP_ERR_UNSUPPORTED with a message that names k.  k = 0, an index >= n, a
 * repeated index, a null index array, a null `m` and a null handle are QIP_ERR_INVALID: there is no host fall-back.  Handles that
 * differ in n or dtype are QIP_ERR_INVALID, handles on different devices QIP_ERR_UNSUPPORTED, an unusable handle QIP_ERR_DEVICE,
 * as by qipx_state_pauli_matrix_elements.  Everything is checked before the first launch: on a refusal neither state nor `m` is
 * touched.
 *
 * Precision and arithmetic.  Products and sums are formed in double for both precisions; f32 amplitudes are widened first.  With
 * ket[a,b] = xr + i xi and bra[a',b] = yr + i yi a column adds xr yr + xi yi to Re and xi yr - xr yi to Im, each as two fused
 * multiply-adds into one running sum per part, entry and lane.  There is no Hermitian symmetry: all 4^k entries are formed.
 *
 * Kernel.  ONE launch of a kernel of its own (k_transition_small, csrc/qip_kernels.h) plus the fold: the gather skeleton of the
 * k <= 3 density kernel on two base pointers, each vector read once with non-temporal 16-byte loads, no atomics.  k = 3: 64
 * complex sums do not fit a lane's registers next to 2 x 8 amplitudes, and the form chosen is THE ENTRIES SPLIT OVER LANES: two
 * lanes that differ in a lane-id bit that is no position pair up, each keeps the four rows a of one half (all eight a') and forms
 * them for its own column and for its partner's, whose amplitudes come by 12 wave shuffles of 16 bytes.  No matrix instruction.
 *
 * Exact promises.  The same call on the same states returns the same bits (one partial matrix per block in `ket`'s reduction
 * scratch, folded entry by entry in block order on the device: only 4^k entries cross PCIe).  The kernel works on the qubits'
 * index positions in ascending order and the host permutes: the result for a permuted index list is the bit-exact row and column
 * permutation of the result for the sorted list.  An entry all of whose products are zero is exactly zero.  Neither state is
 * changed.
 *
 * Scratch.  At most 4096 blocks of 2 * 4^k doubles (4 MiB at k = 3) plus one matrix, in `ket`'s reduction scratch.
 *
 * Error statement.  With S = sum_b |ket[a,b]| |bra[a',b]| <= sqrt(rho_ket[a][a] rho_bra[a'][a']) (Cauchy-Schwarz over two
 * different rows; rho_x[a][a] = sum_b |x[a,b]|^2) and u = 2^-53, each part of an entry is to first order within c u * 2 S of the
 * exact sum over the stored amplitudes, c the longest chain of additions a product passes through.  As built: a lane's chain is
 * its 2^(n-k-20) columns for n - k >= 20 (4096 blocks of 256 lanes), two fused multiply-adds each — at k = 3 the lane meets its
 * partner's columns too, 2 * 2^(n-23) columns — at most 512 columns at n = 30 for every k; the wave's butterfly 6 (5 at k = 3);
 * the block's four waves 3; the block fold 4096 / 64 = 64 in a lane, then a tree of 6:
 *   c <= 2 * 512 + 6 + 3 + 64 + 6 = 1103 at n = 30,
 * the count of the density call, below 1e-12 / (2 u) = 4500: every entry is within 1e-12 * sqrt(rho_ket[a][a] rho_bra[a'][a'])
 * of the exact value for every n <= 30 (tests/test_gpu_f2_transition.py holds every entry to that bar).
 *
 * Calling contract, as qipx_state_pauli_matrix_elements': both handles are put in the caller's order on entry (option
 * "tile_relabel" = 3), the call is ordered after the work queued on both handles, runs on `ket`'s stream and is complete when it
 * returns. */
int qipx_state_transition_matrix(qip_hip_state* bra, qip_hip_state* ket, const uint64_t* indices, uint32_t k, double* m);

/* Vector arithmetic of resident states: what Lanczos and Krylov iterations need besides qipx_state_apply_pauli_sum.  (Purely
 * additive again.)
 *
 * dst[j] <- sum_{i < count} c_i * srcs[i][j],   c_i = coeffs[2i] + i coeffs[2i+1],   for every amplitude j.
 *
 * Shape.  1 <= count <= 16; more is QIP_ERR_UNSUPPORTED.  count == 0 sets dst to zero and *norm_sqr to 0 (null arrays allowed).
 * `dst` may be any of the sources and a handle may appear more than once: the operation is elementwise, every source is read at
 * j before j is stored.  So scaling in place is count = 1 with srcs[0] == dst, and the Lanczos update w <- w - a v - b v' is one
 * call of three sources.
 *
 * Cost.  ONE kernel launch: every listed source is read once (16-byte accesses: one Complex<f64>, two Complex<f32>) and dst is
 * written once, whatever is aliased: count + 1 vectors of traffic.  No atomics.
 *
 * Arithmetic.  Everything is formed in the state's precision (u = 2^-53, 2^-24), without fused multiply-add.  c_i is rounded once
 * to that precision on the host, (cr, ci).  Per amplitude, with src_i[j] = (sr, si),
 *   p_i = ( fl(fl(cr sr) - fl(ci si)),  fl(fl(cr si) + fl(ci sr)) ),
 *   acc = p_0,  then  acc = fl(acc + p_i)  per component for i = 1 .. count-1 in source order,
 * and acc is stored.  Zero, real and imaginary coefficients get no special case (a coefficient 0 still multiplies: a NaN or an
 * infinity in that source spreads, and -0 can appear).  The result depends on the call only: same call, same bits.
 *
 * Norm.  With a non-null `norm_sqr` the same pass also returns sum_j |dst[j]|^2 of the STORED (rounded) amplitudes, formed in
 * double for both precisions: each component is widened, fl(fl(x x) + fl(y y)) is added to the lane's running sum, then wave,
 * block, and one partial per block in dst's reduction scratch, which the host adds in block order, as norm_sqr does.  The grid
 * depends on n and the precision only: the same call returns the same bits, and the value is within 1e-12 times the exact sum
 * (non-negative terms along chains of at most c = 2^(n-20) + 6 + 4 + 4096 additions — lane, wave tree, the block's waves, the
 * host's blocks — which is 5130 at n = 30: (c + 2) 2^-53 = 5.7e-13).
 * (qip_hip.h's norm_sqr forms |psi_j|^2 in the state's precision: on a Complex<f32> state the two agree to f32 rounding only.)
 *
 * Calling contract, as qipx_state_apply_pauli_sum's.  Every handle is put in the caller's order on entry (option "tile_relabel"
 * = 3), the work queued on every source is waited for, the pass runs on dst's stream and THE CALL IS COMPLETE WHEN IT RETURNS.  No
 * source other than dst is changed.  Each of these is refused with a message before anything is queued, dst untouched: a null
 * handle, dst or a source (QIP_ERR_INVALID: there is no host fall-back); an unusable handle (QIP_ERR_DEVICE); a source that
 * differs from dst in n or dtype (QIP_ERR_INVALID) or lives on another device (QIP_ERR_UNSUPPORTED); with count > 0 a null array
 * or a non-finite coefficient (QIP_ERR_INVALID; the message names the source); count > 16 (QIP_ERR_UNSUPPORTED).
 *
 * There is no option: the kernel is compiled for 1, 2, 3, 4, 8 and 16 sources and a call takes the smallest that holds it. */
int qipx_state_linear_combination(qip_hip_state* dst, qip_hip_state* const* srcs, const double* coeffs, uint32_t count,
                                  double* norm_sqr /* may be null */);

/* Inner products of up to 16 states with one state.  (Purely additive again.)
 *
 * values[2i] + i values[2i+1] = <bras[i]|ket> = sum_j conj(bras[i][j]) * ket[j],   i < count.
 *
 * Shape.  1 <= count <= 16; more is QIP_ERR_UNSUPPORTED, count == 0 returns QIP_OK (null arrays allowed).  ONE pass reads `ket`
 * once and each bra once (16-byte accesses): orthogonalising against a basis of m vectors moves m + 1 vectors, not 2m.
 * bras[i] == ket is allowed, and then values[2i+1] is exactly +0: the two products of the imaginary part are the same numbers.
 *
 * Precision.  Products and sums are formed in double for both precisions; f32 amplitudes are widened before the first product.
 * With bra[j] = (pr, pi) and ket[j] = (ar, ai) an amplitude adds fl(fl(pr ar) + fl(pi ai)) and fl(fl(pr ai) - fl(pi ar)) to the
 * lane's two running sums; then wave, block, one partial per block in ket's reduction scratch, added on the host in block
 * order.  No atomics.  Each part is within (c + 2) 2^-53 sum_j |bra[j]| |ket[j]| <= 5.7e-13 |bra| |ket| of the exact sum for
 * n <= 30 (c as above; Cauchy-Schwarz).
 *
 * Reproducibility.  values[2i], values[2i+1] depend on bras[i] and ket only: there is one grid and one accumulation order per n
 * and precision whatever `count` is, so a batch equals its single-bra calls bit for bit.  The bits are NOT those of
 * qipx_state_pauli_matrix_elements with the empty term: that call keeps its kernel and its order.
 *
 * Neither state is changed.  The handles are met as above (ket in the place of dst), the call is ordered after the work queued
 * on all of them and complete when it returns.  With count > 0 a null `bras` or `values` is QIP_ERR_INVALID. */
int qipx_state_inner_products(qip_hip_state* const* bras, uint32_t count, qip_hip_state* ket, double* values);

/* Diagonal Pauli sums of any size in one pass: the cost layer exp(-i gamma D) of QAOA and the first two moments of a cost
 * Hamiltonian D = sum_t coeffs[t] * Z-string_t (MaxCut / SK / Ising energies, penalty terms, any objective on bit strings expanded
 * in Z monomials).  (Purely additive again.)
 *
 * The terms are given exactly as for qipx_state_expect_pauli above (the same arrays, the same codes, qubit q = index bit n-1-q)
 * and are checked by the same code with the same messages; every factor must be I or Z, coeffs[t] is real.  With z_t the z mask
 * of term t,
 *   D(j) = sum_t coeffs[t] * (-1)^popcount(j & z_t).
 *   apply:   psi[j] <- exp(-i * gamma * D(j)) * psi[j]
 *   expect:  moments[0] = sum_j |psi_j|^2 D(j),   moments[1] = sum_j |psi_j|^2 D(j)^2     (raw: not divided by the norm)
 * An empty term (and a term of I factors only) is the constant coeffs[t]: a global phase, an offset.  Repeated z masks are allowed
 * and add.
 *
 * Cost.  ONE kernel launch whatever `count` is; every amplitude is read once (and, by apply, written once, in place).  The
 * vector is cut into tiles of 2^L contiguous amplitudes, L = min(n, 12), j = (h << L) | l.  With z_t = (zhi_t << L) | zlo_t the 2^L
 * energies of tile h are the Walsh-Hadamard transform of a_h[m] = sum_{t : zlo_t = m} k_t (-1)^popcount(h & zhi_t): a tile costs
 * `count` sign evaluations, spread over the block's lanes by low mask, and L additions per amplitude, instead of `count` per
 * amplitude.  (The terms of ONE low mask are summed by one lane: a call whose terms all share a low mask, all of them above bit
 * 12 for instance, serialises there.)  The term table lives in a device buffer of the handle, grown on demand and freed with it.
 * tools/bench_diagonal.py and profiles/diagonal.md hold the measured times against the rotation and expect_pauli paths.
 *
 * Arithmetic.  k_t = fl(gamma * coeffs[t]) in double on the host (apply), k_t = coeffs[t] (expect).  The energy E^(j) is formed IN
 * DOUBLE for both precisions: a_h[m] is the sum of (+-)k_t over the terms of low mask m in the order of the call, starting from
 * +0 (the sign an exact flip); then L butterfly stages (u, v) -> (u + v, u - v) over index bit 0, 1, .., L - 1 in that order, v
 * the entry whose stage bit is set.  E^(j) is a function of the call and of j only, not of the grid or of the element packing
 * (option "packed_f32"): same call, same bits.  No atomics anywhere.
 *   apply    (c, s) = (cos E^, sin E^) evaluated in double and rounded once to the state's precision; the new components are
 *            fl(fl(c re) + fl(s im)) and fl(fl(c im) - fl(s re)), never fused, no special case for zeros, as in the rotation kernel.
 *   expect   p = fl(fl(re re) + fl(im im)) in double (f32 amplitudes widened first, as in qipx_state_expect_pauli); the lane adds
 *            fl(p E^) and fl(fl(p E^) E^) to its two running sums; then wave, block, and two partial sums per block in the
 *            handle's reduction scratch, which the host adds in block order.  The longest chain of additions is
 *              c(n) = 16 * max(1, 2^(n-24)) + 6 + 4 + min(4096, 2^(n-12))      (n >= 12; max(1, 2^(n-8)) + 11 below)
 *            (a lane's 16 amplitudes of each of its block's tiles, the wave's tree, the block's waves, the host's blocks):
 *            5130 at n = 30.
 *
 * Error statement.  With A = sum_t |k_t| and u the unit roundoff of the state (2^-53, 2^-24), to first order
 *   |E^(j) - gamma D(j)| <= (count + L + 1) 2^-53 A          (one rounding of k_t, at most count + L additions)
 *   apply:   |psi'[j] - exp(-i gamma D(j)) psi[j]| <= [12 u + (count + L + 8) 2^-53 A] |psi[j]|
 *   expect:  |moments[0] - exact| <= (count + L + c(n) + 6) 2^-53 A |psi|^2,
 *            |moments[1] - exact| <= (2 (count + L) + c(n) + 10) 2^-53 A^2 |psi|^2.
 * 12 u is the bar of one unit-modulus complex multiply with rounded c and s (the rotation call's, a double-precision reference
 * included); the 8, 6 and 10 hold the few ulps of the double sine and cosine, the roundings of p and of the products, and margin.
 * These are the constants tests/diagonal_ref.py derives and the GPU tests hold both calls to.
 * Large angles are carried by the A term alone: the sine and cosine are double-precision evaluations of a double-precision
 * angle for Complex<f32> states too.
 *
 * Calling contract.  apply: the state is changed in place; the launch is queued on the handle's stream and the call returns
 * without waiting, like qipx_state_apply_pauli_rotations (a relabelled state, option "tile_relabel" = 3, is put back in the
 * caller's order first).  The caller's arrays are not read after the call returns: the table travels through a pinned buffer of
 * the handle; there are two, taken in turn, and a call waits only for the upload of the call before the previous one — never for a
 * kernel — before it rewrites its buffer.
 * expect: the state is not changed (relabelled: settled first, as by the measurement calls); the call is ordered after the work
 * queued on the handle and COMPLETE WHEN IT RETURNS.  count == 0: apply does nothing, expect returns (0, 0) (null arrays allowed).
 * Each of these is refused with a message before anything is queued, the state untouched: a null handle (QIP_ERR_INVALID: there
 * is no host fall-back); an unusable handle (QIP_ERR_DEVICE); with count > 0 a null array or a null `moments`, a non-finite
 * coefficient, a non-finite gamma or a non-finite product of the two (the message names the term), a term with an X or Y factor
 * ("term %llu is not diagonal") or any term error of qipx_state_expect_pauli (all QIP_ERR_INVALID); more than 2^20 terms
 * (QIP_ERR_UNSUPPORTED: the cap of one call).
 *
 * There is no option, and the launches are not a kernel class of the profile. */
int qipx_state_apply_diagonal(qip_hip_state* s, const uint64_t* term_start, const uint64_t* qubits, const uint8_t* paulis,
                              const double* coeffs, uint64_t count, double gamma);
int qipx_state_expect_diagonal(qip_hip_state* s, const uint64_t* term_start, const uint64_t* qubits, const uint8_t* paulis,
                               const double* coeffs, uint64_t count, double* moments /* [2] */);

/* Classical functions between qubit registers in one pass: |x>|y> -> e^{i phi(x)} |x>|y (+) f(x)>, the oracles of Grover and
 * amplitude amplification, the arithmetic of Shor-type circuits with a classical base and modulus, comparators, table look-ups
 * and QROM loads, without Toffoli networks and without ancilla qubits.  (Purely additive again.)
 *
 * Registers.  in_qubits[0..m) and out_qubits[0..k) are disjoint lists of distinct qubits (qubit q = index bit n-1-q); bit i of the
 * register value x / y is the bit of qubit in_qubits[i] / out_qubits[i] (LSB first, as in measure_probs and
 * qipx_state_reduced_density).  For every basis index j with in-register value x and out-register value y, every other bit
 * untouched,
 *   new[j with y replaced by y'] = w(x) * old[j],
 *   QIPX_FN_XOR:  y' = y ^ values[x]            QIPX_FN_ADD:  y' = (y + values[x]) mod 2^k.
 * `values` and `phases` hold 2^m entries.  m = 0 is a constant (an X mask, an increment by a constant).  k = 0 requires
 * values == NULL and a non-NULL `phases`: a phase by table on a register (a Grover oracle for any marked set, any diagonal
 * function of up to 2^m distinct values).  A control needs no parameter of its own: it is an in-register bit with values[x] = 0
 * where it reads 0.  m <= 24, k <= 32, m + k <= n.
 *
 * Arithmetic.  phases == NULL: w = 1, amplitudes are moved, not multiplied; the result carries the input's bits exactly, signed
 * zeros and non-finite values included.  Otherwise w(x) = (cos phases[x], sin phases[x]), evaluated by the host's libm in double and
 * rounded once to the state's precision; it is applied as ONE complex product in the state's precision (re = wr ar - wi ai,
 * im = wr ai + wi ar; a compiler may contract a product into the sum).  An entry that rounds to exactly (1, 0) is not multiplied:
 * that amplitude is moved with its bits.  Against the exact product the error of an amplitude is at most 8 u |psi_j|, u = 2^-53 or
 * 2^-24 (2 u for the rounded table entry, sqrt(5) u for the product, the rest for libm).
 *
 * Cost.  An amplitude only moves among the 2^k indices that share its x and its other bits, so a tile made of a wave row (index
 * bits 0..5) and the out register's positions outside it is closed under the map.  A block stages such tiles in LDS, 2^(6+h)
 * amplitudes for h out positions outside the row, loaded and stored in place as whole rows: every amplitude is read once and
 * written once per pass, no atomics, no second buffer.  A pass holds at most 6 out positions outside the six low index bits
 * (64 KiB of Complex<f64> per block).  QIPX_FN_XOR over more splits into ceil(h / 6) passes over disjoint subsets of the out bits,
 * each a complete XOR on its subset.  QIPX_FN_ADD does not split (carries cross): an out register with MORE THAN 6 positions
 * outside the six low index bits is refused in that mode.  Out bits inside the row cost nothing.  The table is one 32-bit word
 * per entry and pass plus, with phases, one amplitude per entry; it lives in a device buffer of the handle (the one of
 * qipx_state_apply_diagonal), grown on demand and freed with it.  tools/bench_function.py measures the passes against a gate pass
 * and against the same maps as SparseMatrix ops and Toffoli networks.
 *
 * Calling contract.  The state is changed in place; the launches are queued on the handle's stream and the call returns without
 * waiting (a relabelled state, option "tile_relabel" = 3, is put back in the caller's order first; an unusable one is refused with
 * QIP_ERR_DEVICE).  The caller's arrays may be freed or rewritten as soon as the call returns: the table travels through a pinned
 * buffer of the handle and its upload is stream-ordered, exactly as for qipx_state_apply_diagonal.
 * Each of these is QIP_ERR_INVALID with a message, before anything is queued, the state untouched: a null handle (there is no host
 * fall-back); a qubit >= n ("out of range"), listed twice ("repeated") or in both registers; an unknown mode; m > 24 or k > 32; a
 * null qubit array of a non-empty register; k > 0 with values == NULL ("null value array"); k = 0 with values or without phases;
 * values[x] >= 2^k ("does not fit"); a non-finite phase; QIPX_FN_ADD beyond the limit above.
 *
 * qipx_function_passes is host-only, like qipx_pauli_rotation_passes: the number of passes over the vector that the call above
 * makes on n qubits, after the same checks of the registers and the mode with the same messages.  It needs no device.
 *
 * Out of scope: general in-place bijections of a register that do not preserve x (addition or multiplication modulo a QUANTUM
 * register's value, the reference's add_mod / times_mod); recording the call into programs / hipGraph, the sharded state, the
 * builder, replay and QASM; the C++ mirror.  There is no option, and the launches are not a kernel class of the profile. */
#define QIPX_FN_XOR 0
#define QIPX_FN_ADD 1
int qipx_state_apply_function(qip_hip_state* s, const uint64_t* in_qubits, uint32_t m, const uint64_t* out_qubits, uint32_t k, int mode,
                              const uint64_t* values, const double* phases);
int qipx_function_passes(uint32_t n, const uint64_t* in_qubits, uint32_t m, const uint64_t* out_qubits, uint32_t k, int mode,
                         uint32_t* passes);

/* Multiplexed (uniformly controlled) 1- and 2-qubit gates from a table in one in-place pass: for every value x of a select register
 * the matrix U_x on one or two target qubits,
 *   |x>|t>  ->  |x> (U_x |t>)        for all 2^m values x in one call,
 * the non-diagonal counterpart of the table calls above: Moettoenen state preparation and isometries, QROM-controlled rotations,
 * the SELECT of a block encoding on small targets, a batch of parameter sets held in one state.  (Purely additive again.)
 *
 * Registers.  select[0..m) and targets[0..k) are disjoint lists of distinct qubits (qubit q = index bit n-1-q); bit i of x is the bit
 * of qubit select[i]; bit i of a matrix row or column is the bit of qubit targets[i] (the convention of qipx_state_apply_reduce).
 * `matrices` holds 2^m matrices of 2 * 4^k doubles each, row-major, re and im interleaved; entry x is U_x, any complex matrix,
 * unitary or not.  k is 1 or 2, m + 2k <= 20 (a table of at most 16 MiB in Complex<f64>), m + k <= n; m = 0 is a plain gate.
 *
 * Arithmetic.  Every table entry is rounded once to the state's precision.  With M = 2^k, for each group v of the M amplitudes that
 * share x and every other bit, in the state's precision and with no fused multiply-add,
 *   p_a' = ( fl(fl(wr xr) - fl(wi xi)), fl(fl(wr xi) + fl(wi xr)) )      w = U_x[a][a'], x = v[a']
 *   y_a  = p_0, then y_a = fl(y_a + p_a') for a' = 1 .. M-1 in ascending order
 * (zero entries are multiplied like any other).  If row a of the rounded matrix is exactly the unit row e_a (1 at a, zeros of
 * either sign elsewhere), y_a is v_a with its bits, signed zeros and non-finite values included: a controlled multiplexed gate is
 * a table whose matrices are the identity wherever the control bit of x reads 0, and those amplitudes stay untouched, as under
 * apply_op.  To first order |y_a - exact| <= sqrt(2) (M + 2) u |U_x[a]|_2 |v|_2, u = 2^-53 or 2^-24: a term passes one product
 * rounding (sqrt(2) u relative, both parts) and at most M further roundings of the sum, Cauchy-Schwarz bounds the sum of the term
 * magnitudes by |U_x[a]|_2 |v|_2, and one more u covers the rounded table.  The tests hold the arithmetic to (1.5 M + 3) u of
 * that norm product (6 u for k = 1, 9 u for k = 2) and the kernel bit for bit to the arithmetic.
 *
 * Cost.  One launch, one pass: every amplitude is loaded once and stored once to the address it came from, as whole wave rows, no
 * LDS staging, no atomics, no second buffer.  A lane holds the amplitudes of its group whose target bits lie outside the six low
 * index bits and gets the others from its wave by shuffles; it keeps only the matrix rows it stores, and fetches them again only
 * when a select bit of its index changes along its walk, which is ordered so that the other bits vary first.  The table lives in
 * the device buffer of the handle that qipx_state_apply_diagonal and qipx_state_apply_function use.  Measured at n = 30
 * (tools/bench_multiplex.py, profiles/multiplex.md), Complex<f64> / Complex<f32>: 5.8 - 6.4 / 2.9 - 3.1 ms for m <= 10 with a target
 * among the six low index bits, wherever the select bits sit (1.07 - 1.21 / 1.06 - 1.12 dense gate passes on the same targets), 6.9 -
 * 7.4 / 3.7 - 3.9 ms with two targets outside them; m = 16 pays for rounding and uploading its table on top (k = 2: 8.7 - 8.9 / 5.0 -
 * 5.1 ms; at n = 26 the table is most of the call).  2^m controlled gates through apply_ops cost 2.2 - 3.2 / 4.2 - 6.4 times the call at
 * m = 4, and one block-diagonal dense op on 6 qubits 1.30 / 1.58 times.  The call LOSES at the small end: to 4 controlled gates at
 * m = 2, k = 1 in Complex<f64> (5.6 - 5.7 against 6.2 - 6.3 ms), and to one block-diagonal dense op on m + k = 3 .. 5 qubits in
 * Complex<f64> (5.3 - 6.1 against 6.0 - 6.3 ms) and on 3 .. 4 qubits in Complex<f32> (2.7 - 2.9 against 2.9 - 3.1 ms): the pass runs
 * at about 85 % of a gate pass's bandwidth, which is open.
 *
 * Calling contract.  That of qipx_state_apply_function: the state is changed in place, the launch is queued on the handle's stream
 * and the call returns without waiting (a relabelled state is put back in the caller's order first; an unusable one is refused
 * with QIP_ERR_DEVICE); `matrices` may be freed or rewritten as soon as the call returns.  Each of these is QIP_ERR_INVALID with a
 * message, before anything is queued, the state untouched: a null handle (there is no host fall-back); a qubit >= n ("out of
 * range"), listed twice ("repeated") or in both registers; k = 0 or k > 2; m + 2k > 20; a null qubit array of a non-empty
 * register; a null `matrices` ("null matrix array"); an entry that is not finite.
 *
 * qipx_multiplexed_table_bytes is host-only: the bytes of the device table for a state of `dtype` (QIP_C64 / QIP_C32) on n qubits,
 * after the same checks of the registers with the same messages.  It needs no device.
 *
 * Out of scope: three or more target qubits, multiplexed Pauli strings, recording the call into programs / hipGraph, apply_ops
 * fusion, the sharded state, the builder, replay and QASM, the C++ mirror.  There is no option, and the launch is not a kernel
 * class of the profile. */
int qipx_state_apply_multiplexed(qip_hip_state* s, const uint64_t* select, uint32_t m, const uint64_t* targets, uint32_t k,
                                 const double* matrices);
int qipx_multiplexed_table_bytes(int dtype, uint32_t n, const uint64_t* select, uint32_t m, const uint64_t* targets, uint32_t k,
                                 uint64_t* bytes);

/* The quantum Fourier transform of a qubit register in FFT passes: the piece that closes period finding and phase estimation
 * after qipx_state_apply_function and qipx_state_apply_multiplexed.  (Purely additive again.)
 *
 * Register.  qubits[0..m) are distinct qubits (qubit q = index bit n-1-q); bit i of the register value is the bit of qubits[i]
 * (LSB first, as in qipx_state_apply_function, measure_probs and qipx_state_reduced_density), anywhere and in any order, 0 <= m <= n.
 *
 * Definition.  For every fibre (the M = 2^m amplitudes that share all other index bits):
 *   flags = 0                                 new[y] = M^(-1/2) sum_x exp(+2 pi i x y / M) old[x]
 *   QIPX_QFT_INVERSE                          the same with exp(-2 pi i x y / M)
 *   QIPX_QFT_REVERSED                         forward, the result left with the register's bits in reversed order: the amplitude
 *                                             of output value y sits where the register reads rev_m(y)
 *   QIPX_QFT_REVERSED | QIPX_QFT_INVERSE      the input is read in that reversed order and the output is natural: the call
 *                                             after a QIPX_QFT_REVERSED call is the identity
 * m = 0 does nothing.  Sign and order are the reference's qfft: with qubits = [n-1, .., 0] and flags = 0 the call equals the
 * lowered circuit of m Hadamards, m(m-1)/2 controlled phases and m/2 swaps on the whole register with qubit 0 the most
 * significant bit.
 *
 * Arithmetic.  Not bit-exact to anything: per fibre, with u = 2^-53 or 2^-24 by the state's precision,
 *   |got_fibre - exact_fibre|_2 <= 8 m u |old_fibre|_2,
 * a first-order worst case: a radix-2 stage costs one rounding for the sum or difference, two for the 1/sqrt2 scale and its rounded
 * constant, sqrt(5) u for the product with a twiddle and 1.5 u for the twiddle itself (under 6.8 u per stage), plus one more twiddle
 * product per pass.  Every twiddle exponent is formed exactly in integers modulo its power of two before any floating-point
 * operation; for both precisions the sine and cosine come from double arithmetic (a per-pass table built by the host's libm from
 * an octant-reduced exponent for the stages, a device evaluation in double for the one outer twiddle per amplitude and pass) and
 * are rounded once to the state's precision.  The scale 2^(-L/2) of a pass of L stages is applied once, folded into the outer
 * twiddle.  Fibres never mix: a fibre that is zero on entry is zero on exit, of either sign.  No atomics: the same call on the
 * same state gives the same bits, whatever the grid.
 *
 * Cost.  Decimation in frequency from the register's most significant bit down.  A pass takes a contiguous range of register
 * bits whose index positions fit one tile, the wave row (index positions 0..5) plus at most 6 register positions outside it,
 * cut greedily from the top; register bits inside the row are free.  A block loads its tile as whole rows into LDS (64 KiB of
 * Complex<f64> at most, two blocks per CU), runs up to 12 radix-2 stages on it, three at a time in registers, multiplies by the
 * outer twiddle and stores the rows back in place: every amplitude is read once and written once per pass.  Every group of three
 * stages exchanges through LDS, the stages on bits of the wave row included: wave shuffles for those are NOT built, so a pass of
 * 12 stages makes four LDS round trips beside its staging.  With h register
 * positions outside the row there are P = max(1, ceil(h / 6)) tile passes.  QIPX_QFT_REVERSED runs exactly these and never
 * touches the scratch buffer.  Natural order in ONE pass is one pass (the digit reversal is a slot permutation on the way out of
 * LDS); natural order with P > 1 closes with one bit-reversal sweep through the bit-permutation kernel of
 * qip_hip_state_permute_bits, P + 1 passes: THIS case allocates the handle's scratch buffer (or uses the caller's, for a wrapped
 * state) before anything is queued and leaves the result in it as the current buffer, as qip_hip_state_permute_bits does.  The twiddle tables (at most
 * 32 KiB per pass) live in the device buffer of the handle that qipx_state_apply_diagonal, qipx_state_apply_function and
 * qipx_state_apply_multiplexed use.
 * Measured at n = 30 (tools/bench_qft.py, profiles/qft.md), Complex<f64> / Complex<f32>, beside one H gate pass of 5.3 / 2.8 ms: a tile
 * pass of 12 stages takes 10.4 - 10.6 / 7.9 ms (2.0 / 2.8 gate passes: it is bound by its LDS round trips and arithmetic, not by
 * memory, which is open); m = 12 on the top index bits 14.4 / 9.9 ms reversed (2 passes) and 19.7 / 12.5 ms natural (3); m = 16 on
 * the top bits 21.4 / 14.3 and 26.7 / 16.8 ms; m = n = 30 34.5 / 24.7 ms reversed (4 passes) and 40.9 / 28.4 ms natural (5).  The
 * lowered circuit through apply_ops was timed in three modes.  Default (the interpreter's sweeps): 1.22 - 2.35 / 1.04 - 1.89 times
 * the call on every shape (m = n = 30 natural: 96.0 / 53.7 ms).  Compiled IEEE-equal sweeps (tile = 1 + tile_jit): the call wins on
 * every shape in Complex<f64> (whole register 40.9 against 59.6 ms) and LOSES in Complex<f32> on m = 12 on the low bits reversed
 * (7.86 against 7.20 ms) and on m = 16 (16.84 against 16.76 and 14.31 against 13.56 ms).  The 1e-12 mode (tile = 2 + tile_jit +
 * tile_fma + tile_merge): in Complex<f64> the call wins on m = 12 and m = 16 (1.05 - 1.52 times) and LOSES on the whole register,
 * 40.9 against 35.1 ms natural and 34.5 against 28.4 ms reversed; in Complex<f32> it wins only on m = 12 natural on the low bits
 * (1.12) and m = 12 on the top bits (1.03 - 1.04) and LOSES on m = 12 low reversed (7.86 against 6.15 ms), m = 16 (16.8 against
 * 16.2 and 14.3 against 13.2 ms) and the whole register (28.4 against 20.2 and 24.7 against 16.9 ms).  At n = 26 Complex<f64> also
 * LOSES on m = 16 (1.70 against 1.55 ms) and is level on the whole register.
 *
 * Calling contract.  That of qipx_state_apply_function: the state is changed in place, the launches are queued on the handle's
 * stream and the call returns without waiting (a relabelled state is put back in the caller's order first; an unusable one is
 * refused with QIP_ERR_DEVICE); `qubits` may be freed or rewritten as soon as the call returns.  Each of these is QIP_ERR_INVALID
 * with a message, before anything is queued, the state untouched: a null handle (there is no host fall-back); a null `qubits` with
 * m > 0 ("null qubit array"); a qubit >= n ("out of range"); a qubit listed twice ("repeated"); unknown flag bits.
 *
 * qipx_qft_passes is host-only: the passes over the vector that the call makes on a state of `dtype` (QIP_C64 / QIP_C32) on n
 * qubits, P with QIPX_QFT_REVERSED or when P = 1, P + 1 otherwise, 0 for m = 0, after the same checks with the same messages.  It
 * needs no device.  (`dtype` is there so that Complex<f32> may later take seven positions per pass; both precisions take six.)
 *
 * Out of scope: the approximate QFT that drops small rotations, transforms of non-power-of-two size, the sharded state,
 * recording the call into programs / hipGraph, apply_ops fusion, the builder, replay and QASM, the C++ mirror.  There is no
 * option, and the launches are not a kernel class of the profile (the closing sweep counts as the bit permutation it is). */
#define QIPX_QFT_INVERSE 1u
#define QIPX_QFT_REVERSED 2u
int qipx_state_apply_qft(qip_hip_state* s, const uint64_t* qubits, uint32_t m, uint32_t flags);
int qipx_qft_passes(int dtype, uint32_t n, const uint64_t* qubits, uint32_t m, uint32_t flags, uint32_t* passes);

/* Noise channels on a device state by quantum trajectories.  (Purely additive again.)
 *
 * A channel {K_i} on one or two qubits acts on a state vector by drawing branch i with probability |K_i psi|^2 / |psi|^2 and
 * replacing psi by K_i psi, rescaled to the old norm.  Every branch weight comes from ONE read, |K_i psi|^2 = Tr(K_i^H K_i rho)
 * with rho the reduced density matrix on the channel's qubits, and the pass that applies the chosen operator of one channel forms
 * rho for the NEXT channel from the amplitudes it holds anyway: a chain of nch channels costs nch + 1 passes over the vector, not
 * 2 nch.
 *
 * qipx_state_apply_reduce is that pass by itself: psi <- (A on `indices`) psi in place, A any complex 2^k x 2^k matrix (2 * 4^k
 * doubles, row-major, bit i of a row = qubit indices[i], the convention of qipx_state_reduced_density), unitary or not; rho_next
 * = the raw reduced density matrix of the RESULT on next_indices, layout and conventions of qipx_state_reduced_density.
 * Supported: k, k2 in {1, 2}; the lists may overlap or be equal; together they cover at most three qubits.  More (k or k2 = 3,
 * a union of four) is QIP_ERR_UNSUPPORTED; the message of a union of four names both lists.  k or k2 = 0, an index >= n, a repeated
 * index within a list, a null pointer and a null handle are QIP_ERR_INVALID; an unusable handle is QIP_ERR_DEVICE.  Everything is
 * checked before the first launch: on a refusal neither the state nor rho_next is touched.
 *
 * Kernel.  ONE launch of k_apply_density_small (csrc/qip_channel_kernels.h) plus the fold.  G is the sorted union of the two
 * lists' index positions; the gather is the k <= 3 density kernel's on G (high positions walked, lane-id bits transposed in the
 * wave, the packed half bit of Complex<f32>), every element read once with a non-temporal 16-byte load and written once, in
 * place, to the address it came from; no second buffer, no atomics, and no lane writes what another lane reads.  The host hands
 * the operator over expanded to G (A on its qubits, the identity on the rest) as kernel arguments in double.
 *
 * Arithmetic.  y[a] = sum_a' W[a][a'] x[a'] in double for both precisions (f32 amplitudes widened first, the result rounded once
 * to f32): per part one chain of fused multiply-adds in ascending a' (Re: wr xr', then -wi xi'; Im: wr xi', then wi xr').  An
 * operator that is diagonal on G (the identity and every diagonal A) runs a kernel variant that looks at W[a][a] only and does not
 * multiply by a real or imaginary part that is exactly zero: the identity returns every amplitude bit for bit, and a zero on the
 * diagonal gives exactly +0.  Every other operator multiplies all 2^|G| entries of a row, the zeros of the identity padding
 * included (a row whose products are all zero still gives exactly +0; measured, the uniform loop beats skipping entries by
 * flags, profiles/noise.md).  rho is formed from the STORED result
 * (the f32-rounded value for a Complex<f32> state) by the products and fused multiply-adds of qipx_state_reduced_density on G;
 * the host then sums over the qubits of G that are not in next_indices, in ascending order of their bits, and moves rows and
 * columns to the caller's order.  The entries a <= a' are computed once and mirrored: rho_next is exactly Hermitian with +0.0
 * diagonal imaginary parts, and a permuted next_indices list gives the bit-exact row/column permutation.
 *
 * Determinism.  One partial matrix per block in the handle's reduction scratch (at most 4096 blocks of 4^|G| doubles, 2 MiB, plus
 * one matrix), folded entry by entry in block order on the device.  The same call on the same state returns the same bits, in
 * the state and in rho_next.
 *
 * Error statement.  An amplitude of the result is within (2 M + 2) u |A|_F |x| of the exact product for its group x of M = 2^|G|
 * amplitudes (u = 2^-53; one more rounding to 2^-24 for Complex<f32>): well inside 1e-12 |A| |psi| and 1e-5 |A| |psi|.  An entry of
 * rho_next is within c u * 2 S of the exact sum over the stored amplitudes as stated for qipx_state_reduced_density, the trace
 * over at most two further qubits adding 3 to its chain count: c <= 1106 at n = 30, below 4500, so every entry is within
 * 1e-12 * sqrt(rho[a][a] rho[a'][a']) (tests/test_gpu_f3_noise.py holds both to these bars).
 *
 * Calling contract.  A relabelled state (option "tile_relabel" = 3) is put back in the caller's order on entry.  The call is
 * ordered after the work queued on the handle and complete when it returns.
 *
 * qipx_state_apply_channels is the trajectory step.  ch[c].kraus holds `count` matrices of 2 * 4^k doubles each in the convention
 * above, 1 <= count <= 16, k in {1, 2}; count = 1 is a plain gate, any matrix, taken with certainty.  For c = 0 .. nch-1 in order,
 * with rho the raw reduced density matrix of the CURRENT state on ch[c]'s qubits:
 *   w_i = Re Tr(K_i^H K_i rho), E_i = K_i^H K_i formed in double on the host, the trace summed over entries in row-major order;
 *   W = sum_i w_i in index order, N = tr rho;
 *   chosen[c] = the smallest i with rand_u01[c] * W < w_0 + .. + w_i, or the last i with w_i > 0 if none qualifies (the rule of
 *   soft_measure: a branch of weight zero is never taken);
 *   psi <- sqrt(N / w_chosen) K_chosen psi, the scale folded into the matrix handed to the kernel: the norm is carried through.
 * Nothing requires sum_i K_i^H K_i = 1.  W <= 0 or a weight that is not finite is QIP_ERR_INVALID and the state is left as the
 * preceding channels left it.  chosen[c], and weights (if not null: the w_i of all channels one after another, sum of ch[c].count
 * doubles), are filled for every channel that ran.  rand_u01[c] must lie in [0, 1].
 *
 * Pass plan: one read-only reduced-density pass for ch[0]; for every c < nch-1 one fused pass (apply ch[c], reduce on ch[c+1])
 * when the two cover at most three qubits AND the fused pass was measured faster than the two calls it replaces, otherwise a
 * dense apply followed by a reduced-density pass; the last channel is a dense apply through the path of qip_hip_state_apply_op
 * (in the state's precision).  Measured slower and therefore run composed (tools/bench_noise.py, profiles/noise.md): a step of
 * three qubits on a Complex<f32> state, and for n >= 28 a step of at most two qubits none of which is an index bit inside a wave
 * row of 64 elements (index bits 0..5; 0..6 for Complex<f32>).  nch channels on steps that fuse cost nch + 1 passes.
 * qipx_state_channel_passes returns the plan of that handle (its n and precision) from pure host code after the same checks of
 * the list: *passes is the number of passes over the vector, *fused how many of them are fused passes.  qipx_channel_passes is
 * the same for a Complex<f64> state of n qubits and needs no handle and no device.
 * Refusals before anything runs: a null handle, a null channel, index, operator, sample or result array, k = 0, an index >= n
 * or repeated, count = 0 or > 16, a sample outside [0, 1] (QIP_ERR_INVALID); k > 2 (QIP_ERR_UNSUPPORTED).  nch = 0 does nothing.
 * The call is complete when it returns.
 *
 * Profile.  The fused pass and the reduced-density call are kernel classes of the profile (option "profile"), numbered after
 * those of qip_hip_kernel_class_count, which keep their count and indices: qipx_kernel_class_count / qipx_kernel_class_name
 * cover both ranges and qipx_state_profile_get reads any of them, as qip_hip_state_profile_get reads the first range.
 *
 * Out of scope: batching many trajectories in one state, channels on three or more qubits, channels inside tile sweeps, the
 * sharded state. */
typedef struct qipx_channel {
  const uint64_t* indices; /* k qubits */
  uint32_t k;
  const double* kraus;     /* count matrices of 2 * 4^k doubles */
  uint32_t count;
} qipx_channel;
int qipx_state_apply_reduce(qip_hip_state* s, const uint64_t* indices, uint32_t k, const double* matrix, const uint64_t* next_indices,
                            uint32_t k2, double* rho_next);
int qipx_state_apply_channels(qip_hip_state* s, const qipx_channel* ch, uint64_t nch, const double* rand_u01, uint32_t* chosen,
                              double* weights /* may be null */);
int qipx_channel_passes(uint32_t n, const qipx_channel* ch, uint64_t nch, uint64_t* passes, uint64_t* fused);
int qipx_state_channel_passes(qip_hip_state* s, const qipx_channel* ch, uint64_t nch, uint64_t* passes, uint64_t* fused);
int qipx_kernel_class_count(void);
const char* qipx_kernel_class_name(int cls);
int qipx_state_profile_get(qip_hip_state* s, int cls, uint64_t* launches, double* total_ms, double* algorithmic_bytes);

#ifdef __cplusplus
}
#endif

#endif /* QIP_HIPX_H */
