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

#ifdef __cplusplus
}
#endif

#endif /* QIP_HIPX_H */
