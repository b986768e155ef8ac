// qip_channel.hip — noise channels on a device state by quantum trajectories (include/qip_hipx.h: qipx_state_apply_reduce,
// qipx_state_apply_channels, qipx_channel_passes).
//   check   every list, count and pointer before the first launch (qip_channel_plan.h: all that qipx_channel_passes runs)
//   plan    qip_channel_plan.h: the union G, the operator expanded to G, the pass plan of a chain, weights and selection
//   launch  one k_apply_density_small launch per fused pass (qip_channel_kernels.h) on the geometry, the grid and the fold of the k <= 3 density call
//           (qip_measure.hip: dens_small_geom, dens_small_dispatch, dens_small_collect); 4^|G| doubles come back
//   trace   the host traces G down to the next qubits and permutes to the caller's order (chan_trace)
// The first density of a chain, the unfused steps and the last apply go through the calls that exist for them
// (qipx_state_reduced_density, qip_hip_state_apply_op).
#include "qip_internal.h"
#include "../../include/qip_hipx.h"
#include "qip_channel_kernels.h"
#include "qip_channel_plan.h"

namespace {
template <bool DIAG>
struct ChanLaunch {  // what dens_small_dispatch launches for one (KE, KL, B0): k_apply_density_small
  const ChanW& cw;
  template <typename T, int KE, int KL, bool B0, typename E>
  void run(qip_hip_state* s, const DensSmallGeom& g) const {
    hipLaunchKernelGGL((k_apply_density_small<T, KE, KL, B0, DIAG, E>), dim3(g.gx), dim3(kBlock), 0, s->stream, (E*)s->cur, g.ins, g.d, cw, s->d_partial);
  }
};
}  // namespace

// One fused pass: psi <- scale * (A on apos) psi in place, rho_next = the density of the result on bpos.  Everything was checked.
static int apply_reduce_pass(qip_hip_state* s, const std::vector<uint32_t>& apos, const double* a, double scale, const std::vector<uint32_t>& bpos,
                             double* rho_next) {
  const ChanUnion u = chan_union(apos, bpos);
  const uint32_t M = 1u << u.g.size();
  ChanW cw;
  memset(&cw, 0, sizeof cw);
  bool diag = false;
  chan_expand(u, (uint32_t)apos.size(), a, scale, cw.w, cw.nzr, cw.nzi, &diag);
  const DensSmallGeom g = dens_small_geom(s, u.g);  // the density call's geometry on G, its grid and its fold
  const size_t nout = (size_t)M * M;
  QCHK(ensure_partial(s, (size_t)g.gx * nout + nout));
  ProfRec rec;
  if (s->profile) QCHK(prof_begin(s, KCX_APPLY_DENSITY, 2.0 * (double)s->amp_bytes * (double)s->namps, &rec));
  if (diag) dens_small_dispatch(s, g, ChanLaunch<true>{cw});
  else dens_small_dispatch(s, g, ChanLaunch<false>{cw});
  const hipError_t launched = hipGetLastError();
  if (s->profile) QCHK(prof_end(s, &rec));  // (the pair is closed whether the launch succeeded or not)
  HIPCHK(launched);
  std::vector<double> up;
  QCHK(dens_small_collect(s, g.gx, M, &up));
  chan_trace(u, (uint32_t)bpos.size(), up.data(), rho_next);
  return QIP_OK;
}

static std::string list_text(const uint64_t* q, uint32_t k) {
  std::string t = "[";
  for (uint32_t i = 0; i < k; ++i) t += (i ? ", " : "") + std::to_string((unsigned long long)q[i]);
  return t + "]";
}

extern "C" int qipx_state_apply_reduce(qip_hip_state* s, const uint64_t* indices, uint32_t k, const double* matrix,
                                       const uint64_t* next_indices, uint32_t k2, double* rho_next) try {
  STATE_ENTER_RAW(s);
  const char* what = "apply_reduce";
  if (!indices || !next_indices || !matrix || !rho_next) return fail(QIP_ERR_INVALID, "%s: null argument", what);
  std::vector<uint32_t> apos, bpos;
  std::string err = chan_check_indices(s->n, indices, k, &apos);
  if (!err.empty()) return fail(QIP_ERR_INVALID, "%s: %s (indices)", what, err.c_str());
  err = chan_check_indices(s->n, next_indices, k2, &bpos);
  if (!err.empty()) return fail(QIP_ERR_INVALID, "%s: %s (next_indices)", what, err.c_str());
  if (k > kChanMaxK || k2 > kChanMaxK)
    return fail(QIP_ERR_UNSUPPORTED, "%s: an operator on %u qubits and a density on %u, at most %u each", what, k, k2, kChanMaxK);
  if (chan_union_size(apos, bpos) > kChanMaxUnion)
    return fail(QIP_ERR_UNSUPPORTED, "%s: indices %s and next_indices %s cover %u qubits together, at most %u fit one pass", what,
                list_text(indices, k).c_str(), list_text(next_indices, k2).c_str(), chan_union_size(apos, bpos), kChanMaxUnion);
  if (!s->layout.empty()) QCHK(state_settle(s));  // a relabelled state: the caller's order first (nothing was launched before)
  return apply_reduce_pass(s, apos, matrix, 1.0, bpos, rho_next);
} QIP_CATCH_ALL

// the checks of a channel list, shared by the two calls below
static int check_channels(uint32_t n, const qipx_channel* ch, uint64_t nch, std::vector<std::vector<uint32_t>>* pos) {
  const char* what = "channels";
  if (nch > 0 && !ch) return fail(QIP_ERR_INVALID, "%s: null channel array", what);
  pos->resize((size_t)nch);
  for (uint64_t c = 0; c < nch; ++c) {
    const std::string err = chan_check_indices(n, ch[c].indices, ch[c].k, &(*pos)[(size_t)c]);
    if (!err.empty()) return fail(QIP_ERR_INVALID, "%s: channel %llu: %s", what, (unsigned long long)c, err.c_str());
    if (ch[c].k > kChanMaxK)
      return fail(QIP_ERR_UNSUPPORTED, "%s: channel %llu acts on %u qubits, at most %u", what, (unsigned long long)c, ch[c].k, kChanMaxK);
    if (ch[c].count < 1 || ch[c].count > kChanMaxKraus)
      return fail(QIP_ERR_INVALID, "%s: channel %llu has %u operators, 1 to %u are supported", what, (unsigned long long)c, ch[c].count, kChanMaxKraus);
    if (!ch[c].kraus) return fail(QIP_ERR_INVALID, "%s: channel %llu has a null operator array", what, (unsigned long long)c);
  }
  return QIP_OK;
}

extern "C" int qipx_channel_passes(uint32_t n, const qipx_channel* ch, uint64_t nch, uint64_t* passes, uint64_t* fused) try {
  if (!passes || !fused) return fail(QIP_ERR_INVALID, "null output");
  *passes = *fused = 0;
  std::vector<std::vector<uint32_t>> pos;
  QCHK(check_channels(n, ch, nch, &pos));
  const ChanPlan p = chan_plan(n, false, false, pos);
  *passes = p.passes;
  *fused = p.nfused;
  return QIP_OK;
} QIP_CATCH_ALL

static ChanPlan state_plan(const qip_hip_state* s, const std::vector<std::vector<uint32_t>>& pos) {
  const bool f32 = s->dtype != QIP_C64;
  return chan_plan(s->n, f32, f32 && s->packed_f32 && s->n >= 2, pos);
}

extern "C" int qipx_state_channel_passes(qip_hip_state* s, const qipx_channel* ch, uint64_t nch, uint64_t* passes, uint64_t* fused) try {
  if (!s) return fail(QIP_ERR_INVALID, "null state handle");
  if (!passes || !fused) return fail(QIP_ERR_INVALID, "null output");
  *passes = *fused = 0;
  std::vector<std::vector<uint32_t>> pos;
  QCHK(check_channels(s->n, ch, nch, &pos));
  const ChanPlan p = state_plan(s, pos);
  *passes = p.passes;
  *fused = p.nfused;
  return QIP_OK;
} QIP_CATCH_ALL

// scale * K on `indices` through the dense path of apply_op: its Matrix op takes indices[0] as the MOST significant row bit, so
// the list goes in reversed and the matrix as it is, in the state's precision
static int dense_apply(qip_hip_state* s, const uint64_t* indices, uint32_t k, const double* K, double scale) {
  const size_t len = (size_t)2 << (2 * k);
  uint64_t rev[kChanMaxK];
  for (uint32_t i = 0; i < k; ++i) rev[i] = indices[k - 1 - i];
  std::vector<double> m64(len);
  for (size_t i = 0; i < len; ++i) m64[i] = scale != 1.0 ? K[i] * scale : K[i];
  std::vector<float> m32;
  qip_op op;
  memset(&op, 0, sizeof op);
  op.kind = QIP_OP_MATRIX;
  op.n_indices = k;
  op.indices = rev;
  op.dense = m64.data();
  if (s->dtype != QIP_C64) {
    m32.assign(m64.begin(), m64.end());
    op.dense = m32.data();
  }
  QCHK(qip_hip_state_apply_op(s, &op));
  return hipStreamSynchronize(s->stream) == hipSuccess ? QIP_OK : fail(QIP_ERR_DEVICE, "channels: the dense apply failed");  // (the op's payload is ours)
}

extern "C" int qipx_state_apply_channels(qip_hip_state* s, const qipx_channel* ch, uint64_t nch, const double* rand_u01, uint32_t* chosen,
                                         double* weights) try {
  STATE_ENTER_RAW(s);
  const char* what = "apply_channels";
  std::vector<std::vector<uint32_t>> pos;
  QCHK(check_channels(s->n, ch, nch, &pos));
  if (nch == 0) return QIP_OK;
  if (!rand_u01 || !chosen) return fail(QIP_ERR_INVALID, "%s: null sample or result array", what);
  for (uint64_t c = 0; c < nch; ++c)
    if (!(rand_u01[c] >= 0.0 && rand_u01[c] <= 1.0)) return fail(QIP_ERR_INVALID, "%s: rand_u01[%llu] is not in [0, 1]", what, (unsigned long long)c);
  if (!s->layout.empty()) QCHK(state_settle(s));
  const ChanPlan plan = state_plan(s, pos);
  double rho[2 * 16], next[2 * 16], w[kChanMaxKraus];
  QCHK(qipx_state_reduced_density(s, ch[0].indices, ch[0].k, rho));
  size_t wat = 0;
  for (uint64_t c = 0; c < nch; ++c) {
    const uint32_t k = ch[c].k, M = 1u << k;
    const size_t len = (size_t)2 * M * M;
    for (uint32_t i = 0; i < ch[c].count; ++i) w[i] = chan_weight(k, ch[c].kraus + i * len, rho);
    double W = 0.0, N = 0.0;
    for (uint32_t a = 0; a < M; ++a) N += rho[2 * (a * M + a)];
    const int pick = chan_select(w, ch[c].count, rand_u01[c], &W);
    if (weights)
      for (uint32_t i = 0; i < ch[c].count; ++i) weights[wat + i] = w[i];
    wat += ch[c].count;
    if (pick < 0)
      return fail(QIP_ERR_INVALID, "%s: channel %llu has no branch to take (total weight %g): the state is as the %llu channels before it left it",
                  what, (unsigned long long)c, W, (unsigned long long)c);
    chosen[c] = (uint32_t)pick;
    const double scale = sqrt(N / w[pick]);
    const double* K = ch[c].kraus + (size_t)pick * len;
    if (c + 1 == nch) {
      QCHK(dense_apply(s, ch[c].indices, k, K, scale));
    } else if (plan.fused[(size_t)c]) {
      QCHK(apply_reduce_pass(s, pos[(size_t)c], K, scale, pos[(size_t)c + 1], next));
      memcpy(rho, next, sizeof rho);
    } else {
      QCHK(dense_apply(s, ch[c].indices, k, K, scale));
      QCHK(qipx_state_reduced_density(s, ch[c + 1].indices, ch[c + 1].k, rho));
    }
  }
  return QIP_OK;
} QIP_CATCH_ALL
