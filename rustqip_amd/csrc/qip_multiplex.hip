// qip_multiplex.hip — multiplexed (uniformly controlled) 1- and 2-qubit gates on a device state (include/qip_hipx.h:
// qipx_state_apply_multiplexed, qipx_multiplexed_table_bytes).
//   check   the registers (mx_shape: all that qipx_multiplexed_table_bytes runs), then the matrices
//   plan    qip_multiplex_plan.h: the walk and its descriptor
//   table   the 2^m matrices rounded once to the state's precision, row-major, written straight into the pinned copy whose turn it
//           is of the handle's table buffer (qip_pauli.hip: table_stage / table_commit) and uploaded stream-ordered: the caller's
//           array is not read after the call returns
//   launch  one k_multiplex launch (qip_multiplex_kernels.h), queued on the handle's stream
#include "qip_internal.h"
#include "../../include/qip_hipx.h"
#include "qip_multiplex_kernels.h"

namespace {
struct MxShape {
  std::vector<uint32_t> spos, tpos;  // index position of bit i of x / of the matrix index
};
}  // namespace

static int mx_shape(uint32_t n, const uint64_t* select, uint32_t m, const uint64_t* targets, uint32_t k, MxShape* sh) {
  const char* what = "apply_multiplexed";
  if (n < 1 || n > 63) return fail(QIP_ERR_INVALID, "%s: %u qubits", what, n);
  if (k < 1 || k > kMxMaxK) return fail(QIP_ERR_INVALID, "%s: %u target qubits, 1 or 2 are supported", what, k);
  if (m > kMxMaxTableBits || m + 2 * k > kMxMaxTableBits)
    return fail(QIP_ERR_INVALID, "%s: %u select and %u target qubits, m + 2k is at most %u", what, m, k, kMxMaxTableBits);
  if ((m > 0 && !select) || !targets) return fail(QIP_ERR_INVALID, "%s: null qubit array", what);
  uint64_t sel_seen = 0, tgt_seen = 0;
  for (uint32_t i = 0; i < m + k; ++i) {
    const bool sel = i < m;
    const uint64_t q = sel ? select[i] : targets[i - m];
    if (q >= n) return fail(QIP_ERR_INVALID, "%s: qubit %llu out of range", what, (unsigned long long)q);
    const uint64_t bit = 1ull << (n - 1 - q);
    if ((sel ? sel_seen : tgt_seen) & bit) return fail(QIP_ERR_INVALID, "%s: qubit %llu repeated", what, (unsigned long long)q);
    if (sel_seen & bit) return fail(QIP_ERR_INVALID, "%s: qubit %llu is in both registers", what, (unsigned long long)q);
    (sel ? sel_seen : tgt_seen) |= bit;
    (sel ? sh->spos : sh->tpos).push_back((uint32_t)(n - 1 - q));
  }
  return QIP_OK;
}

extern "C" int qipx_multiplexed_table_bytes(int dtype, uint32_t n, const uint64_t* select, uint32_t m, const uint64_t* targets, uint32_t k,
                                            uint64_t* bytes) try {
  if (!bytes) return fail(QIP_ERR_INVALID, "null output");
  *bytes = 0;
  if (dtype != QIP_C64 && dtype != QIP_C32) return fail(QIP_ERR_INVALID, "apply_multiplexed: unknown dtype %d", dtype);
  MxShape sh;
  QCHK(mx_shape(n, select, m, targets, k, &sh));
  *bytes = ((uint64_t)(dtype == QIP_C64 ? 16 : 8)) << (m + 2 * k);
  return QIP_OK;
} QIP_CATCH_ALL

template <typename T, int K, int HM, int U>
static void mx_launch_nt(qip_hip_state* s, const MxPlan& P, const amp_t<T>* tab) {
  const dim3 grid = grid2d(P.nblocks, 1), block(P.threads);
  if (use_nt(s)) hipLaunchKernelGGL((k_multiplex<T, K, HM, U, true>), grid, block, 0, s->stream, (amp_t<T>*)s->cur, P.nwaves, P.d, tab);
  else hipLaunchKernelGGL((k_multiplex<T, K, HM, U, false>), grid, block, 0, s->stream, (amp_t<T>*)s->cur, P.nwaves, P.d, tab);
}

// (U is 1 or kMxLoads / H)
template <typename T, int K, int HM>
static void mx_launch_u(qip_hip_state* s, const MxPlan& P, const amp_t<T>* tab) {
  constexpr int UF = (int)kMxLoads / (HM == 3 ? 4 : HM == 0 ? 1 : 2);
  if constexpr (UF > 1) {
    if (P.U == (uint32_t)UF) return mx_launch_nt<T, K, HM, UF>(s, P, tab);
  }
  mx_launch_nt<T, K, HM, 1>(s, P, tab);
}

template <typename T>
static int multiplexed_t(qip_hip_state* s, const MxShape& sh, const double* matrices) {
  using A = amp_t<T>;
  const MxPlan P = mx_plan(s->n, sh.spos, sh.tpos);
  const size_t entries = (size_t)1 << (P.m + 2 * P.k);
  const size_t bytes = entries * sizeof(A);
  char* h = nullptr;
  uint32_t turn = 0;
  QCHK(table_stage(s, bytes, &h, &turn));
  A* ht = (A*)h;
  for (size_t e = 0; e < entries; ++e) ht[e] = mk<T>(matrices[2 * e], matrices[2 * e + 1]);  // rounded once
  QCHK(table_commit(s, turn, bytes));
  const A* tab = (const A*)s->d_diag;
  if (P.k == 1) {
    if (P.hm == 0) mx_launch_u<T, 1, 0>(s, P, tab);
    else mx_launch_u<T, 1, 1>(s, P, tab);
  } else {
    switch (P.hm) {
      case 0: mx_launch_u<T, 2, 0>(s, P, tab); break;
      case 1: mx_launch_u<T, 2, 1>(s, P, tab); break;
      case 2: mx_launch_u<T, 2, 2>(s, P, tab); break;
      default: mx_launch_u<T, 2, 3>(s, P, tab); break;
    }
  }
  HIPCHK(hipGetLastError());
  return QIP_OK;
}

extern "C" int qipx_state_apply_multiplexed(qip_hip_state* s, const uint64_t* select, uint32_t m, const uint64_t* targets, uint32_t k,
                                            const double* matrices) try {
  STATE_ENTER_RAW(s);
  const char* what = "apply_multiplexed";
  MxShape sh;
  QCHK(mx_shape(s->n, select, m, targets, k, &sh));
  if (!matrices) return fail(QIP_ERR_INVALID, "%s: null matrix array", what);
  const uint64_t doubles = 2ull << (m + 2 * k);
  for (uint64_t i = 0; i < doubles; ++i)
    if (!std::isfinite(matrices[i]))
      return fail(QIP_ERR_INVALID, "%s: entry %llu of matrix %llu is not finite", what, (unsigned long long)((i >> 1) & ((1ull << (2 * k)) - 1)),
                  (unsigned long long)(i >> (1 + 2 * k)));
  if (!s->layout.empty()) QCHK(state_settle(s));  // (a relabelled state: the caller's order first, as by STATE_ENTER)
  return s->dtype == QIP_C64 ? multiplexed_t<double>(s, sh, matrices) : multiplexed_t<float>(s, sh, matrices);
} QIP_CATCH_ALL
