// qip_function.hip — classical functions between qubit registers on a device state (include/qip_hipx.h:
// qipx_state_apply_function, qipx_function_passes).
//   check   the registers and the mode (fn_shape: all that qipx_function_passes runs), then the values and the phases
//   plan    qip_function_plan.h: the passes, the tile and the descriptor of each
//   table   one 32-bit word per x and pass, then w(x) in the state's precision, written straight into the pinned copy whose turn
//           it is of the handle's table buffer (qip_pauli.hip: table_stage / table_commit, the diagonal sums' path) and uploaded
//           stream-ordered: the caller's arrays are not read after the call returns
//   launch  one k_function_tile launch per pass (qip_function_kernels.h), queued on the handle's stream
#include "qip_internal.h"
#include "../../include/qip_hipx.h"
#include "qip_function_kernels.h"

namespace {
struct FnShape {
  std::vector<uint32_t> ipos, opos;  // index position of bit i of x / y
};
}  // namespace

static int fn_shape(uint32_t n, const uint64_t* in_qubits, uint32_t m, const uint64_t* out_qubits, uint32_t k, int mode, FnShape* sh) {
  const char* what = "apply_function";
  if (n < 1 || n > 63) return fail(QIP_ERR_INVALID, "%s: %u qubits", what, n);
  if (mode != QIPX_FN_XOR && mode != QIPX_FN_ADD) return fail(QIP_ERR_INVALID, "%s: unknown mode %d", what, mode);
  if (m > kFnMaxIn) return fail(QIP_ERR_INVALID, "%s: an in register of %u qubits, at most %u are supported", what, m, kFnMaxIn);
  if (k > kFnMaxOut) return fail(QIP_ERR_INVALID, "%s: an out register of %u qubits, at most %u are supported", what, k, kFnMaxOut);
  if ((m > 0 && !in_qubits) || (k > 0 && !out_qubits)) return fail(QIP_ERR_INVALID, "%s: null qubit array", what);
  uint64_t in_seen = 0, out_seen = 0;
  for (uint32_t i = 0; i < m + k; ++i) {
    const bool in = i < m;
    const uint64_t q = in ? in_qubits[i] : out_qubits[i - m];
    if (q >= n) return fail(QIP_ERR_INVALID, "%s: qubit %llu out of range", what, (unsigned long long)q);
    const uint64_t bit = 1ull << (n - 1 - q);
    if ((in ? in_seen : out_seen) & bit) return fail(QIP_ERR_INVALID, "%s: qubit %llu repeated", what, (unsigned long long)q);
    if (in_seen & bit) return fail(QIP_ERR_INVALID, "%s: qubit %llu is in both registers", what, (unsigned long long)q);
    (in ? in_seen : out_seen) |= bit;
    (in ? sh->ipos : sh->opos).push_back((uint32_t)(n - 1 - q));
  }
  if (mode == QIPX_FN_ADD && fn_out_high(sh->opos) > kFnTileHigh)
    return fail(QIP_ERR_INVALID, "%s: QIPX_FN_ADD with %u out positions outside the six low index bits, at most %u fit one tile", what,
                fn_out_high(sh->opos), kFnTileHigh);
  return QIP_OK;
}

extern "C" int qipx_function_passes(uint32_t n, const uint64_t* in_qubits, uint32_t m, const uint64_t* out_qubits, uint32_t k, int mode,
                                    uint32_t* passes) try {
  if (!passes) return fail(QIP_ERR_INVALID, "null output");
  *passes = 0;
  FnShape sh;
  QCHK(fn_shape(n, in_qubits, m, out_qubits, k, mode, &sh));
  *passes = fn_pass_count(sh.opos);
  return QIP_OK;
} QIP_CATCH_ALL

template <typename T, int U, int MODE, bool PH>
static void fn_launch_nt(qip_hip_state* s, const FnPass& P, const Ins& ins, const uint32_t* tab, const amp_t<T>* w) {
  const dim3 grid = grid2d(P.ntiles, 1), block(P.threads);
  const size_t lds = MODE == kFnPhaseOnly ? 0 : sizeof(amp_t<T>) << (6 + P.d.kt);  // at most 64 KiB
  if (use_nt(s)) hipLaunchKernelGGL((k_function_tile<T, U, MODE, PH, true>), grid, block, lds, s->stream, (amp_t<T>*)s->cur, P.ntiles, ins, P.d, tab, w);
  else hipLaunchKernelGGL((k_function_tile<T, U, MODE, PH, false>), grid, block, lds, s->stream, (amp_t<T>*)s->cur, P.ntiles, ins, P.d, tab, w);
}

template <typename T, int U>
static void fn_launch_u(qip_hip_state* s, const FnPass& P, const Ins& ins, const uint32_t* tab, const amp_t<T>* w) {
  if (P.mode == kFnPhaseOnly) fn_launch_nt<T, U, kFnPhaseOnly, true>(s, P, ins, tab, w);
  else if (P.mode == kFnAdd) P.phase ? fn_launch_nt<T, U, kFnAdd, true>(s, P, ins, tab, w) : fn_launch_nt<T, U, kFnAdd, false>(s, P, ins, tab, w);
  else P.phase ? fn_launch_nt<T, U, kFnXor, true>(s, P, ins, tab, w) : fn_launch_nt<T, U, kFnXor, false>(s, P, ins, tab, w);
}

template <typename T>
static int function_t(qip_hip_state* s, const FnShape& sh, int mode, const uint64_t* values, const double* phases) {
  using A = amp_t<T>;
  const std::vector<FnPass> plan = fn_plan(s->n, sh.ipos, sh.opos, mode, phases != nullptr);
  const size_t entries = (size_t)1 << sh.ipos.size();
  const size_t words = sh.opos.empty() ? 0 : plan.size() * entries;
  const size_t off_w = (words * sizeof(uint32_t) + 15) & ~(size_t)15;
  const size_t bytes = off_w + (phases ? entries * sizeof(A) : 0);
  char* h = nullptr;
  uint32_t turn = 0;
  QCHK(table_stage(s, std::max<size_t>(bytes, 16), &h, &turn));
  uint32_t* hw = (uint32_t*)h;
  for (size_t ps = 0; ps < plan.size() && words; ++ps) {
    const FnPass& P = plan[ps];
    uint32_t* row = hw + ps * entries;
    if (P.mode == kFnAdd) {
      for (size_t x = 0; x < entries; ++x) row[x] = (uint32_t)values[x];
    } else {  // XOR: the value's bits of this pass, spread over the tile's slot bits
      for (size_t x = 0; x < entries; ++x) row[x] = fn_xor_word(P, values[x]);
    }
  }
  if (phases) {
    A* hp = (A*)(h + off_w);
    for (size_t x = 0; x < entries; ++x) hp[x] = mk<T>(cos(phases[x]), sin(phases[x]));  // in double, rounded once
  }
  if (bytes) QCHK(table_commit(s, turn, bytes));
  for (size_t ps = 0; ps < plan.size(); ++ps) {
    const FnPass& P = plan[ps];
    const Ins ins = make_ins(P.opened, 0);
    const uint32_t* tab = (const uint32_t*)s->d_diag + ps * entries;
    const A* w = (const A*)((const char*)s->d_diag + off_w);
    switch (P.rows_per_wave) {
      case 1: fn_launch_u<T, 1>(s, P, ins, tab, w); break;
      case 2: fn_launch_u<T, 2>(s, P, ins, tab, w); break;
      case 4: fn_launch_u<T, 4>(s, P, ins, tab, w); break;
      default: fn_launch_u<T, 8>(s, P, ins, tab, w); break;
    }
    HIPCHK(hipGetLastError());
  }
  return QIP_OK;
}

extern "C" int qipx_state_apply_function(qip_hip_state* s, const uint64_t* in_qubits, uint32_t m, const uint64_t* out_qubits, uint32_t k,
                                         int mode, const uint64_t* values, const double* phases) try {
  STATE_ENTER_RAW(s);
  const char* what = "apply_function";
  FnShape sh;
  QCHK(fn_shape(s->n, in_qubits, m, out_qubits, k, mode, &sh));
  if (k > 0 && !values) return fail(QIP_ERR_INVALID, "%s: null value array", what);
  if (k == 0 && values) return fail(QIP_ERR_INVALID, "%s: an empty out register takes no values", what);
  if (k == 0 && !phases) return fail(QIP_ERR_INVALID, "%s: an empty out register needs phases", what);
  const uint64_t entries = 1ull << m;
  if (k > 0 && k < 64)
    for (uint64_t x = 0; x < entries; ++x)
      if (values[x] >> k)
        return fail(QIP_ERR_INVALID, "%s: values[%llu] = %llu does not fit the out register of %u qubits", what, (unsigned long long)x,
                    (unsigned long long)values[x], k);
  if (phases)
    for (uint64_t x = 0; x < entries; ++x)
      if (!std::isfinite(phases[x])) return fail(QIP_ERR_INVALID, "%s: the phase of entry %llu is not finite", what, (unsigned long long)x);
  if (!s->layout.empty()) QCHK(state_settle(s));  // (a relabelled state: the caller's order first, as by STATE_ENTER)
  return s->dtype == QIP_C64 ? function_t<double>(s, sh, mode, values, phases) : function_t<float>(s, sh, mode, values, phases);
} QIP_CATCH_ALL
