// qip_qft.hip — the quantum Fourier transform of a qubit register on a device state (include/qip_hipx.h: qipx_state_apply_qft,
// qipx_qft_passes).
//   check   the register and the flags (qft_shape: all that qipx_qft_passes runs)
//   plan    qip_qft_plan.h: the passes, the tile, the steps and the descriptor of each
//   table   per pass W_(2^L)^j for j < 2^(L-1), evaluated in double from the integer exponent and rounded once to the state's
//           precision, written straight into the pinned copy whose turn it is of the handle's table buffer (qip_pauli.hip:
//           table_stage / table_commit) and uploaded stream-ordered
//   launch  one k_qft_tile launch per pass (qip_qft_kernels.h), queued on the handle's stream; a natural-order call of more than
//           one pass closes with the bit-reversal of the register through launch_permute (qip_launch.hip), which writes the
//           second buffer and makes it the current one
#include "qip_internal.h"
#include "../../include/qip_hipx.h"
#include "qip_qft_kernels.h"

static int qft_shape(uint32_t n, const uint64_t* qubits, uint32_t m, uint32_t flags, std::vector<uint32_t>* pos) {
  const char* what = "apply_qft";
  if (n < 1 || n > 63) return fail(QIP_ERR_INVALID, "%s: %u qubits", what, n);
  if (flags & ~(uint32_t)(QIPX_QFT_INVERSE | QIPX_QFT_REVERSED)) return fail(QIP_ERR_INVALID, "%s: unknown flag bits 0x%x", what, flags);
  if (m > 0 && !qubits) return fail(QIP_ERR_INVALID, "%s: null qubit array", what);
  uint64_t seen = 0;
  for (uint32_t i = 0; i < m; ++i) {
    const uint64_t q = qubits[i];
    if (q >= n) return fail(QIP_ERR_INVALID, "%s: qubit %llu out of range", what, (unsigned long long)q);
    const uint64_t bit = 1ull << (n - 1 - q);
    if (seen & bit) return fail(QIP_ERR_INVALID, "%s: qubit %llu repeated", what, (unsigned long long)q);
    seen |= bit;
    pos->push_back((uint32_t)(n - 1 - q));
  }
  return QIP_OK;
}

extern "C" int qipx_qft_passes(int dtype, uint32_t n, const uint64_t* qubits, uint32_t m, uint32_t flags, uint32_t* passes) try {
  if (!passes) return fail(QIP_ERR_INVALID, "null output");
  *passes = 0;
  if (dtype != QIP_C64 && dtype != QIP_C32) return fail(QIP_ERR_INVALID, "apply_qft: dtype %d is not a state precision", dtype);
  std::vector<uint32_t> pos;
  QCHK(qft_shape(n, qubits, m, flags, &pos));
  *passes = qft_pass_count(pos, (flags & QIPX_QFT_REVERSED) != 0);  // (six positions per pass in both precisions)
  return QIP_OK;
} QIP_CATCH_ALL

template <typename T, int E>
static void qft_launch(qip_hip_state* s, const QftPass& P, const Ins& ins, const amp_t<T>* tw) {
  const dim3 grid = grid2d(P.ntiles, 1), block(P.threads);
  const size_t lds = sizeof(amp_t<T>) << P.d.tbits;  // at most 64 KiB
  if (use_nt(s)) hipLaunchKernelGGL((k_qft_tile<T, E, true>), grid, block, lds, s->stream, (amp_t<T>*)s->cur, P.ntiles, ins, P.d, tw);
  else hipLaunchKernelGGL((k_qft_tile<T, E, false>), grid, block, lds, s->stream, (amp_t<T>*)s->cur, P.ntiles, ins, P.d, tw);
}

template <typename T>
static int qft_t(qip_hip_state* s, const std::vector<uint32_t>& pos, int sign, bool natural) {
  using A = amp_t<T>;
  const std::vector<QftPass> plan = qft_plan(s->n, pos, sign, natural);
  // (the closing sweep's buffer before anything is queued: a failed allocation leaves the state untouched)
  if (natural && plan.size() > 1) QCHK(ensure_alt(s));
  std::vector<size_t> off(plan.size());
  size_t bytes = 0;
  for (size_t ps = 0; ps < plan.size(); ++ps) {
    off[ps] = bytes;
    bytes += ((size_t)plan[ps].table_entries * sizeof(A) + 15) & ~(size_t)15;
  }
  char* h = nullptr;
  uint32_t turn = 0;
  QCHK(table_stage(s, std::max<size_t>(bytes, 16), &h, &turn));
  for (size_t ps = 0; ps < plan.size(); ++ps) {
    A* row = (A*)(h + off[ps]);
    const uint32_t L = plan[ps].d.hi - plan[ps].d.lo;
    for (uint32_t j = 0; j < plan[ps].table_entries; ++j) {
      double c, sn;
      qft_twiddle<double>(j, L, sign, &c, &sn);
      row[j] = mk<T>(c, sn);
    }
  }
  QCHK(table_commit(s, turn, bytes));
  for (size_t ps = 0; ps < plan.size(); ++ps) {
    const QftPass& P = plan[ps];
    const Ins ins = make_ins(P.opened, 0);
    const A* tw = (const A*)((const char*)s->d_diag + off[ps]);
    if (P.d.ebits == 3u) qft_launch<T, 3>(s, P, ins, tw);
    else qft_launch<T, 1>(s, P, ins, tw);
    HIPCHK(hipGetLastError());
  }
  if (natural && plan.size() > 1) {  // the flow leaves the register bit-reversed: destination bit pos[i] takes source bit pos[m-1-i]
    std::vector<uint32_t> pi(s->n);
    for (uint32_t b = 0; b < s->n; ++b) pi[b] = b;
    for (size_t i = 0; i < pos.size(); ++i) pi[pos[i]] = pos[pos.size() - 1 - i];
    QCHK(launch_permute(s, pi.data()));
  }
  return QIP_OK;
}

extern "C" int qipx_state_apply_qft(qip_hip_state* s, const uint64_t* qubits, uint32_t m, uint32_t flags) try {
  STATE_ENTER_RAW(s);
  std::vector<uint32_t> pos;
  QCHK(qft_shape(s->n, qubits, m, flags, &pos));
  if (m == 0) return QIP_OK;
  if (!s->layout.empty()) QCHK(state_settle(s));  // (a relabelled state: the caller's order first, as by STATE_ENTER)
  const bool inverse = (flags & QIPX_QFT_INVERSE) != 0, reversed = (flags & QIPX_QFT_REVERSED) != 0;
  if (inverse && reversed) std::reverse(pos.begin(), pos.end());  // reversed input, natural output: the flow on the reversed list
  const int sign = inverse ? -1 : 1;
  return s->dtype == QIP_C64 ? qft_t<double>(s, pos, sign, !reversed) : qft_t<float>(s, pos, sign, !reversed);
} QIP_CATCH_ALL
