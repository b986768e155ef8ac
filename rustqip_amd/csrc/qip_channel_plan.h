// qip_channel_plan.h — the host side of the noise-channel calls (qipx_state_apply_reduce, qipx_state_apply_channels,
// qipx_channel_passes of include/qip_hipx.h) that needs no device: the checks of a channel list, the union G of the qubits acted
// on and the qubits reduced next, the operator expanded to G, the trace from G down to the next qubits, the branch weights and the
// selection rule, and the pass plan.  What qip_channel.hip adds is the handle, the launches (qip_channel_kernels.h) and the fold.
//
// Plain C++17 as well as HIP, in the manner of qip_function_plan.h: no HIP types and no fail().
//
// Conventions.  Qubit q is index position n - 1 - q.  Bit i of a row of a caller's matrix is the bit of qubit indices[i] (the
// convention of qipx_state_reduced_density).  The kernel works on G's positions in ascending order: bit j of its row index g is
// the j-th lowest position of G.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

namespace qipk {

constexpr uint32_t kChanMaxK = 2;       // qubits of one channel
constexpr uint32_t kChanMaxUnion = 3;   // qubits of one fused pass: the channel's and the next one's
constexpr uint32_t kChanMaxKraus = 16;  // operators of one channel

// the checks of one index list (those of the density call); "" when it is good, the positions in the caller's order in *pos
inline std::string chan_check_indices(uint32_t n, const uint64_t* indices, uint32_t k, std::vector<uint32_t>* pos) {
  if (n < 1 || n > 63) return "a state of " + std::to_string(n) + " qubits";
  if (k == 0 || k > n || !indices) return "bad qubit index list";
  uint64_t seen = 0;
  pos->clear();
  for (uint32_t i = 0; i < k; ++i) {
    if (indices[i] >= n) return "qubit index out of range";
    if (seen & (1ull << indices[i])) return "repeated qubit index";
    seen |= 1ull << indices[i];
    pos->push_back((uint32_t)(n - 1 - indices[i]));
  }
  return "";
}

struct ChanUnion {
  std::vector<uint32_t> g;   // G: the positions of both lists, ascending
  uint32_t abit[kChanMaxK];  // bit of g that bit i of the operator's row index is
  uint32_t bbit[kChanMaxK];  // bit of g that bit i of the next density's row index is
  uint32_t amask = 0, bmask = 0;
};

inline ChanUnion chan_union(const std::vector<uint32_t>& apos, const std::vector<uint32_t>& bpos) {
  ChanUnion u;
  u.g = apos;
  u.g.insert(u.g.end(), bpos.begin(), bpos.end());
  std::sort(u.g.begin(), u.g.end());
  u.g.erase(std::unique(u.g.begin(), u.g.end()), u.g.end());
  auto bit_of = [&](uint32_t p) { return (uint32_t)(std::find(u.g.begin(), u.g.end(), p) - u.g.begin()); };
  for (size_t i = 0; i < apos.size() && i < kChanMaxK; ++i) {
    u.abit[i] = bit_of(apos[i]);
    u.amask |= 1u << u.abit[i];
  }
  for (size_t i = 0; i < bpos.size() && i < kChanMaxK; ++i) {
    u.bbit[i] = bit_of(bpos[i]);
    u.bmask |= 1u << u.bbit[i];
  }
  return u;
}

// how many positions the two lists cover together
inline uint32_t chan_union_size(const std::vector<uint32_t>& apos, const std::vector<uint32_t>& bpos) {
  uint64_t m = 0;
  for (uint32_t p : apos) m |= 1ull << p;
  for (uint32_t p : bpos) m |= 1ull << p;
  return (uint32_t)__builtin_popcountll(m);
}

// W = scale * (A on its qubits, the identity on the rest of G), 2 M^2 doubles in G's sorted bit order: W[g][g'] = A[a(g)][a(g')]
// when g and g' agree outside A's bits, else exactly +0.  nzr / nzi: per row, which entries have a real / imaginary part that is
// not zero (what the kernel variant for diagonal operators multiplies by).  *diag: no entry off the diagonal is non-zero.
inline void chan_expand(const ChanUnion& u, uint32_t k, const double* a, double scale, double* w, uint32_t* nzr, uint32_t* nzi, bool* diag) {
  const uint32_t M = 1u << u.g.size(), MA = 1u << k;
  auto sub = [&](uint32_t g) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < k; ++i) r |= ((g >> u.abit[i]) & 1u) << i;
    return r;
  };
  *diag = true;
  for (uint32_t g = 0; g < M; ++g) {
    nzr[g] = nzi[g] = 0;
    for (uint32_t g2 = 0; g2 < M; ++g2) {
      double re = 0.0, im = 0.0;
      if (((g ^ g2) & ~u.amask) == 0) {
        const size_t at = 2 * ((size_t)sub(g) * MA + sub(g2));
        re = a[at];
        im = a[at + 1];
        if (scale != 1.0) {
          re *= scale;
          im *= scale;
        }
      }
      w[2 * ((size_t)g * M + g2)] = re;
      w[2 * ((size_t)g * M + g2) + 1] = im;
      if (re != 0.0) nzr[g] |= 1u << g2;
      if (im != 0.0) nzi[g] |= 1u << g2;
      if (g != g2 && (re != 0.0 || im != 0.0)) *diag = false;
    }
  }
}

// rho on the next qubits from the density matrix on G.  `up`: the entries g <= g' of the matrix on G in sorted bit order,
// up[2 (g M + g')] and + 1.  The entries s <= s' in the next qubits' SORTED order are the sums over the other bits of G in
// ascending order (an entry with nothing to sum over is copied); then rows and columns go to the caller's bit order and the
// conjugates are written: rho is exactly Hermitian with +0.0 diagonal imaginary parts, and a permuted list permutes it exactly.
inline void chan_trace(const ChanUnion& u, uint32_t k2, const double* up, double* rho) {
  const uint32_t kg = (uint32_t)u.g.size(), M = 1u << kg, MB = 1u << k2, NR = 1u << (kg - k2);
  uint32_t sb[kChanMaxK], rb[kChanMaxUnion], ns = 0, nr = 0;
  for (uint32_t j = 0; j < kg; ++j) {
    if ((u.bmask >> j) & 1u) sb[ns++] = j;
    else rb[nr++] = j;
  }
  auto gidx = [&](uint32_t s, uint32_t r) {
    uint32_t g = 0;
    for (uint32_t j = 0; j < ns; ++j) g |= ((s >> j) & 1u) << sb[j];
    for (uint32_t j = 0; j < nr; ++j) g |= ((r >> j) & 1u) << rb[j];
    return g;
  };
  auto to_caller = [&](uint32_t s) {
    uint32_t c = 0;
    for (uint32_t i = 0; i < k2; ++i)
      for (uint32_t j = 0; j < ns; ++j)
        if (sb[j] == u.bbit[i]) c |= ((s >> j) & 1u) << i;
    return c;
  };
  for (uint32_t s = 0; s < MB; ++s) {
    const uint32_t cs = to_caller(s);
    for (uint32_t s2 = s; s2 < MB; ++s2) {
      double re = 0.0, im = 0.0;
      for (uint32_t r = 0; r < NR; ++r) {
        const size_t at = 2 * ((size_t)gidx(s, r) * M + gidx(s2, r));  // (s <= s' and shared other bits: g <= g')
        re = r == 0 ? up[at] : re + up[at];
        im = r == 0 ? up[at + 1] : im + up[at + 1];
      }
      const uint32_t cs2 = to_caller(s2);
      if (s == s2) {
        rho[2 * ((size_t)cs * MB + cs)] = re;
        rho[2 * ((size_t)cs * MB + cs) + 1] = 0.0;
      } else {
        rho[2 * ((size_t)cs * MB + cs2)] = re;
        rho[2 * ((size_t)cs * MB + cs2) + 1] = im;
        rho[2 * ((size_t)cs2 * MB + cs)] = re;
        rho[2 * ((size_t)cs2 * MB + cs) + 1] = -im;
      }
    }
  }
}

// w = Re Tr(K^H K rho) for one operator K (2 * 4^k doubles) and the raw reduced density matrix rho on its qubits: E = K^H K in
// double, E[a][b] = sum_c conj(K[c][a]) K[c][b] over ascending c, then the sum of Re(E[a][b] rho[b][a]) over (a, b) in row-major order.
inline double chan_weight(uint32_t k, const double* K, const double* rho) {
  const uint32_t M = 1u << k;
  double w = 0.0;
  for (uint32_t a = 0; a < M; ++a)
    for (uint32_t b = 0; b < M; ++b) {
      double er = 0.0, ei = 0.0;
      for (uint32_t c = 0; c < M; ++c) {
        const double xr = K[2 * (c * M + a)], xi = K[2 * (c * M + a) + 1], yr = K[2 * (c * M + b)], yi = K[2 * (c * M + b) + 1];
        er += xr * yr + xi * yi;
        ei += xr * yi - xi * yr;
      }
      w += er * rho[2 * (b * M + a)] - ei * rho[2 * (b * M + a) + 1];
    }
  return w;
}

// The selection rule (soft_measure's): the smallest i with u01 * W < w_0 + .. + w_i, W the sum of the weights in index order; the
// last i with w_i > 0 when none qualifies.  -1: W <= 0 or a weight that is not finite.
inline int chan_select(const double* w, uint32_t count, double u01, double* total) {
  double W = 0.0;
  for (uint32_t i = 0; i < count; ++i) {
    if (!std::isfinite(w[i])) return -1;
    W += w[i];
  }
  *total = W;
  if (!(W > 0.0) || !std::isfinite(W)) return -1;
  const double r = u01 * W;
  double cum = 0.0;
  int last = -1;
  for (uint32_t i = 0; i < count; ++i) {
    cum += w[i];
    if (r < cum) return (int)i;  // (not true at i - 1: w_i > 0)
    if (w[i] > 0.0) last = (int)i;
  }
  return last;
}

// Which steps run as ONE fused pass.  The two lists must cover at most kChanMaxUnion qubits; beyond that the choice is the
// measured one (tools/bench_noise.py, profiles/noise.md: the fused pass against a dense apply plus a density pass, n = 30 and 26):
//   Complex<f32> with |G| = 3   the fused pass forms 8 x 8 products and 64 sums in double for half the bytes: 1.11 .. 1.40 x the two
//                               calls at n = 26 for every position set and 1.08 .. 1.11 x at n = 30 on high positions (0.92 .. 0.98 x at
//                               n = 30 on low positions: given up for one rule per precision)
//   |G| <= 2, no position of G inside a wave row of 64 elements, n >= 28
//                               four scattered read and write streams per lane: 1.00 .. 1.01 x the two calls at n = 30 (0.76 .. 0.92 x
//                               at n = 26; only these two sizes are measured and the threshold sits between them)
// Those steps run composed.  `f32`: a Complex<f32> state; `packed`: its elements hold two amplitudes (position 0 is the half).
inline bool chan_fuses(uint32_t n, bool f32, bool packed, const std::vector<uint32_t>& apos, const std::vector<uint32_t>& bpos) {
  const ChanUnion u = chan_union(apos, bpos);
  if (u.g.size() > kChanMaxUnion) return false;
  if (f32 && u.g.size() == 3) return false;
  bool in_row = false;
  for (uint32_t p : u.g) in_row = in_row || p < 6u + (packed ? 1u : 0u);
  if (!in_row && u.g.size() <= 2 && n >= 28) return false;
  return true;
}

// The pass plan of a chain: one read-only density pass for the first channel; for every channel but the last one fused pass
// (apply it, reduce on the next one's qubits) where chan_fuses says so, else a dense apply and a density pass; a dense apply for
// the last.  pos[c]: channel c's positions.
struct ChanPlan {
  std::vector<uint8_t> fused;  // per channel but the last
  uint64_t passes = 0, nfused = 0;
};
inline ChanPlan chan_plan(uint32_t n, bool f32, bool packed, const std::vector<std::vector<uint32_t>>& pos) {
  ChanPlan p;
  if (pos.empty()) return p;
  p.passes = 2;
  for (size_t c = 0; c + 1 < pos.size(); ++c) {
    const bool f = chan_fuses(n, f32, packed, pos[c], pos[c + 1]);
    p.fused.push_back(f ? 1 : 0);
    p.passes += f ? 1 : 2;
    p.nfused += f ? 1 : 0;
  }
  return p;
}

}  // namespace qipk
