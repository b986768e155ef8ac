// qip_qft_plan.h — the host side of the quantum Fourier transform of a register (qipx_state_apply_qft, qipx_qft_passes of
// include/qip_hipx.h) that needs no device: where the register sits, how its bits are cut into passes, the tile, the steps and
// the integer twiddle exponents of each pass.  What qip_qft.hip adds is entry checks, the twiddle tables and one launch per pass
// (qip_qft_kernels.h).
//
// Plain C++17 as well as HIP, in the manner of qip_function_plan.h: no HIP types and no fail().  The index helpers the kernel
// and the stand-alone host model (tests/cpp/test_qft_plan.cpp) share are QIP_QFT_HD.
//
// The flow is decimation in frequency from the register's most significant bit down.  With W_N = exp(sign 2 pi i / N), the
// stage on register bit i is the butterfly
//     (a, b) -> ((a + b) / sqrt2, (a - b) / sqrt2 * W_(2^(i+1))^(x mod 2^i))
// over the pairs that differ in bit i (x = the register value of a).  After the stages m-1 .. 0 the amplitude of output value y
// sits where the register reads rev_m(y): natural input gives bit-reversed output.
//   pass     a contiguous range [lo, hi) of register bits whose index positions fit one tile: the wave row (index positions
//            0..5) plus at most kQftTileHigh positions outside it.  Cut greedily from the top: a pass takes bits downward until
//            a seventh position outside the row would enter; register bits inside the row are free.  x mod 2^i splits into the
//            bits from lo up, which make the stage the one of a 2^(hi-lo)-point transform inside the tile (twiddle
//            W_(2^L)^(v << (L-1-j)), L = hi - lo, j = i - lo, v = the bits lo..i-1), and the bits below lo, whose factors of
//            all the pass's stages collect into ONE outer twiddle per amplitude after the pass, W_(2^hi)^(k * xlow): k = the
//            pass's output digit in natural order (the bit reversal of the bits lo..hi-1 where the amplitude sits), xlow = the
//            register value below lo.  k * xlow < 2^hi is formed exactly in 64-bit integers.
//   tile     slot bit b < 6 = index position b, slot bit 6 + t = the t-th of the tile's other positions, ascending; filled up
//            with the lowest other positions to min(n - 6, kQftFillHigh) row bits, as the function tiles are.  Below n = 6 the
//            tile is the whole vector.
//   step     a thread holds 2^E amplitudes (E = 3; 1 below n = 3) that differ in E slot bits and runs up to E stages on them in
//            registers; between steps the tile lives in LDS.  ebit[E-1] is the slot bit of the step's first (highest) stage; when
//            fewer than E stages are left the lowest element bits are bystanders (the highest free slot bits).
//   scale    2^(-L/2) once per pass, folded into the outer twiddle (one rounding for both).
//   orders   QIPX_QFT_REVERSED forward is the flow itself.  REVERSED | INVERSE is the flow with sign -1 on the REVERSED qubit
//            list (relabelling by the reversal R turns R F* into F* R).  Natural order in one pass reads the tile out of LDS
//            through the digit reversal; natural order in several passes closes with one bit-reversal sweep (the caller's).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#if defined(__HIPCC__)
#define QIP_QFT_HD __host__ __device__ __forceinline__
#else
#define QIP_QFT_HD inline
#endif

namespace qipk {

constexpr uint32_t kQftTileHigh = 6;   // register positions outside the wave row per pass: 2^12 amplitudes = 64 KiB of Complex<f64>
constexpr uint32_t kQftFillHigh = 5;   // row bits a tile is filled up to: 2^11 amplitudes
constexpr uint32_t kQftSlotBits = 6 + kQftTileHigh;
constexpr uint32_t kQftMaxSteps = 4;   // ceil(12 / 3)
constexpr uint32_t kQftMaxLow = 64;    // register bits below a pass that sit outside its tile

struct QftStep {
  uint32_t r;        // stages of this step, 1..E
  uint32_t top;      // j = i - lo of its first stage; the others follow downward
  uint32_t ins[3];   // the element slot bits, ascending (a thread's base slot opens them)
  uint32_t ebit[3];  // slot bit of element bit k
  uint32_t evm[3];   // vmap[ebit[k]]
};

struct QftDesc {
  uint32_t tbits;    // slot bits of the tile: min(n, 6) + kt
  uint32_t kt;       // tile row bits
  uint32_t ebits;    // E: a thread holds 2^E amplitudes
  uint32_t lo, hi;   // the pass's register bits
  uint32_t natural;  // 1: the only pass of a natural-order call, read out through the digit reversal
  int32_t sign;      // +1 forward, -1 inverse
  uint32_t nsteps;
  uint64_t hoff[kQftTileHigh];      // 1 << (index position of tile row bit t); 0 from t = kt on
  uint32_t vmap[kQftSlotBits];      // slot bit b holds register bit i in [lo, hi): 1 << (i - lo); else 0
  uint64_t xmap[kQftSlotBits];      // slot bit b holds register bit i < lo: 1 << i; else 0
  uint8_t vslot[kQftSlotBits];      // the slot bit of register bit lo + j
  uint32_t nb;                      // register bits below lo outside the tile ...
  uint8_t bpos[kQftMaxLow], bbit[kQftMaxLow];  // ... index position and register bit
  uint32_t vmask;                   // the slot bits with a vmap entry
  double scale;                     // 2^(-(hi - lo) / 2)
  double unit;                      // 2^(1 - hi): the outer twiddle is sincospi(k * xlow * unit)
  QftStep step[kQftMaxSteps];
};

struct QftPass {
  QftDesc d;
  std::vector<uint32_t> opened;  // the tile's row positions, ascending: what the block number does not fill (beside the row's)
  uint64_t ntiles = 0;
  uint32_t threads = 0;
  uint32_t table_entries = 0;    // W_(2^L)^j for j < max(1, 2^(L-1))
};

// the LDS word of a tile slot: bits 4..7 folded into bits 0..3, so that the 16 lanes of a bank group hit distinct banks both
// when they walk a row (slot bits 0..3) and when a step's element bits are low and the lanes walk the bits above them
QIP_QFT_HD uint32_t qft_lds_slot(uint32_t slot) { return slot ^ ((slot >> 4) & 15u); }
QIP_QFT_HD uint32_t qft_open(uint32_t w, uint32_t p) { return ((w >> p) << (p + 1u)) | (w & ((1u << p) - 1u)); }
QIP_QFT_HD uint32_t qft_rev(uint32_t v, uint32_t bits) {  // the low `bits` bits of v in reversed order
  uint32_t r = 0;
  for (uint32_t b = 0; b < bits; ++b) r |= ((v >> b) & 1u) << (bits - 1u - b);
  return r;
}

// the register positions outside the wave row
inline uint32_t qft_high(const std::vector<uint32_t>& pos) {
  return (uint32_t)std::count_if(pos.begin(), pos.end(), [](uint32_t p) { return p >= 6u; });
}
// the tile passes, and all passes of a call (the closing bit-reversal sweep of a natural-order call of several passes included)
inline uint32_t qft_tile_passes(const std::vector<uint32_t>& pos) {
  return pos.empty() ? 0u : std::max<uint32_t>(1u, (qft_high(pos) + kQftTileHigh - 1) / kQftTileHigh);
}
inline uint32_t qft_pass_count(const std::vector<uint32_t>& pos, bool reversed) {
  const uint32_t p = qft_tile_passes(pos);
  return (reversed || p <= 1u) ? p : p + 1u;
}

// W_(2^logn)^t = (c, s) for sign = +1, (c, -s) for sign = -1, from the exact integer exponent: t is reduced to an octant in
// integers, the angle left is at most pi / 4, and cos / sin are the real type's own (double on the product path, long double in
// the host model)
template <typename R>
inline void qft_twiddle(uint64_t t, uint32_t logn, int sign, R* c, R* s) {
  if (logn < 3u) {
    t <<= 3u - logn;
    logn = 3u;
  }
  const uint64_t n = 1ull << logn, quarter = n >> 2;
  t &= n - 1ull;
  const uint64_t quad = t / quarter, r = t % quarter;
  const R pi = (R)3.14159265358979323846264338327950288L;
  R c0, s0;
  if (r <= quarter / 2) {
    const R a = pi * (R)r / (R)(n >> 1);
    c0 = std::cos(a), s0 = std::sin(a);
  } else {
    const R a = pi * (R)(quarter - r) / (R)(n >> 1);
    c0 = std::sin(a), s0 = std::cos(a);
  }
  R cc, ss;
  switch (quad) {
    case 0: cc = c0, ss = s0; break;
    case 1: cc = -s0, ss = c0; break;
    case 2: cc = -c0, ss = -s0; break;
    default: cc = s0, ss = -c0; break;
  }
  *c = cc;
  *s = sign < 0 ? -ss : ss;
}

// pos[i] = the index position of register bit i (distinct, below n), already in the order the flow runs on (the caller has
// reversed it for REVERSED | INVERSE); natural = the caller wants natural order
inline std::vector<QftPass> qft_plan(uint32_t n, const std::vector<uint32_t>& pos, int sign, bool natural) {
  const uint32_t m = (uint32_t)pos.size();
  std::vector<QftPass> plan;
  if (m == 0) return plan;
  const uint32_t npass = qft_tile_passes(pos);
  const uint32_t lowbits = std::min<uint32_t>(n, 6u);
  uint32_t hi = m;
  while (hi > 0) {
    uint32_t lo = hi, nhigh = 0;
    while (lo > 0) {
      const bool outside = pos[lo - 1] >= 6u;
      if (outside && nhigh == kQftTileHigh) break;
      nhigh += outside;
      --lo;
    }
    QftPass P;
    QftDesc d = {};
    std::vector<uint32_t> hp;
    for (uint32_t i = lo; i < hi; ++i)
      if (pos[i] >= 6u) hp.push_back(pos[i]);
    const uint32_t kt = n > 6u ? std::min<uint32_t>(n - 6u, std::max<uint32_t>((uint32_t)hp.size(), kQftFillHigh)) : 0u;
    for (uint32_t p = 6; p < n && hp.size() < kt; ++p)
      if (std::find(hp.begin(), hp.end(), p) == hp.end()) hp.push_back(p);
    std::sort(hp.begin(), hp.end());
    d.kt = kt;
    d.tbits = lowbits + kt;
    d.ebits = d.tbits >= 3u ? 3u : 1u;
    d.lo = lo;
    d.hi = hi;
    d.sign = sign;
    d.natural = (natural && npass == 1u) ? 1u : 0u;
    // (a power of two for an even count; else the rounded 1 / sqrt2 times one)
    d.scale = std::ldexp(((hi - lo) & 1u) ? 0.70710678118654752440 : 1.0, -(int)((hi - lo) / 2u));
    d.unit = std::ldexp(1.0, 1 - (int)hi);
    auto slot_of = [&](uint32_t p) -> int {  // the tile-slot bit of an index position, -1 = outside the tile
      if (p < 6u) return (int)p;
      const auto it = std::find(hp.begin(), hp.end(), p);
      return it == hp.end() ? -1 : 6 + (int)(it - hp.begin());
    };
    for (uint32_t t = 0; t < kt; ++t) d.hoff[t] = 1ull << hp[t];
    for (uint32_t i = 0; i < hi; ++i) {
      const int sl = slot_of(pos[i]);
      if (i >= lo) {  // (every bit of the pass is in the tile)
        d.vmap[sl] = 1u << (i - lo);
        d.vmask |= 1u << sl;
        d.vslot[i - lo] = (uint8_t)sl;
      } else if (sl >= 0) {
        d.xmap[sl] = 1ull << i;
      } else {
        d.bpos[d.nb] = (uint8_t)pos[i];
        d.bbit[d.nb++] = (uint8_t)i;
      }
    }
    const uint32_t E = d.ebits, L = hi - lo;
    for (uint32_t j = L; j > 0;) {
      QftStep& st = d.step[d.nsteps++];
      st.r = std::min<uint32_t>(E, j);
      st.top = j - 1u;
      uint32_t used = 0;
      for (uint32_t q = 0; q < st.r; ++q) {
        st.ebit[E - 1u - q] = d.vslot[j - 1u - q];
        used |= 1u << d.vslot[j - 1u - q];
      }
      uint32_t fill = d.tbits;
      for (uint32_t q = st.r; q < E; ++q) {  // bystander element bits: the highest free slot bits
        do --fill; while ((used >> fill) & 1u);
        st.ebit[E - 1u - q] = fill;
        used |= 1u << fill;
      }
      for (uint32_t k = 0; k < E; ++k) st.ins[k] = st.ebit[k], st.evm[k] = d.vmap[st.ebit[k]];
      std::sort(st.ins, st.ins + E);
      j -= st.r;
    }
    P.d = d;
    P.opened = hp;
    P.ntiles = n > 6u ? 1ull << (n - 6u - kt) : 1ull;
    P.threads = 1u << (d.tbits - E);
    P.table_entries = L >= 1u ? std::max<uint32_t>(1u, 1u << (L - 1u)) : 1u;
    plan.push_back(P);
    hi = lo;
  }
  return plan;
}

}  // namespace qipk
