// qip_function_plan.h — the host side of the classical-function call (qipx_state_apply_function, qipx_function_passes of
// include/qip_hipx.h) that needs no device: where the two registers sit, how the out register is cut into passes, and the
// descriptor of each pass.  What qip_function.hip adds is entry checks, the table and one launch per pass
// (qip_function_kernels.h).
//
// Plain C++17 as well as HIP, in the manner of qip_diag_plan.h: no HIP types and no fail().
//
// |x>|y> -> w(x) |x>|y'>: an amplitude only moves among the 2^k indices that share its x and its other bits.  A tile made of
// the wave row (index positions 0..5) and the out register's positions outside it is therefore closed under the map: a block
// loads such tiles as whole rows, puts every amplitude at its destination slot in LDS and stores the rows back in place.
//   tile slot   bit b < 6 = index position b (the lane), bit 6 + t = the t-th of the tile's other positions, ascending
//   kt          tile rows = 2^kt: the pass's out positions outside the row, filled up with the lowest other positions to
//               min(n - 6, 5) so that a small out register still gives a block 2^11 amplitudes (the tile sweeps' tile); those
//               positions ride along unchanged
//   passes      an XOR acts on every out bit alone: out positions outside the row are taken kFnTileHigh at a time, ascending, one
//               pass each; the out bits inside the row and the phase go with the first.  An ADD carries across all of its bits and
//               needs them in ONE tile: more than kFnTileHigh outside the row are refused by the caller.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace qipk {

constexpr uint32_t kFnMaxIn = 24;    // 2^24 table entries
constexpr uint32_t kFnMaxOut = 32;   // a value is one 32-bit word on the device
constexpr uint32_t kFnTileHigh = 6;  // out positions outside the wave row per pass: 2^12 amplitudes = 64 KiB of Complex<f64>
constexpr uint32_t kFnFillHigh = 5;  // rows a tile is filled up to: 2^11 amplitudes
constexpr int kFnXor = 0, kFnAdd = 1, kFnPhaseOnly = 2;  // the kernel's MODE (the first two are the header's QIPX_FN_*)

struct FnDesc {
  uint32_t kt;          // tile row bits
  uint32_t rowlen;      // amplitudes of a row: 64, or 2^n below n = 6
  uint64_t hoff[kFnTileHigh];                   // 1 << (index position of tile row bit t); 0 from t = kt on
  uint32_t hx[kFnTileHigh], lx[6];              // the bit of x that row bit t / lane bit b is (0: none)
  uint32_t hy[kFnTileHigh], ly[6];              // ADD: the bit of y
  uint32_t nb;                                  // in-register bits outside the tile ...
  uint8_t bpos[kFnMaxIn], bbit[kFnMaxIn];       // ... index position and bit number in x
  uint32_t kmask, ymask;                        // ADD: 2^k - 1, and the tile-slot bits of y
  uint8_t yslot[6 + kFnTileHigh];               // ADD: tile-slot bit of bit i of y
};

struct FnPass {
  FnDesc d;
  std::vector<uint32_t> opened;  // the tile's row positions, ascending: what the block number does not fill (beside the row's)
  uint64_t ntiles = 0;
  uint32_t rows_per_wave = 0, threads = 0;
  int mode = kFnXor;
  bool phase = false;            // this pass multiplies by w(x)
  std::vector<uint32_t> vbit, vslot;  // XOR: bit vbit[i] of the value flips tile-slot bit vslot[i]
};

// XOR: the table word of a value in pass P, its bits spread over the tile's slot bits (destination slot = slot ^ word)
inline uint32_t fn_xor_word(const FnPass& P, uint64_t value) {
  uint32_t word = 0;
  for (size_t i = 0; i < P.vbit.size(); ++i) word |= (uint32_t)((value >> P.vbit[i]) & 1ull) << P.vslot[i];
  return word;
}

// ipos[i] / opos[i]: the index position of bit i of x / y (distinct, below n).  The out positions outside the wave row:
inline uint32_t fn_out_high(const std::vector<uint32_t>& opos) {
  return (uint32_t)std::count_if(opos.begin(), opos.end(), [](uint32_t p) { return p >= 6u; });
}
inline uint32_t fn_pass_count(const std::vector<uint32_t>& opos) {
  return std::max<uint32_t>(1u, (fn_out_high(opos) + kFnTileHigh - 1) / kFnTileHigh);
}

inline std::vector<FnPass> fn_plan(uint32_t n, const std::vector<uint32_t>& ipos, const std::vector<uint32_t>& opos, int mode,
                                   bool phases) {
  std::vector<uint32_t> high;
  for (uint32_t p : opos)
    if (p >= 6u) high.push_back(p);
  std::sort(high.begin(), high.end());
  const uint32_t npass = fn_pass_count(opos);
  std::vector<FnPass> plan(npass);
  for (uint32_t ps = 0; ps < npass; ++ps) {
    FnPass& P = plan[ps];
    std::vector<uint32_t> hp(high.begin() + std::min<size_t>(high.size(), (size_t)ps * kFnTileHigh),
                             high.begin() + std::min<size_t>(high.size(), (size_t)(ps + 1) * kFnTileHigh));
    const std::vector<uint32_t> own = hp;  // the out positions outside the row that this pass moves
    const uint32_t kt = n > 6u ? std::min<uint32_t>(n - 6u, std::max<uint32_t>((uint32_t)hp.size(), kFnFillHigh)) : 0u;
    for (uint32_t p = 6; p < n && hp.size() < kt; ++p)
      if (std::find(hp.begin(), hp.end(), p) == hp.end()) hp.push_back(p);
    std::sort(hp.begin(), hp.end());
    FnDesc d = {};
    d.kt = kt;
    d.rowlen = n >= 6u ? 64u : 1u << n;
    auto slot_of = [&](uint32_t pos) -> int {  // the tile-slot bit of an index position, -1 = outside the tile
      if (pos < 6u) return (int)pos;
      const auto it = std::find(hp.begin(), hp.end(), pos);
      return it == hp.end() ? -1 : 6 + (int)(it - hp.begin());
    };
    for (uint32_t t = 0; t < kt; ++t) d.hoff[t] = 1ull << hp[t];
    for (uint32_t i = 0; i < ipos.size(); ++i) {
      const int sl = slot_of(ipos[i]);
      if (sl < 0) {
        d.bpos[d.nb] = (uint8_t)ipos[i];
        d.bbit[d.nb++] = (uint8_t)i;
      } else if (sl < 6) {
        d.lx[sl] = 1u << i;
      } else {
        d.hx[sl - 6] = 1u << i;
      }
    }
    P.mode = opos.empty() ? kFnPhaseOnly : mode;
    P.phase = phases && ps == 0;
    for (uint32_t i = 0; i < opos.size(); ++i) {
      const bool mine = opos[i] < 6u ? ps == 0 : std::find(own.begin(), own.end(), opos[i]) != own.end();
      if (!mine) continue;
      const int sl = slot_of(opos[i]);
      if (P.mode == kFnAdd) {  // (one pass: every out bit is in the tile, and i < 6 + kFnTileHigh)
        d.yslot[i] = (uint8_t)sl;
        d.ymask |= 1u << sl;
        if (sl < 6) d.ly[sl] = 1u << i;
        else d.hy[sl - 6] = 1u << i;
      } else {
        P.vbit.push_back(i);
        P.vslot.push_back((uint32_t)sl);
      }
    }
    d.kmask = P.mode == kFnAdd ? (1u << opos.size()) - 1u : 0u;
    P.d = d;
    P.opened = hp;
    P.ntiles = n > 6u ? 1ull << (n - 6u - kt) : 1ull;
    P.rows_per_wave = std::min<uint32_t>(8u, 1u << kt);
    P.threads = 64u * ((1u << kt) / P.rows_per_wave);
  }
  return plan;
}

}  // namespace qipk
