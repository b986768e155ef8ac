// qip_multiplex_plan.h — the host side of the multiplexed gate (qipx_state_apply_multiplexed, qipx_multiplexed_table_bytes of
// include/qip_hipx.h) that needs no device: where the select and target registers sit, how the vector is cut into wave walks, and
// the descriptor the kernel reads.  What qip_multiplex.hip adds is entry checks, the table and one launch (qip_multiplex_kernels.h).
//
// Plain C++17 as well as HIP, in the manner of qip_function_plan.h: no HIP types and no fail().  The index arithmetic of a walk
// (mx_* below) is compiled for both sides from this one text, so a stand-alone host program walks exactly what the kernel walks.
//
// |x>|t> -> |x> U_x|t>: an amplitude only mixes with the 2^k indices that share its x and its other bits (its GROUP).
//   row      index positions 0..5, the lane (2^n amplitudes below n = 6): loaded and stored as whole wave rows
//   H        a lane holds, per ITEM, the 2^kh amplitudes that differ in the kh target positions outside the row; target positions
//            inside the row are another lane's, fetched by a wave shuffle.  Either way every lane ends up with its whole group
//   item     one value of the OUTER positions: all that are neither the row's nor a target's outside it.  Item number w, bit i of w
//            at position opos[i]: the outer positions that are NOT select positions first, ascending, then the select positions,
//            ascending.  x is therefore constant over 2^nf consecutive items, nf = outer non-select positions
//   walk     a wave owns steps * U consecutive items (w = wave number * steps * U + t * U + u): U items are in flight per step.
//            U > 1 only when U <= 2^nf, so the U items of a step share x, and a lane re-fetches its matrix rows only at a step
//            whose x differs from the step before (mx_refetch): never, when steps * U <= 2^nf
//   x        = (bits fixed by the wave number) | (bits fixed by the walk step) | (bits of the lane)
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define QIP_MX_HD __host__ __device__ __forceinline__
#else
#define QIP_MX_HD inline
#endif

namespace qipk {

constexpr uint32_t kMxMaxK = 2;            // target qubits
constexpr uint32_t kMxMaxTableBits = 20;   // m + 2k: 2^20 entries = 16 MiB of Complex<f64>
constexpr uint32_t kMxLoads = 4;           // amplitudes of a lane in flight per step: U * H
constexpr uint32_t kMxWaves = 4;           // waves of a block (fewer when the state has fewer items)
constexpr uint32_t kMxMaxSteps = 8;        // walk steps of a wave, at most
constexpr uint32_t kMxFillBlocks = 256;    // a wave walks more than one step only once the launch has this many blocks
constexpr uint32_t kMxWalkBits = 5;        // log2(kMxMaxSteps * kMxLoads)
constexpr uint32_t kMxMaxOuter = 58;       // room for the outer positions: n <= 63 less the row's six

struct MxDesc {
  uint32_t rowlen;                 // amplitudes of a row: 64, or 2^n below n = 6
  uint32_t steps;                  // walk steps of a wave (a power of two)
  uint32_t lu;                     // log2 U
  uint32_t nwalk;                  // log2(steps * U): the low bits of the item number that the walk fills
  uint64_t woff[kMxWalkBits];      // 1 << (index position of walk bit i); 0 from i = nwalk on
  uint32_t wx[kMxWalkBits];        // the bit of x that walk bit i is (0: none)
  uint32_t nb;                     // bits of the wave number ...
  uint8_t bpos[kMxMaxOuter];       // ... the index position of bit i
  uint32_t nxb;                    // select bits fixed by the wave number ...
  uint8_t xpos[kMxMaxTableBits], xbit[kMxMaxTableBits];  // ... index position and bit number in x
  uint32_t lx[6];                  // the bit of x that lane bit b is (0: none)
  uint32_t la[6];                  // the bit of the matrix index that lane bit b is (0: none)
  uint64_t hoff[kMxMaxK];          // matrix-index bit i outside the row: 1 << its position; else 0
  uint32_t lsrc[kMxMaxK];          // matrix-index bit i inside the row: 1 << its position; else 0
  uint32_t lmask;                  // lsrc[0] | lsrc[1]
};

struct MxPlan {
  MxDesc d;
  uint32_t k = 0, m = 0;
  uint32_t hm = 0;        // matrix-index bits whose target sits outside the row (the kernel's HM)
  uint32_t H = 1, U = 1;  // amplitudes a lane holds per item; items per step
  uint32_t waves = 1;     // per block
  uint32_t threads = 64;
  uint64_t nwaves = 1, nblocks = 1;
  uint32_t nf = 0;        // outer positions that are not select positions
};

// the index (row bits zero, walk bits zero, target bits zero) of wave number wb
QIP_MX_HD uint64_t mx_wave_base(const MxDesc& d, uint64_t wb) {
  uint64_t base = 0;
  for (uint32_t i = 0; i < d.nb; ++i) base |= ((wb >> i) & 1ull) << d.bpos[i];
  return base;
}
// the bits of x that `base` fixes
QIP_MX_HD uint32_t mx_wave_x(const MxDesc& d, uint64_t base) {
  uint32_t x = 0;
  for (uint32_t j = 0; j < d.nxb; ++j) x |= (uint32_t)((base >> d.xpos[j]) & 1ull) << d.xbit[j];
  return x;
}
// walk item j = t * U + u of a wave: its index offset and its bits of x (every list walked to its full length with selects)
QIP_MX_HD uint64_t mx_walk_off(const MxDesc& d, uint32_t j) {
  uint64_t off = 0;
  for (uint32_t i = 0; i < kMxWalkBits; ++i) off |= ((j >> i) & 1u) ? d.woff[i] : 0ull;
  return off;
}
QIP_MX_HD uint32_t mx_walk_x(const MxDesc& d, uint32_t j) {
  uint32_t x = 0;
  for (uint32_t i = 0; i < kMxWalkBits; ++i) x |= ((j >> i) & 1u) ? d.wx[i] : 0u;
  return x;
}
// a lane re-fetches its matrix rows at step t: the first step, and every step whose x differs from the step before
QIP_MX_HD bool mx_refetch(const MxDesc& d, uint32_t t) {
  return t == 0u || mx_walk_x(d, t << d.lu) != mx_walk_x(d, (t - 1u) << d.lu);
}
QIP_MX_HD uint32_t mx_lane_x(const MxDesc& d, uint32_t lane) {
  uint32_t x = 0;
  for (uint32_t b = 0; b < 6; ++b) x |= ((lane >> b) & 1u) ? d.lx[b] : 0u;
  return x;
}
// the matrix-index bits of the lane's own amplitudes that the lane number fixes
QIP_MX_HD uint32_t mx_lane_a(const MxDesc& d, uint32_t lane) {
  uint32_t a = 0;
  for (uint32_t b = 0; b < 6; ++b) a |= ((lane >> b) & 1u) ? d.la[b] : 0u;
  return a;
}
// the lane of this lane's group that holds matrix index `a` (only the bits of `a` whose target is inside the row count)
QIP_MX_HD uint32_t mx_src_lane(const MxDesc& d, uint32_t lane, uint32_t a) {
  uint32_t src = lane & ~d.lmask;
  for (uint32_t i = 0; i < kMxMaxK; ++i) src |= ((a >> i) & 1u) ? d.lsrc[i] : 0u;
  return src;
}
// the index offset of the amplitude a lane holds for matrix index `a` (only the bits of `a` whose target is outside the row count)
QIP_MX_HD uint64_t mx_high_off(const MxDesc& d, uint32_t a) {
  uint64_t off = 0;
  for (uint32_t i = 0; i < kMxMaxK; ++i) off |= ((a >> i) & 1u) ? d.hoff[i] : 0ull;
  return off;
}

// spos[i] / tpos[i]: the index position of bit i of x / of the matrix index (distinct, below n; k = 1 or 2; m + 2k <= 20).
// fill_blocks: kMxFillBlocks for the library; a host test passes less to meet walks of several steps on small states.
inline MxPlan mx_plan(uint32_t n, const std::vector<uint32_t>& spos, const std::vector<uint32_t>& tpos,
                      uint32_t fill_blocks = kMxFillBlocks) {
  MxPlan P;
  MxDesc d = {};
  const uint32_t k = (uint32_t)tpos.size(), m = (uint32_t)spos.size();
  const uint32_t nrow = std::min<uint32_t>(n, 6u);
  d.rowlen = 1u << nrow;
  uint32_t kh = 0;
  for (uint32_t i = 0; i < k; ++i) {
    if (tpos[i] >= 6u) {
      d.hoff[i] = 1ull << tpos[i];
      P.hm |= 1u << i;
      ++kh;
    } else {
      d.lsrc[i] = 1u << tpos[i];
      d.lmask |= d.lsrc[i];
      d.la[tpos[i]] = 1u << i;
    }
  }
  auto xbit_of = [&](uint32_t pos) -> int {
    const auto it = std::find(spos.begin(), spos.end(), pos);
    return it == spos.end() ? -1 : (int)(it - spos.begin());
  };
  std::vector<uint32_t> free_pos, sel_pos;  // the outer positions, ascending: non-select, select
  for (uint32_t p = 6; p < n; ++p) {
    if (std::find(tpos.begin(), tpos.end(), p) != tpos.end()) continue;
    (xbit_of(p) < 0 ? free_pos : sel_pos).push_back(p);
  }
  for (uint32_t b = 0; b < nrow; ++b) {
    const int xb = xbit_of(b);
    if (xb >= 0) d.lx[b] = 1u << xb;
  }
  std::vector<uint32_t> opos = free_pos;
  opos.insert(opos.end(), sel_pos.begin(), sel_pos.end());
  const uint32_t no = (uint32_t)opos.size();
  const uint64_t items = 1ull << no;
  P.nf = (uint32_t)free_pos.size();
  P.H = 1u << kh;
  P.U = kMxLoads / P.H;
  if ((1ull << P.nf) < P.U) P.U = 1;  // the items of a step share x
  P.waves = (uint32_t)std::min<uint64_t>(kMxWaves, items / P.U);
  uint64_t steps = items / ((uint64_t)P.U * P.waves * fill_blocks);
  steps = std::max<uint64_t>(1, std::min<uint64_t>(kMxMaxSteps, steps));
  d.steps = (uint32_t)steps;
  for (d.lu = 0; (1u << d.lu) < P.U; ++d.lu) {}
  for (d.nwalk = d.lu; (1u << d.nwalk) < d.steps * P.U; ++d.nwalk) {}
  for (uint32_t i = 0; i < no; ++i) {
    const int xb = xbit_of(opos[i]);
    if (i < d.nwalk) {
      d.woff[i] = 1ull << opos[i];
      d.wx[i] = xb < 0 ? 0u : 1u << xb;
    } else {
      d.bpos[d.nb++] = (uint8_t)opos[i];
      if (xb >= 0) {
        d.xpos[d.nxb] = (uint8_t)opos[i];
        d.xbit[d.nxb++] = (uint8_t)xb;
      }
    }
  }
  P.nwaves = items >> d.nwalk;
  P.nblocks = P.nwaves / P.waves;
  P.threads = 64u * P.waves;
  P.k = k;
  P.m = m;
  P.d = d;
  return P;
}

}  // namespace qipk
