// qip_diag_plan.h — the host side of the diagonal Pauli-sum calls (qipx_state_apply_diagonal, qipx_state_expect_diagonal of
// include/qip_hipx.h) that needs no device: the tile width, the split of every z mask at the tile boundary, the stable sort of
// the terms by their low mask into groups, the geometry of the one pass, and the host reference of the energy E^(j) in the stated
// order of operations.  What qip_pauli.hip adds is entry checks, the upload of the term table and two launches
// (qip_diag_kernels.h).
//
// Plain C++17 as well as HIP, in the manner of qip_pauli_plan.h: no HIP types and no fail(), so a stand-alone program
// (tests/test_diagonal_cpu.py) checks all of it by brute force.
//
// D(j) = sum_t k_t (-1)^popcount(j & z_t).  A tile is 2^L contiguous amplitudes, L = min(n, kDiagTileBits): j = (h << L) | l.
// With z_t = (zhi_t << L) | zlo_t,
//   D(h, l) = sum_m a_h[m] (-1)^popcount(l & m),      a_h[m] = sum_{t : zlo_t = m} k_t (-1)^popcount(h & zhi_t),
// the Walsh-Hadamard transform of a_h: T sign evaluations per tile, then L additions per amplitude.
//   E^(j)   a_h[m] = the sum of (+-)k_t over the terms of low mask m in the order of the call, starting from +0 (entries no term
//           names are +0); then L butterfly stages (u, v) -> (u + v, u - v) over index bit 0, 1, .., L - 1 IN THAT ORDER (v the
//           entry whose stage bit is set).  All in double.  A function of the terms, their order and j only: neither the
//           element packing nor the grid enters.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace qipk {

#ifndef QIP_DIAG_TILE_BITS
#define QIP_DIAG_TILE_BITS 12  // (a build-time switch for tools/bench_diagonal.py's comparison of 11, 12, 13 only)
#endif
constexpr uint32_t kDiagTileBits = QIP_DIAG_TILE_BITS;  // 4096 energies: 32 KiB of LDS (+ 2 KiB of padding), 16 per lane
static_assert(kDiagTileBits >= 9 && kDiagTileBits <= 13, "a lane owns 2^(kDiagTileBits - 8) entries of the table");
constexpr uint64_t kDiagMaxTerms = 1ull << 20;  // the cap of one call: a term table of 16 MiB + at most 8 MiB of group lists
constexpr uint32_t kDiagMaxBlocks = 4096;       // the grid's cap (pauli_geom's)
constexpr uint32_t kDiagBlock = 256;            // qip_kernels.h's kBlock (checked where both are seen: qip_diag_kernels.h)

struct DiagTerm {
  uint64_t zhi;  // the z mask above the tile boundary, shifted down: the sign of the term in tile h is (-1)^popcount(h & zhi)
  double k;
};
struct DiagPlan {
  uint32_t tile_bits = 0;             // L = min(n, kDiagTileBits)
  std::vector<DiagTerm> terms;        // sorted stably by low mask
  std::vector<uint32_t> order;        // terms[i] is the call's term order[i]
  std::vector<uint32_t> group_start;  // group g = terms[group_start[g] .. group_start[g + 1]): ngroups + 1 entries
  std::vector<uint32_t> group_mask;   // ... all of low mask group_mask[g]; ascending, distinct
};
// The one pass over 2^n amplitudes.  `packed`: a Complex<f32> state read in 16-byte elements of two amplitudes (the tile is the
// same 2^L amplitudes: 2^(L-1) elements).  A block takes `tiles_per_block` contiguous tiles.
struct DiagGeom {
  uint32_t tile_bits, shift;  // shift: 1 = two amplitudes per element
  uint64_t ntiles, tiles_per_block, tile_elems;
  uint32_t nblocks;
};

inline uint32_t diag_tile_bits(uint32_t n) { return std::min<uint32_t>(n, kDiagTileBits); }

// the terms (z masks over amplitude-index bits, k) of a call on n qubits, split and grouped
inline DiagPlan diag_plan(uint32_t n, const uint64_t* z, const double* k, size_t count) {
  DiagPlan p;
  p.tile_bits = diag_tile_bits(n);
  const uint64_t lomask = (1ull << p.tile_bits) - 1ull;
  p.order.resize(count);
  for (size_t t = 0; t < count; ++t) p.order[t] = (uint32_t)t;
  std::stable_sort(p.order.begin(), p.order.end(), [&](uint32_t a, uint32_t b) { return (z[a] & lomask) < (z[b] & lomask); });
  p.terms.resize(count);
  p.group_start.clear();
  p.group_mask.clear();
  for (size_t i = 0; i < count; ++i) {
    const uint64_t zt = z[p.order[i]];
    p.terms[i] = DiagTerm{zt >> p.tile_bits, k[p.order[i]]};
    if (i == 0 || (zt & lomask) != p.group_mask.back()) {
      p.group_start.push_back((uint32_t)i);
      p.group_mask.push_back((uint32_t)(zt & lomask));
    }
  }
  p.group_start.push_back((uint32_t)count);
  return p;
}

inline DiagGeom diag_geom(uint32_t n, bool packed_f32_elements) {
  DiagGeom g;
  g.tile_bits = diag_tile_bits(n);
  g.shift = packed_f32_elements ? 1u : 0u;  // (n >= 1: a tile is never half an element)
  g.ntiles = 1ull << (n - g.tile_bits);
  g.tile_elems = (1ull << g.tile_bits) >> g.shift;
  g.tiles_per_block = std::max<uint64_t>(g.ntiles / kDiagMaxBlocks, 1);
  g.nblocks = (uint32_t)((g.ntiles + g.tiles_per_block - 1) / g.tiles_per_block);
  return g;
}

// The longest chain of additions an addend of qipx_state_expect_diagonal's sums passes through: the lane's running sum (its
// amplitudes of a tile, tile after tile), the wave's tree (6), the block's four waves (4), the host's blocks.
inline uint64_t diag_chain_length(uint32_t n) {
  const DiagGeom g = diag_geom(n, false);
  const uint64_t per_lane = std::max<uint64_t>((1ull << g.tile_bits) / kDiagBlock, 1);
  return per_lane * g.tiles_per_block + 6 + 4 + g.nblocks;
}

inline uint32_t diag_parity(uint64_t v) {
  v ^= v >> 32, v ^= v >> 16, v ^= v >> 8, v ^= v >> 4, v ^= v >> 2, v ^= v >> 1;
  return (uint32_t)(v & 1ull);
}

// The host reference: out[l] = E^((h << L) | l) for the 2^L amplitudes of tile h, in the stated order of operations.
inline void diag_tile_energies(const DiagPlan& p, uint64_t h, double* out) {
  const size_t size = (size_t)1 << p.tile_bits;
  for (size_t i = 0; i < size; ++i) out[i] = 0.0;
  for (size_t g = 0; g < p.group_mask.size(); ++g) {
    double sum = 0.0;
    for (uint32_t t = p.group_start[g]; t < p.group_start[g + 1]; ++t)
      sum += diag_parity(h & p.terms[t].zhi) ? -p.terms[t].k : p.terms[t].k;
    out[p.group_mask[g]] = sum;
  }
  for (uint32_t s = 0; s < p.tile_bits; ++s)
    for (size_t i = 0; i < size; ++i)
      if (!((i >> s) & 1u)) {
        const double u = out[i], v = out[i | ((size_t)1 << s)];
        out[i] = u + v;
        out[i | ((size_t)1 << s)] = u - v;
      }
}

}  // namespace qipk
