// qip_pauli_plan.h — the host side of a Pauli-string pass that needs no device: terms reduced to masks, the two planners, the
// geometry of a pass and the transposed z masks every Pauli kernel takes (qip_pauli_kernels.h), plus the slot capacities the
// options are held to (qip_core.hip).  What qip_pauli.hip adds is entry checks, descriptors' own tails and launches.
//
// Plain C++17 as well as HIP, in the manner of qip_tile_wire.h: no HIP types and no fail(), so a stand-alone program
// (tests/test_pauli_plan_cpu.py) checks all of it by brute force.
//   reduce  a term is (x mask, z mask, n_Y mod 4) over amplitude-index bits: P|j> = i^n_Y (-1)^popcount(j & z) |j ^ x>
//   plan    passes of at most `group` terms of ONE x mask: sorted stably by x (pauli_plan_sorted: the terms commute with the
//           sum they go into) or cut from runs of consecutive terms (pauli_plan_in_order: rotations do not commute)
//   pass    pauli_geom depends on n, the element packing and the class of the x mask only (zero / bit 0 set / bit 0 clear),
//           never on the group: with the kernels' per-slot arithmetic that makes a result a function of the state and its term
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace qipk {

// slots of one pass: the largest kernel capacity of each family
constexpr int kExpectMaxGroup = 32;
constexpr int kRotateMaxGroup = 32;
constexpr int kSumMaxGroup = 32;
constexpr int kMelemMaxGroup = 16;  // (two running sums per slot)

constexpr uint32_t kPauliStrideShift = 11;  // qip_kernels.h's kStrideShift (checked where both are seen: qip_pauli_kernels.h)

struct PauliTerm {
  uint64_t x, z;
  uint32_t ny;  // n_Y mod 4
};
struct PauliPass {
  uint32_t first, count;  // the terms order[first .. first + count) (in order: first .. first + count), all of one x mask
};
struct PauliGeom {
  bool pair, packed;
  uint64_t nwork, chunk;
  uint32_t nblocks, shift, hbit;  // shift: 1 = positions in 16-byte elements of two amplitudes; hbit: x's highest bit, in elements
};
// The head of every pass descriptor (ExpectDesc, RotateDesc, SumDesc, MelemDesc):
//   col   the z masks TRANSPOSED: bit g of col[b] = the amplitude-index bit behind WORK-index bit b lies under slot g's z mask
//   half  packed Complex<f32>: bit g = bit 0 of slot g's z mask, the sign the upper half of an element has on top of the lower's
struct PauliMasks {
  uint64_t x;      // the pass's x mask, in elements
  uint32_t count;  // slots in use
  uint32_t half;
  uint32_t col[64];
};

// the terms sorted by x mask, stably, each run of one x cut into passes of at most `group` terms
inline void pauli_plan_sorted(const std::vector<PauliTerm>& terms, uint32_t group, std::vector<uint32_t>* order,
                              std::vector<PauliPass>* passes) {
  order->resize(terms.size());
  for (size_t t = 0; t < terms.size(); ++t) (*order)[t] = (uint32_t)t;
  std::stable_sort(order->begin(), order->end(), [&](uint32_t a, uint32_t b) { return terms[a].x < terms[b].x; });
  passes->clear();
  for (size_t at = 0; at < order->size();) {
    size_t end = at;
    while (end < order->size() && terms[(*order)[end]].x == terms[(*order)[at]].x) ++end;
    for (; at < end; at += std::min<size_t>(group, end - at))
      passes->push_back(PauliPass{(uint32_t)at, (uint32_t)std::min<size_t>(group, end - at)});
  }
}

// maximal runs of CONSECUTIVE terms of one x mask, cut at `group` terms: the terms keep their order
inline void pauli_plan_in_order(const std::vector<PauliTerm>& terms, uint32_t group, std::vector<PauliPass>* passes) {
  passes->clear();
  for (size_t at = 0; at < terms.size();) {
    size_t end = at + 1;
    while (end < terms.size() && end - at < group && terms[end].x == terms[at].x) ++end;
    passes->push_back(PauliPass{(uint32_t)at, (uint32_t)(end - at)});
    at = end;
  }
}

inline uint32_t pauli_top_bit(uint64_t v) {
  uint32_t b = 0;
  while (v >>= 1) ++b;
  return b;
}

// The pass of x mask `x` over 2^n amplitudes.  x != 0: the pairs (j, j ^ x) with bit h of j clear, h = x's highest bit.
// `packed_f32_elements`: a Complex<f32> state read in 16-byte elements of two amplitudes, unless the pair differs in index bit 0
// (its halves would cross elements).  A block takes `chunk` contiguous work items: whole spans of a kernel's main loop, or all.
inline PauliGeom pauli_geom(uint32_t n, bool packed_f32_elements, uint64_t x) {
  PauliGeom g;
  g.pair = x != 0;
  g.packed = packed_f32_elements && n >= 2 && (x & 1ull) == 0;
  g.shift = g.packed ? 1u : 0u;
  g.hbit = g.pair ? pauli_top_bit(x) - g.shift : 0u;
  g.nwork = ((1ull << n) >> g.shift) >> (g.pair ? 1 : 0);
  const uint64_t span = (uint64_t)(g.pair ? 2 : 4) << kPauliStrideShift;  // one round of pauli_walk's main loop
  g.chunk = std::min<uint64_t>(std::max<uint64_t>(g.nwork / 4096, span), g.nwork);
  g.nblocks = (uint32_t)((g.nwork + g.chunk - 1) / g.chunk);
  return g;
}

// The descriptor head of one pass in geometry `g`: slot s holds terms[ids[s]] (ids == nullptr: terms[s]), all of one x mask.
inline PauliMasks pauli_masks(const PauliGeom& g, uint32_t n, const PauliTerm* terms, const uint32_t* ids, uint32_t count) {
  PauliMasks m = {};
  m.x = (count ? terms[ids ? ids[0] : 0].x : 0) >> g.shift;
  m.count = count;
  for (uint32_t slot = 0; slot < count; ++slot) {
    const uint64_t z = terms[ids ? ids[slot] : slot].z;
    if (g.packed && (z & 1ull)) m.half |= 1u << slot;
    for (uint32_t b = 0; b + g.shift + (g.pair ? 1 : 0) < n; ++b) {
      const uint32_t pos = (g.pair && b >= g.hbit ? b + 1 : b) + g.shift;  // the amplitude-index bit behind work-index bit b
      if ((z >> pos) & 1ull) m.col[b] |= 1u << slot;
    }
  }
  return m;
}

}  // namespace qipk
