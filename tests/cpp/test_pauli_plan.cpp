// The host side of a Pauli-string pass (rustqip_amd/csrc/qip_pauli_plan.h) by brute force, without a GPU: the geometry of a pass,
// the transposed z masks against popcount parities at every work index, and the two planners.  Plain C++: the header alone.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "qip_pauli_plan.h"

using namespace qipk;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

static uint32_t parity(uint64_t v) { return (uint32_t)__builtin_popcountll(v) & 1u; }

// the amplitude index a kernel reaches from work index w: a zero inserted at hbit when paired, then the shift to amplitudes
static uint64_t index_of(const PauliGeom& g, uint64_t w) {
  if (g.pair) w = ((w >> g.hbit) << (g.hbit + 1)) | (w & ((1ull << g.hbit) - 1ull));
  return w << g.shift;
}

static void check_geometry(uint32_t n, bool packed, uint64_t x) {
  const PauliGeom g = pauli_geom(n, packed, x);
  const uint64_t span = (uint64_t)(g.pair ? 2 : 4) << kPauliStrideShift;
  CHECK(g.pair == (x != 0));
  CHECK(g.packed == (packed && n >= 2 && !(x & 1)));
  CHECK(g.shift == (g.packed ? 1u : 0u));
  CHECK(g.nwork == ((1ull << n) >> g.shift) >> (g.pair ? 1 : 0));
  CHECK(g.chunk >= 1 && (uint64_t)g.nblocks * g.chunk >= g.nwork && (uint64_t)(g.nblocks - 1) * g.chunk < g.nwork);
  CHECK(g.nblocks == 1 || g.chunk % span == 0);
  CHECK(g.nblocks <= 4096);
}

static const int kSlots[3] = {0, 5, 31};

static long check_masks(uint32_t n, bool packed, uint64_t x, uint64_t z) {
  const uint64_t full = (1ull << n) - 1;
  const PauliGeom g = pauli_geom(n, packed, x);
  // 32 terms of one x mask: the z under test in slots 0, 5 and 31, other masks in between; then the same through an index list
  std::vector<PauliTerm> terms(32), shuffled(32);
  std::vector<uint32_t> ids(32);
  for (uint32_t s = 0; s < 32; ++s) {
    terms[s] = PauliTerm{x, (z * (2 * s + 1) + s) & full, s & 3u};
    ids[s] = (s * 13 + 7) % 32;
  }
  for (int s : kSlots) terms[s].z = z;
  for (uint32_t s = 0; s < 32; ++s) shuffled[ids[s]] = terms[s];
  const PauliMasks m = pauli_masks(g, n, terms.data(), nullptr, 32);
  const PauliMasks ms = pauli_masks(g, n, shuffled.data(), ids.data(), 32);
  CHECK(m.x == x >> g.shift && m.count == 32 && ms.x == m.x && ms.count == 32 && ms.half == m.half);
  for (int b = 0; b < 64; ++b) CHECK(m.col[b] == ms.col[b]);
  const PauliMasks few = pauli_masks(g, n, terms.data(), nullptr, 6);  // slots past the count stay clear
  CHECK(few.count == 6 && (few.half >> 6) == 0);
  for (int b = 0; b < 64; ++b) CHECK((few.col[b] >> 6) == 0 && (few.col[b] & 63u) == (m.col[b] & 63u));
  std::vector<uint8_t> met((size_t)1 << n, 0);
  long checked = 0;
  for (uint64_t w = 0; w < g.nwork; ++w) {
    const uint64_t j = index_of(g, w);
    CHECK(j <= full);
    if (g.pair) CHECK((j ^ x) > j && (j ^ x) <= full);
    uint32_t word = 0;
    for (uint32_t b = 0; b < 64; ++b)
      if ((w >> b) & 1ull) word ^= m.col[b];
    for (uint32_t s = 0; s < 32; ++s) {
      CHECK(((word >> s) & 1u) == parity(j & terms[s].z));
      CHECK(((m.half >> s) & 1u) == ((g.packed && (terms[s].z & 1)) ? 1u : 0u));
      ++checked;
    }
    for (uint64_t half = 0; half <= g.shift; ++half) {
      ++met[j | half];
      if (g.pair) ++met[(j ^ x) | half];
    }
  }
  for (uint64_t a = 0; a <= full; ++a) CHECK(met[a] == 1);
  return checked;
}

static std::vector<PauliTerm> term_list(int which) {
  // x masks repeated and interleaved; z and n_Y tell the terms of one x mask apart
  static const uint64_t xs[3][12] = {{5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5},
                                     {3, 0, 3, 9, 0, 3, 3, 9, 9, 0, 3, 3},
                                     {8, 8, 1, 1, 1, 8, 0, 0, 8, 8, 8, 1}};
  std::vector<PauliTerm> terms;
  const int copies = which == 0 ? 4 : 3;  // 48 and 36 terms: runs longer than 32 of one x mask in list 0
  for (int c = 0; c < copies; ++c)
    for (int t = 0; t < 12; ++t) terms.push_back(PauliTerm{xs[which][t], (uint64_t)terms.size(), (uint32_t)t & 3u});
  if (which == 2) terms.resize(7);
  return terms;
}

static void check_planners(const std::vector<PauliTerm>& terms, uint32_t group) {
  std::vector<uint32_t> order;
  std::vector<PauliPass> passes;
  pauli_plan_sorted(terms, group, &order, &passes);
  CHECK(order.size() == terms.size());
  std::vector<int> seen(terms.size(), 0);
  size_t at = 0;
  for (size_t p = 0; p < passes.size(); ++p) {
    CHECK(passes[p].first == at && passes[p].count >= 1 && passes[p].count <= group);
    for (uint32_t s = 0; s < passes[p].count; ++s) {
      const uint32_t id = order[at + s];
      CHECK(id < terms.size() && terms[id].x == terms[order[at]].x);
      ++seen[id];
      if (s) CHECK(order[at + s - 1] < id);  // equal-x terms keep their input order
    }
    if (p + 1 < passes.size()) {
      const uint64_t xa = terms[order[at]].x, xb = terms[order[at + passes[p].count]].x;
      CHECK(xa <= xb);
      if (xa == xb) {
        CHECK(passes[p].count == group);  // all full except the last of one x
        CHECK(order[at + passes[p].count - 1] < order[at + passes[p].count]);
      }
    }
    at += passes[p].count;
  }
  CHECK(at == terms.size());
  for (int c : seen) CHECK(c == 1);

  pauli_plan_in_order(terms, group, &passes);
  at = 0;
  for (size_t p = 0; p < passes.size(); ++p) {
    CHECK(passes[p].first == at && passes[p].count >= 1 && passes[p].count <= group);  // concatenated: the identity order
    for (uint32_t s = 1; s < passes[p].count; ++s) CHECK(terms[at + s].x == terms[at].x);
    if (p + 1 < passes.size()) CHECK(terms[at].x != terms[at + passes[p].count].x || passes[p].count == group);
    at += passes[p].count;
  }
  CHECK(at == terms.size());
  if (terms.empty()) CHECK(passes.empty());
}

int main() {
  long checked = 0, geometries = 0;
  for (uint32_t n = 1; n <= 12; ++n) {
    const uint64_t full = (1ull << n) - 1, top = 1ull << (n - 1);
    const uint64_t xs[] = {0, 1, top, 1ull << (n / 2), full, 0xB5Aull & full & ~1ull, (top | (top >> 2) | 4) & full & ~1ull};
    const uint64_t zs[] = {0, full, 0x555ull & full, 0xA53ull & full, (top | 1) & full};
    for (int packed = 0; packed < 2; ++packed)
      for (uint64_t x : xs) {
        check_geometry(n, packed != 0, x);
        ++geometries;
        for (uint64_t z : zs) checked += check_masks(n, packed != 0, x, z);
      }
  }
  // n = 13 .. 30: the geometry alone (several blocks from n = 13 on); at n = 26, unpacked, a block holds at least two spans
  // (where the sign word is carried from span to span)
  for (uint32_t n = 13; n <= 30; ++n)
    for (int packed = 0; packed < 2; ++packed)
      for (uint64_t x : {0ull, 1ull, 1ull << (n - 1), 1ull << (n / 2), (1ull << n) - 1, 0x1812ull}) {
        check_geometry(n, packed != 0, x);
        ++geometries;
        const PauliGeom g = pauli_geom(n, packed != 0, x);
        if (n >= 16) CHECK(g.nblocks > 1);
        if (n == 26 && !g.packed) CHECK(g.chunk >= 2 * ((uint64_t)(g.pair ? 2 : 4) << kPauliStrideShift));
      }
  for (int which = 0; which < 3; ++which)
    for (uint32_t group : {1u, 2u, 16u, 32u}) check_planners(term_list(which), group);
  for (uint32_t group : {1u, 32u}) check_planners(std::vector<PauliTerm>(), group);
  std::printf("pauli plan ok: %ld geometries, %ld sign bits\n", geometries, checked);
  return 0;
}
