// The host side of the diagonal Pauli-sum calls (rustqip_amd/csrc/qip_diag_plan.h) by brute force, without a GPU: the groups, the
// geometry of the pass and the host reference of the energy against the term-by-term sum.  Plain C++: the header alone.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "qip_diag_plan.h"

using namespace qipk;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() {  // xorshift64*
  g_rng ^= g_rng >> 12, g_rng ^= g_rng << 25, g_rng ^= g_rng >> 27;
  return g_rng * 0x2545F4914F6CDD1Dull;
}

static uint32_t parity(uint64_t v) { return (uint32_t)__builtin_popcountll(v) & 1u; }

// every amplitude belongs to exactly one row of one tile of one block
static void check_geometry(uint32_t n, bool packed) {
  const DiagGeom g = diag_geom(n, packed);
  CHECK(g.tile_bits == (n < kDiagTileBits ? n : kDiagTileBits));
  CHECK(g.shift == (packed ? 1u : 0u));
  CHECK(g.ntiles << g.tile_bits == 1ull << n);
  CHECK(g.tile_elems << g.shift == 1ull << g.tile_bits && g.tile_elems >= 1);
  CHECK(g.nblocks >= 1 && g.nblocks <= kDiagMaxBlocks);
  CHECK((uint64_t)g.nblocks * g.tiles_per_block >= g.ntiles && (uint64_t)(g.nblocks - 1) * g.tiles_per_block < g.ntiles);
  if (n > 16) return;
  std::vector<uint8_t> seen((size_t)1 << n, 0);
  for (uint32_t b = 0; b < g.nblocks; ++b) {
    const uint64_t first = (uint64_t)b * g.tiles_per_block;
    const uint64_t last = first + g.tiles_per_block < g.ntiles ? first + g.tiles_per_block : g.ntiles;
    for (uint64_t h = first; h < last; ++h)
      for (uint64_t row = 0; row * kDiagBlock < g.tile_elems; ++row)
        for (uint32_t lane = 0; lane < kDiagBlock; ++lane) {
          const uint64_t e = row * kDiagBlock + lane;  // the element of the tile this lane takes in this row
          if (e >= g.tile_elems) continue;
          for (uint64_t half = 0; half < (1ull << g.shift); ++half) {
            const uint64_t j = ((h * g.tile_elems + e) << g.shift) | half;
            CHECK(j < seen.size());
            seen[j] += 1;
          }
        }
  }
  for (uint8_t s : seen) CHECK(s == 1);
}

static void check_case(uint32_t n, const std::vector<uint64_t>& z, const std::vector<double>& k, bool dyadic) {
  const DiagPlan p = diag_plan(n, z.data(), k.data(), z.size());
  const uint32_t L = p.tile_bits;
  const uint64_t lomask = (1ull << L) - 1ull;
  // the groups partition the terms, ascending distinct masks, and keep the order of the call
  CHECK(p.terms.size() == z.size() && p.order.size() == z.size());
  CHECK(p.group_start.size() == p.group_mask.size() + 1);
  CHECK(p.group_start.front() == 0 && p.group_start.back() == z.size());
  std::vector<uint8_t> used(z.size(), 0);
  for (size_t g = 0; g < p.group_mask.size(); ++g) {
    CHECK(p.group_start[g] < p.group_start[g + 1]);
    if (g) CHECK(p.group_mask[g - 1] < p.group_mask[g]);
    for (uint32_t i = p.group_start[g]; i < p.group_start[g + 1]; ++i) {
      const uint32_t t = p.order[i];
      CHECK(t < z.size() && !used[t]);
      used[t] = 1;
      CHECK((z[t] & lomask) == p.group_mask[g] && (z[t] >> L) == p.terms[i].zhi && p.terms[i].k == k[t]);
      if (i > p.group_start[g]) CHECK(p.order[i - 1] < t);
    }
  }
  for (uint8_t u : used) CHECK(u == 1);
  // the host reference against the brute-force sum
  double weight = 0;
  for (double v : k) weight += std::fabs(v);
  std::vector<double> tile((size_t)1 << L);
  for (uint64_t h = 0; h < (1ull << (n - L)); ++h) {
    diag_tile_energies(p, h, tile.data());
    for (uint64_t l = 0; l <= lomask; ++l) {
      const uint64_t j = (h << L) | l;
      long double want = 0;
      for (size_t t = 0; t < z.size(); ++t) want += parity(j & z[t]) ? -(long double)k[t] : (long double)k[t];
      const double err = std::fabs((double)((long double)tile[l] - want));
      if (dyadic) CHECK(err == 0.0);
      else CHECK(err <= (double)(z.size() + L + 1) * 0x1p-53 * weight);
    }
  }
}

static void random_case(uint32_t n, size_t count, uint64_t keep_mask, uint32_t distinct_low_bits, bool dyadic) {
  std::vector<uint64_t> z(count);
  std::vector<double> k(count);
  for (size_t t = 0; t < count; ++t) {
    z[t] = next_u64() & ((1ull << n) - 1ull) & keep_mask;
    if (distinct_low_bits < 64) z[t] &= ((1ull << distinct_low_bits) - 1ull) | ~((1ull << kDiagTileBits) - 1ull);
    const int64_t r = (int64_t)(next_u64() % 2049) - 1024;
    k[t] = dyadic ? (double)r / 64.0 : (double)r / 1000.0 + 1e-3 * (double)(next_u64() % 1000) / 7.0;
  }
  if (count > 3) z[1] = z[0], z[count - 1] = z[0];  // repeated masks, apart
  if (count > 4) z[2] = 0;                          // the empty term
  check_case(n, z, k, dyadic);
}

int main() {
  for (uint32_t n = 1; n <= 30; ++n)
    for (int packed = 0; packed < 2; ++packed) check_geometry(n, packed != 0);
  CHECK(diag_chain_length(30) == 1024 + 6 + 4 + 4096);
  CHECK(diag_chain_length(13) == 16 + 6 + 4 + 2 && diag_chain_length(5) == 1 + 6 + 4 + 1);
  for (uint32_t n = 1; n <= 16; ++n) {
    const uint64_t below = (1ull << kDiagTileBits) - 1ull;
    for (int dyadic = 0; dyadic < 2; ++dyadic) {
      random_case(n, 1, ~0ull, 64, dyadic != 0);
      random_case(n, 40, ~0ull, 64, dyadic != 0);
      random_case(n, 40, below, 64, dyadic != 0);   // only below the tile boundary
      random_case(n, 40, ~below, 64, dyadic != 0);  // only above it: every term lands in a[0] (n <= kDiagTileBits: all empty)
      random_case(n, 30, ~0ull, 2, dyadic != 0);    // at most four low masks: long groups
    }
    if (n >= 10) random_case(n, 700, ~0ull, 64, true);  // more distinct low masks than the 256 lanes of a block
  }
  std::printf("diag plan ok\n");
  return 0;
}
