// The multiplexed gate's plan (rustqip_amd/csrc/qip_multiplex_plan.h) without a device: for n = 1 .. 14, k = 1, 2 and a spread of
// register placements, walk every block, wave, step, item and lane as k_multiplex does (the same mx_* functions) and check against
// the definition: every index is loaded and stored exactly once; x is the select register's value of the index; the lane's matrix
// index a and the partners it gathers are its group in matrix-index order; a lane's x changes between two steps of its walk only
// where mx_refetch says its rows are fetched again; the items of one step share x.  Walks of several steps need 2^8 blocks in the
// library's plan, more than n = 14 gives: the plan is walked with that constant and with 1 and 4 in its place.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "qip_multiplex_plan.h"

using namespace qipk;

static int g_fail = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      if (++g_fail < 20) {                    \
        std::printf("FAIL %s: ", #cond);      \
        std::printf(__VA_ARGS__);             \
        std::printf("\n");                    \
      }                                       \
    }                                         \
  } while (0)

static uint32_t spread_hm(uint32_t hm, uint32_t c) { return hm == 3 ? c : hm == 2 ? c << 1 : hm == 1 ? c : 0u; }

static uint64_t g_cases = 0, g_refetch_walks = 0, g_multi = 0;

static void walk(uint32_t n, const std::vector<uint32_t>& spos, const std::vector<uint32_t>& tpos, uint32_t fill) {
  const MxPlan P = mx_plan(n, spos, tpos, fill);
  const MxDesc& d = P.d;
  const uint32_t k = (uint32_t)tpos.size(), M = 1u << k;
  const uint64_t N = 1ull << n;
  ++g_cases;
  CHECK(P.nblocks * P.waves == P.nwaves, "n=%u", n);
  CHECK(P.threads == 64u * P.waves && P.waves <= kMxWaves, "n=%u", n);
  CHECK(P.U * P.H <= kMxLoads, "n=%u", n);
  CHECK((1u << d.lu) == P.U && (1u << d.nwalk) == d.steps * P.U && d.nwalk <= kMxWalkBits, "n=%u", n);
  CHECK(d.steps == 1 || P.nblocks >= fill, "n=%u steps=%u blocks=%llu", n, d.steps, (unsigned long long)P.nblocks);
  if (P.nblocks > 1 && d.steps > 1) ++g_multi;
  uint64_t tmask = 0;
  for (uint32_t p : tpos) tmask |= 1ull << p;
  auto x_of = [&](uint64_t idx) {
    uint32_t x = 0;
    for (size_t i = 0; i < spos.size(); ++i) x |= (uint32_t)((idx >> spos[i]) & 1ull) << i;
    return x;
  };
  auto with_a = [&](uint64_t idx, uint32_t a) {
    idx &= ~tmask;
    for (uint32_t i = 0; i < k; ++i) idx |= (uint64_t)((a >> i) & 1u) << tpos[i];
    return idx;
  };
  std::vector<uint8_t> seen(N, 0);
  bool any_refetch = false;
  for (uint64_t blk = 0; blk < P.nblocks; ++blk) {
    for (uint32_t wave = 0; wave < P.waves; ++wave) {
      const uint64_t wb = blk * P.waves + wave;
      const uint64_t base = mx_wave_base(d, wb);
      const uint32_t xb = mx_wave_x(d, base);
      for (uint32_t lane = 0; lane < d.rowlen; ++lane) {
        const uint32_t xl = mx_lane_x(d, lane), al = mx_lane_a(d, lane);
        uint32_t x_rows = 0;  // the x the lane's rows were fetched for
        for (uint32_t t = 0; t < d.steps; ++t) {
          if (mx_refetch(d, t)) {
            x_rows = xb | mx_walk_x(d, t << d.lu) | xl;
            if (t > 0) any_refetch = true;
          }
          for (uint32_t u = 0; u < P.U; ++u) {
            const uint32_t j = (t << d.lu) | u;
            const uint64_t g = (base | mx_walk_off(d, j)) + lane;
            CHECK((xb | mx_walk_x(d, j) | xl) == x_rows, "n=%u t=%u u=%u: x moved without a re-fetch", n, t, u);
            for (uint32_t c = 0; c < P.H; ++c) {
              const uint32_t ah = spread_hm(P.hm, c);
              const uint64_t idx = g | mx_high_off(d, ah);
              CHECK(idx < N, "n=%u idx=%llu", n, (unsigned long long)idx);
              if (idx >= N) continue;
              ++seen[idx];
              CHECK(x_of(idx) == x_rows, "n=%u idx=%llu x=%u rows for %u", n, (unsigned long long)idx, x_of(idx), x_rows);
              const uint32_t a = ah | al;
              CHECK(with_a(idx, a) == idx, "n=%u idx=%llu a=%u", n, (unsigned long long)idx, a);
              for (uint32_t a2 = 0; a2 < M; ++a2) {  // v[a2]: the lane's own register for the high bits, from lane src
                const uint32_t src = mx_src_lane(d, lane, a2);
                CHECK(src < d.rowlen, "n=%u src=%u", n, src);
                const uint64_t partner = ((base | mx_walk_off(d, j)) + src) | mx_high_off(d, a2 & P.hm);
                CHECK(partner == with_a(idx, a2), "n=%u idx=%llu a2=%u partner=%llu", n, (unsigned long long)idx, a2,
                      (unsigned long long)partner);
              }
            }
          }
          if (t > 0 && !mx_refetch(d, t))
            CHECK(mx_walk_x(d, t << d.lu) == mx_walk_x(d, (t - 1) << d.lu), "n=%u t=%u", n, t);
        }
      }
    }
  }
  if (any_refetch) ++g_refetch_walks;
  for (uint64_t i = 0; i < N; ++i) CHECK(seen[i] == 1, "n=%u index %llu visited %u times", n, (unsigned long long)i, (unsigned)seen[i]);
  // re-fetches happen only when the walk reaches into the select positions
  if (d.nwalk <= P.nf) CHECK(!any_refetch, "n=%u nwalk=%u nf=%u", n, d.nwalk, P.nf);
}

int main() {
  std::mt19937 rng(20240611u);
  for (uint32_t n = 1; n <= 14; ++n) {
    for (uint32_t k = 1; k <= 2 && k <= n; ++k) {
      // fixed placements: registers at the low end, at the high end, across positions 5/6
      std::vector<std::vector<uint32_t>> orders;
      std::vector<uint32_t> asc(n), desc(n);
      for (uint32_t i = 0; i < n; ++i) asc[i] = i, desc[i] = n - 1 - i;
      orders.push_back(asc);
      orders.push_back(desc);
      if (n > 6) {
        std::vector<uint32_t> mid;
        for (uint32_t i = 0; i < n; ++i) mid.push_back((5 + i) % n);
        orders.push_back(mid);
        std::vector<uint32_t> mid2;
        for (uint32_t i = 0; i < n; ++i) mid2.push_back((6 + n - i) % n);
        orders.push_back(mid2);
      }
      for (int r = 0; r < 6; ++r) {
        std::vector<uint32_t> p = asc;
        std::shuffle(p.begin(), p.end(), rng);
        orders.push_back(p);
      }
      for (const auto& o : orders) {
        for (uint32_t m = 0; m + k <= n && m + 2 * k <= kMxMaxTableBits; m += (m < 3 || m + k + 1 >= n) ? 1 : 2) {
          // targets first in the order, then select; and select first, then targets
          std::vector<uint32_t> t1(o.begin(), o.begin() + k), s1(o.begin() + k, o.begin() + k + m);
          for (uint32_t fill : {kMxFillBlocks, 1u, 4u}) walk(n, s1, t1, fill);
          std::vector<uint32_t> s2(o.begin(), o.begin() + m), t2(o.begin() + m, o.begin() + m + k);
          for (uint32_t fill : {kMxFillBlocks, 1u, 4u}) walk(n, s2, t2, fill);
        }
      }
    }
  }
  CHECK(g_refetch_walks > 0, "no case re-fetched along a walk");
  CHECK(g_multi > 0, "no case with more than one block and more than one step");
  std::printf("%llu cases, %llu with a re-fetch along the walk, %llu with several blocks of several steps\n", (unsigned long long)g_cases,
              (unsigned long long)g_refetch_walks, (unsigned long long)g_multi);
  if (g_fail) {
    std::printf("%d failures\n", g_fail);
    return 1;
  }
  std::printf("multiplex plan ok\n");
  return 0;
}
