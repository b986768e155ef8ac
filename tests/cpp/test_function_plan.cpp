// The host side of qipx_state_apply_function (rustqip_amd/csrc/qip_function_plan.h) alone, by brute force: for n = 1 .. 14, both
// modes and random register placements, a plain C++ walk over every block, wave, row and lane that reads the pass descriptors the
// way k_function_tile does (block base from the opened positions, x and y from the short lists, the destination slot from the
// table word) is compared with the definition new[j with y -> y'] = old[j].  It also holds every slot and every index to its
// bounds: what the kernel would write outside its tile or its vector fails here, on the host.
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>

#include "qip_function_plan.h"

using namespace qipk;

static int failures = 0;
#define CHECK(c)                                                 \
  do {                                                           \
    if (!(c)) {                                                  \
      if (++failures < 20) printf("line %d: %s\n", __LINE__, #c); \
    }                                                            \
  } while (0)

static uint64_t open_bits(uint64_t w, const std::vector<uint32_t>& pos) {  // insert_bits of qip_kernels.h (ascending positions)
  for (uint32_t p : pos) w = ((w >> p) << (p + 1)) | (w & ((1ull << p) - 1ull));
  return w;
}

static uint64_t gather(uint64_t j, const std::vector<uint32_t>& pos) {
  uint64_t v = 0;
  for (size_t i = 0; i < pos.size(); ++i) v |= ((j >> pos[i]) & 1ull) << i;
  return v;
}

static void run_case(uint32_t n, const std::vector<uint32_t>& ipos, const std::vector<uint32_t>& opos, int mode, std::mt19937_64& rng) {
  const uint32_t m = (uint32_t)ipos.size(), k = (uint32_t)opos.size();
  const uint64_t N = 1ull << n, kmask = (1ull << k) - 1ull;
  std::vector<uint64_t> values(1ull << m);
  for (auto& v : values) v = rng() & kmask;
  // the definition
  std::vector<uint64_t> want(N), cur(N), next(N);
  for (uint64_t j = 0; j < N; ++j) {
    const uint64_t x = gather(j, ipos), y = gather(j, opos);
    const uint64_t y2 = mode == kFnAdd ? (y + values[x]) & kmask : y ^ values[x];
    uint64_t to = j;
    for (uint32_t i = 0; i < k; ++i) to = (to & ~(1ull << opos[i])) | (((y2 >> i) & 1ull) << opos[i]);
    want[to] = j;
  }
  std::iota(cur.begin(), cur.end(), 0ull);  // amplitude j carries its own index
  const std::vector<FnPass> plan = fn_plan(n, ipos, opos, mode, false);
  CHECK(plan.size() == fn_pass_count(opos));
  for (const FnPass& P : plan) {
    const FnDesc& d = P.d;
    const uint32_t rows = 1u << d.kt, nw = P.threads / 64;
    CHECK(P.rows_per_wave * nw == rows && P.threads <= 512 && P.threads % 64 == 0);
    CHECK(d.kt <= kFnTileHigh && (P.ntiles << (d.kt + (n >= 6 ? 6 : n))) == N);
    std::vector<uint64_t> tile((size_t)64 << d.kt), seen(N, 0);
    for (uint64_t blk = 0; blk < P.ntiles; ++blk) {
      const uint64_t base = open_bits(blk << 6, P.opened);
      uint32_t xb = 0;
      for (uint32_t j = 0; j < d.nb; ++j) xb |= (uint32_t)((base >> d.bpos[j]) & 1ull) << d.bbit[j];
      std::fill(tile.begin(), tile.end(), ~0ull);
      for (int store = 0; store < 2; ++store)
        for (uint32_t wave = 0; wave < nw; ++wave)
          for (uint32_t i = 0; i < P.rows_per_wave; ++i)
            for (uint32_t lane = 0; lane < d.rowlen; ++lane) {
              const uint32_t r = i * nw + wave;
              uint64_t off = 0;
              uint32_t xr = 0, yr = 0, xl = 0, yl = 0;
              for (uint32_t t = 0; t < kFnTileHigh; ++t)
                if ((r >> t) & 1u) off |= d.hoff[t], xr |= d.hx[t], yr |= d.hy[t];
              for (uint32_t b = 0; b < 6; ++b)
                if ((lane >> b) & 1u) xl |= d.lx[b], yl |= d.ly[b];
              const uint64_t g = (base | off) + lane;
              CHECK(g < N);
              const uint32_t x = xb | xr | xl;
              CHECK(x == gather(g, ipos));
              const uint32_t slot = (r << 6) | lane;
              if (store) {
                CHECK(tile[slot] != ~0ull);
                next[g] = tile[slot];
                continue;
              }
              CHECK(!seen[g]++);
              uint32_t to = slot;
              if (P.mode == kFnXor) {
                to = slot ^ fn_xor_word(P, values[x]);
              } else if (P.mode == kFnAdd) {
                const uint32_t y = ((yr | yl) + (uint32_t)values[x]) & d.kmask;
                to = slot & ~d.ymask;
                for (uint32_t b = 0; b < 6 + kFnTileHigh; ++b) to |= ((y >> b) & 1u) << d.yslot[b];
              }
              CHECK(to < tile.size() && tile[to] == ~0ull);
              if (to < tile.size()) tile[to] = cur[g];
            }
    }
    cur = next;
  }
  for (uint64_t j = 0; j < N; ++j) CHECK(cur[j] == want[j]);
}

int main() {
  std::mt19937_64 rng(20240611);
  int cases = 0;
  for (uint32_t n = 1; n <= 14; ++n)
    for (int rep = 0; rep < 40; ++rep) {
      std::vector<uint32_t> pos(n);
      std::iota(pos.begin(), pos.end(), 0u);
      std::shuffle(pos.begin(), pos.end(), rng);
      const uint32_t m = (uint32_t)(rng() % (std::min<uint32_t>(n, 8u) + 1));
      const uint32_t k = (uint32_t)(rng() % (n - m + 1));
      const std::vector<uint32_t> ipos(pos.begin(), pos.begin() + m), opos(pos.begin() + m, pos.begin() + m + k);
      for (int mode : {kFnXor, kFnAdd}) {
        if (mode == kFnAdd && fn_out_high(opos) > kFnTileHigh) continue;
        run_case(n, ipos, opos, mode, rng);
        ++cases;
      }
    }
  // the pass counts the header states: six out positions outside the row are one pass, seven are two; those inside do not count
  CHECK(fn_pass_count({6, 7, 8, 9, 10, 11}) == 1 && fn_pass_count({6, 7, 8, 9, 10, 11, 12}) == 2);
  CHECK(fn_pass_count({0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}) == 1 && fn_pass_count({}) == 1 && fn_pass_count({3}) == 1);
  run_case(16, {15, 14, 13}, {6, 7, 8, 9, 10, 11, 12, 0, 3}, kFnXor, rng);  // two passes, the second of one own position
  if (failures) {
    printf("%d failures\n", failures);
    return 1;
  }
  printf("function plan ok (%d cases)\n", cases + 1);
  return 0;
}
