// The host side of qipx_state_apply_qft (rustqip_amd/csrc/qip_qft_plan.h) alone: for n = 1 .. 14, a spread of registers and all
// four flag combinations, a plain C++ walk over every block, thread, step and element that reads the pass descriptors the way
// k_qft_tile does (block base from the opened positions, LDS words through qft_lds_slot, the steps' element bits, integer twiddle
// exponents, the digit reversal of a one-pass natural-order call) runs the flow in long double and is compared with the direct
// DFT of every fibre.  It also holds every slot, table index and vector index to its bounds and every LDS word to one owner per
// step: what the kernel would touch outside its tile, its table or its vector fails here, on the host.
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>

#include "qip_qft_plan.h"

using namespace qipk;
using cld = std::complex<long double>;

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

static uint64_t gather(uint64_t j, const std::vector<uint32_t>& pos, uint32_t from, uint32_t to) {
  uint64_t v = 0;
  for (uint32_t i = from; i < to; ++i) v |= ((j >> pos[i]) & 1ull) << i;
  return v;
}

static cld twiddle(uint64_t t, uint32_t logn, int sign) {
  long double c, s;
  qft_twiddle<long double>(t, logn, sign, &c, &s);
  return cld(c, s);
}

// one pass of the flow on `st`, walked as the kernel walks it; pos = the register the flow runs on
static void run_pass(uint32_t n, const std::vector<uint32_t>& pos, const QftPass& P, std::vector<cld>& st) {
  const QftDesc& d = P.d;
  const uint64_t N = 1ull << n;
  const uint32_t E = d.ebits, NE = 1u << E, lg = d.tbits - E, L = d.hi - d.lo, slots = 1u << d.tbits;
  CHECK(E == 1 || E == 3);
  CHECK(d.tbits >= E && d.tbits <= kQftSlotBits && d.kt <= kQftTileHigh && P.threads == 1u << lg && P.threads <= 512);
  CHECK((P.ntiles << d.tbits) == N && L >= 1 && L <= kQftSlotBits && d.nsteps >= 1 && d.nsteps <= kQftMaxSteps);
  CHECK(P.table_entries == std::max(1u, 1u << (L - 1)));
  // (the product scales by the double d.scale; the model by the same number in long double, so that its bar can be 1e-16)
  const long double scale = std::ldexp((L & 1u) ? std::sqrt(0.5L) : 1.0L, -(int)(L / 2u));
  CHECK((double)scale == d.scale && d.unit == std::ldexp(1.0, 1 - (int)d.hi));
  std::vector<cld> tw(P.table_entries);
  for (uint32_t j = 0; j < P.table_entries; ++j) tw[j] = twiddle(j, L, d.sign);
  auto index_of = [&](uint64_t base, uint32_t slot) {
    uint64_t off = slot & 63u;
    for (uint32_t b = 6; b < d.tbits; ++b)
      if ((slot >> b) & 1u) off |= d.hoff[b - 6];
    return base | off;
  };
  auto v_of = [&](uint32_t slot) {
    uint32_t v = 0;
    for (uint32_t b = 0; b < kQftSlotBits; ++b)
      if ((slot >> b) & 1u) v |= d.vmap[b];
    return v;
  };
  std::vector<uint32_t> seen(N, 0);
  std::vector<cld> tile(slots);
  std::vector<uint32_t> owner(slots);
  for (uint64_t blk = 0; blk < P.ntiles; ++blk) {
    const uint64_t base = d.kt ? open_bits(blk << 6, P.opened) : 0ull;
    std::fill(owner.begin(), owner.end(), ~0u);
    for (uint32_t t = 0; t < P.threads; ++t)
      for (uint32_t j = 0; j < NE; ++j) {
        const uint32_t slot = t | (j << lg);
        const uint64_t g = index_of(base, slot);
        CHECK(slot < slots && g < N);
        if (g >= N) continue;
        CHECK(!seen[g]++);
        CHECK(v_of(slot) == (gather(g, pos, d.lo, d.hi) >> d.lo));
        const uint32_t w = qft_lds_slot(slot);
        CHECK(w < slots && owner[w] == ~0u);
        if (w < slots) tile[w] = st[g], owner[w] = t;
      }
    uint32_t done = L;
    for (uint32_t s = 0; s < d.nsteps; ++s) {
      const QftStep& sp = d.step[s];
      CHECK(sp.r >= 1 && sp.r <= E && sp.top == done - 1);
      done -= sp.r;
      for (uint32_t q = 0; q < sp.r; ++q) CHECK(sp.ebit[E - 1 - q] == d.vslot[sp.top - q]);
      std::fill(owner.begin(), owner.end(), ~0u);
      for (uint32_t t = 0; t < P.threads; ++t) {
        uint32_t b0 = t;
        for (uint32_t k = 0; k < E; ++k) {
          CHECK(sp.ins[k] < d.tbits && (k == 0 || sp.ins[k] > sp.ins[k - 1]));
          b0 = qft_open(b0, sp.ins[k]);
        }
        const uint32_t vb = v_of(b0);
        std::vector<cld> a(NE);
        std::vector<uint32_t> eo(NE, 0), ev(NE, 0);
        for (uint32_t e = 0; e < NE; ++e) {
          for (uint32_t k = 0; k < E; ++k)
            if ((e >> k) & 1u) eo[e] |= 1u << sp.ebit[k], ev[e] |= sp.evm[k];
          const uint32_t w = qft_lds_slot(b0 | eo[e]);
          CHECK((b0 & eo[e]) == 0 && w < slots && owner[w] == ~0u);
          CHECK((vb | ev[e]) == v_of(b0 | eo[e]));
          if (w >= slots) return;
          owner[w] = t;
          a[e] = tile[w];
        }
        for (uint32_t q = 0; q < sp.r; ++q) {
          const uint32_t k = E - 1 - q, j = sp.top - q, mask = (1u << j) - 1u, sh = L - 1u - j;
          for (uint32_t e = 0; e < NE; ++e) {
            if ((e >> k) & 1u) continue;
            const uint32_t e1 = e | (1u << k), ti = ((vb | ev[e]) & mask) << sh;
            CHECK(ti < P.table_entries);
            if (ti >= P.table_entries) return;
            const cld sum = a[e] + a[e1], dif = a[e] - a[e1];
            a[e] = sum;
            a[e1] = tw[ti] * dif;
          }
        }
        for (uint32_t e = 0; e < NE; ++e) tile[qft_lds_slot(b0 | eo[e])] = a[e];
      }
    }
    CHECK(done == 0);
    uint64_t xb = 0;
    for (uint32_t i = 0; i < d.nb; ++i) xb |= ((base >> d.bpos[i]) & 1ull) << d.bbit[i];
    for (uint32_t t = 0; t < P.threads; ++t)
      for (uint32_t j = 0; j < NE; ++j) {
        const uint32_t slot = t | (j << lg), v = v_of(slot);
        uint64_t xl = xb;
        for (uint32_t b = 0; b < kQftSlotBits; ++b)
          if ((slot >> b) & 1u) xl |= d.xmap[b];
        const uint64_t g = index_of(base, slot);
        CHECK(xl == gather(g, pos, 0, d.lo));
        const uint32_t kdig = qft_rev(v, L);
        uint32_t src = slot;
        if (d.natural) {
          CHECK(d.lo == 0);
          src = slot & ~d.vmask;
          for (uint32_t b = 0; b < kQftSlotBits; ++b) src |= ((kdig >> b) & 1u) << d.vslot[b];
        }
        CHECK(src < slots);
        cld x = tile[qft_lds_slot(src)];
        if (d.lo > 0) {
          const uint64_t tt = (uint64_t)kdig * xl;
          CHECK(tt < (1ull << d.hi));
          x *= twiddle(tt, d.hi, d.sign) * scale;
        } else {
          x *= scale;
        }
        st[g] = x;
      }
  }
  for (uint64_t g = 0; g < N; ++g) CHECK(seen[g] == 1);  // every index lies in exactly one tile of the pass
}

static void check_groups(const std::vector<uint32_t>& pos, const std::vector<QftPass>& plan, bool reversed) {
  const uint32_t m = (uint32_t)pos.size();
  CHECK(plan.size() == qft_tile_passes(pos));
  const uint32_t h = qft_high(pos), P = m ? std::max(1u, (h + 5u) / 6u) : 0u;
  CHECK(qft_tile_passes(pos) == P && qft_pass_count(pos, reversed) == ((reversed || P <= 1) ? P : P + 1));
  uint32_t hi = m;
  for (const QftPass& ps : plan) {  // contiguous from the top, at most six positions outside the row, cut only by a seventh
    CHECK(ps.d.hi == hi && ps.d.lo < hi);
    uint32_t out = 0;
    for (uint32_t i = ps.d.lo; i < ps.d.hi; ++i) out += pos[i] >= 6u;
    CHECK(out <= kQftTileHigh);
    if (ps.d.lo > 0) CHECK(out == kQftTileHigh && pos[ps.d.lo - 1] >= 6u);
    hi = ps.d.lo;
  }
  CHECK(hi == 0);
}

static void run_case(uint32_t n, const std::vector<uint32_t>& pos, uint32_t flags, std::mt19937_64& rng) {
  const uint32_t m = (uint32_t)pos.size();
  const uint64_t N = 1ull << n, M = 1ull << m;
  const bool inverse = flags & 1u, reversed = flags & 2u;
  const int sign = inverse ? -1 : 1;
  // a few entries per fibre, so that the direct DFT costs N * 3
  std::vector<cld> in(N, cld(0, 0));
  std::uniform_real_distribution<double> u(-1, 1);
  std::vector<std::vector<uint64_t>> support(N >> m);
  auto fibre_of = [&](uint64_t g) {
    uint64_t f = 0, bit = 0;
    for (uint32_t b = 0; b < n; ++b)
      if (std::find(pos.begin(), pos.end(), b) == pos.end()) f |= ((g >> b) & 1ull) << bit++;
    return f;
  };
  auto index_at = [&](uint64_t any, uint64_t x) {  // `any` with its register value replaced by x
    for (uint32_t i = 0; i < m; ++i) any = (any & ~(1ull << pos[i])) | (((x >> i) & 1ull) << pos[i]);
    return any;
  };
  for (uint64_t g = 0; g < N; ++g)
    if (gather(g, pos, 0, m) == 0)
      for (int e = 0; e < 3; ++e) {
        const uint64_t x = rng() & (M - 1);
        in[index_at(g, x)] = cld(u(rng), u(rng));
        support[fibre_of(g)].push_back(x);
      }
  // the definition: reversed | inverse reads its input in reversed order, reversed forward leaves its output in it
  std::vector<cld> want(N);
  const long double pi2 = 6.283185307179586476925286766559005768L;
  for (uint64_t g = 0; g < N; ++g) {
    uint64_t y = gather(g, pos, 0, m);
    if (reversed && !inverse) y = qft_rev((uint32_t)y, m);
    cld acc(0, 0);
    std::vector<uint64_t> xs = support[fibre_of(g)];
    std::sort(xs.begin(), xs.end());
    xs.erase(std::unique(xs.begin(), xs.end()), xs.end());
    for (uint64_t xs_i : xs) {
      const uint64_t x = (reversed && inverse) ? qft_rev((uint32_t)xs_i, m) : xs_i;  // the value the entry at xs_i stands for
      const uint64_t e = (x * y) & (M - 1);
      const long double ang = sign * pi2 * (long double)e / (long double)M;
      acc += cld(std::cos(ang), std::sin(ang)) * in[index_at(g, xs_i)];
    }
    want[g] = acc / std::sqrt((long double)M);
  }
  std::vector<uint32_t> flow = pos;
  if (inverse && reversed) std::reverse(flow.begin(), flow.end());
  const std::vector<QftPass> plan = qft_plan(n, flow, sign, !reversed);
  check_groups(flow, plan, reversed);
  std::vector<cld> cur = in;
  for (const QftPass& P : plan) {
    CHECK(P.d.natural == ((!reversed && plan.size() == 1) ? 1u : 0u));
    run_pass(n, flow, P, cur);
    if (failures) return;
  }
  if (!reversed && plan.size() > 1) {  // the closing sweep: destination bit pos[i] takes source bit pos[m-1-i]
    std::vector<cld> next(N);
    for (uint64_t g = 0; g < N; ++g) next[g] = cur[index_at(g, qft_rev((uint32_t)gather(g, pos, 0, m), m))];
    cur = next;
  }
  long double worst = 0;
  for (uint64_t g = 0; g < N; ++g) worst = std::max(worst, std::abs(cur[g] - want[g]));
  CHECK(worst < 1e-16L);
  if (!(worst < 1e-16L) && failures < 20) {
    printf("n=%u flags=%u worst=%Lg pos:", n, flags, worst);
    for (uint32_t p : pos) printf(" %u", p);
    printf("\n");
  }
}

int main(int argc, char**) {
  std::mt19937_64 rng(20240917);
  int cases = 0;
  if (argc > 1) {  // `test_qft_plan big`: the pass boundaries of the GPU tests at n = 19 and a walk at n = 15 (built without sanitizers by the test: seconds)
    std::vector<uint32_t> all(19), high12, high13, mixed15 = {6, 2, 7, 8, 9, 10, 11, 12, 13};
    std::iota(all.begin(), all.end(), 0u);
    for (uint32_t p = 6; p < 18; ++p) high12.push_back(p);
    for (uint32_t p = 6; p < 19; ++p) high13.push_back(p);
    for (uint32_t flags = 0; flags < 4; ++flags) {
      run_case(19, all, flags, rng);
      run_case(19, high12, flags, rng);
      run_case(19, high13, flags, rng);
      run_case(15, mixed15, flags, rng);
    }
    if (failures) printf("%d failures\n", failures);
    else printf("qft plan ok (big)\n");
    return failures ? 1 : 0;
  }
  for (uint32_t n = 1; n <= 14; ++n)
    for (int rep = 0; rep < 14; ++rep) {
      std::vector<uint32_t> pos(n);
      std::iota(pos.begin(), pos.end(), 0u);
      uint32_t m = 1 + (uint32_t)(rng() % n);
      if (rep == 0) m = n;                                   // the whole register, ascending
      else if (rep == 1) m = n, std::reverse(pos.begin(), pos.end());
      else if (rep == 2) m = std::min(n, 4u);                // inside the row
      else if (rep == 3) std::rotate(pos.begin(), pos.begin() + std::min(n - 1, 6u), pos.end()), m = std::max(1u, n - std::min(n - 1, 6u));  // outside it
      else std::shuffle(pos.begin(), pos.end(), rng);
      pos.resize(m);
      for (uint32_t flags = 0; flags < 4; ++flags) {
        run_case(n, pos, flags, rng);
        ++cases;
      }
    }
  // the pass counts the header states
  CHECK(qft_pass_count({}, false) == 0 && qft_pass_count({}, true) == 0);
  CHECK(qft_pass_count({0, 1, 2, 3, 4, 5}, false) == 1 && qft_pass_count({6, 7, 8, 9, 10, 11, 0, 3}, false) == 1);
  CHECK(qft_pass_count({6, 7, 8, 9, 10, 11, 12}, true) == 2 && qft_pass_count({6, 7, 8, 9, 10, 11, 12}, false) == 3);
  std::vector<uint32_t> all30(30);
  std::iota(all30.begin(), all30.end(), 0u);
  CHECK(qft_pass_count(all30, true) == 4 && qft_pass_count(all30, false) == 5);
  if (failures) {
    printf("%d failures\n", failures);
    return 1;
  }
  printf("qft plan ok (%d cases)\n", cases);
  return 0;
}
