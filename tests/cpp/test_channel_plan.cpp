// The host-only plan of the noise-channel calls (rustqip_amd/csrc/qip_channel_plan.h) against brute force at n = 5: for every
// ordered list of k = 1, 2 qubits acted on and k2 = 1, 2 qubits reduced next that cover at most three qubits together — equal,
// nested, overlapping and disjoint lists, in every order — the union G, the operator expanded to G applied group by group as the
// kernel does, the density matrix on G traced down to the next qubits and permuted to the caller's order are compared with the
// definitions on the full vector.  Plain C++17: no device, no HIP.
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "qip_channel_plan.h"

using namespace qipk;
using cd = std::complex<double>;

static int failures = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      ++failures;                   \
      printf("FAILED %s: ", #cond); \
      printf(__VA_ARGS__);          \
      printf("\n");                 \
    }                               \
  } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (double)(rng_state >> 11) / 9007199254740992.0 - 0.5;
}

// bit i of the sub-index = bit pos[i] of j
static uint32_t sub_index(uint32_t j, const std::vector<uint32_t>& pos) {
  uint32_t a = 0;
  for (size_t i = 0; i < pos.size(); ++i) a |= ((j >> pos[i]) & 1u) << i;
  return a;
}
static uint32_t with_sub(uint32_t j, const std::vector<uint32_t>& pos, uint32_t a) {
  for (size_t i = 0; i < pos.size(); ++i) j = (j & ~(1u << pos[i])) | (((a >> i) & 1u) << pos[i]);
  return j;
}

static void one_case(uint32_t n, const std::vector<uint64_t>& aq, const std::vector<uint64_t>& bq, int kind) {
  const uint32_t k = (uint32_t)aq.size(), k2 = (uint32_t)bq.size(), dim = 1u << n, MA = 1u << k, MB = 1u << k2;
  std::vector<uint32_t> apos, bpos;
  CHECK(chan_check_indices(n, aq.data(), k, &apos).empty(), "indices refused");
  CHECK(chan_check_indices(n, bq.data(), k2, &bpos).empty(), "next refused");
  for (uint32_t i = 0; i < k; ++i) CHECK(apos[i] == n - 1 - aq[i], "position");
  std::vector<cd> x(dim), A(MA * MA);
  for (auto& v : x) v = cd(rnd(), rnd());
  for (uint32_t r = 0; r < MA; ++r)
    for (uint32_t c = 0; c < MA; ++c) {
      cd v(rnd(), rnd());
      if (kind == 1) v = r == c ? v : cd(0, 0);                  // diagonal
      if (kind == 2) v = r == 0 ? cd(0, 0) : v;                  // a zero row
      if (kind == 3) v = r == c ? cd(1, 0) : cd(0, 0);           // the identity
      A[r * MA + c] = v;
    }
  // the definitions
  std::vector<cd> y(dim, cd(0, 0));
  for (uint32_t j = 0; j < dim; ++j)
    for (uint32_t c = 0; c < MA; ++c) y[j] += A[sub_index(j, apos) * MA + c] * x[with_sub(j, apos, c)];
  std::vector<cd> want(MB * MB, cd(0, 0));
  for (uint32_t j = 0; j < dim; ++j)
    for (uint32_t b2 = 0; b2 < MB; ++b2) want[sub_index(j, bpos) * MB + b2] += y[j] * std::conj(y[with_sub(j, bpos, b2)]);
  // the plan
  const ChanUnion u = chan_union(apos, bpos);
  const uint32_t kg = (uint32_t)u.g.size(), M = 1u << kg;
  CHECK(kg == chan_union_size(apos, bpos) && kg <= kChanMaxUnion, "union size %u", kg);
  for (uint32_t j = 1; j < kg; ++j) CHECK(u.g[j - 1] < u.g[j], "G is not ascending");
  for (uint32_t i = 0; i < k; ++i) CHECK(u.g[u.abit[i]] == apos[i], "abit");
  for (uint32_t i = 0; i < k2; ++i) CHECK(u.g[u.bbit[i]] == bpos[i], "bbit");
  std::vector<double> w(2 * M * M);
  uint32_t nzr[8], nzi[8];
  bool diag = false;
  chan_expand(u, k, reinterpret_cast<const double*>(A.data()), 1.0, w.data(), nzr, nzi, &diag);
  CHECK(diag == (kind == 1 || kind == 3), "diag flag %d for kind %d", (int)diag, kind);
  for (uint32_t g = 0; g < M; ++g)
    for (uint32_t g2 = 0; g2 < M; ++g2) {
      CHECK(((nzr[g] >> g2) & 1u) == (w[2 * (g * M + g2)] != 0.0 ? 1u : 0u), "nzr");
      CHECK(((nzi[g] >> g2) & 1u) == (w[2 * (g * M + g2) + 1] != 0.0 ? 1u : 0u), "nzi");
    }
  if (kind == 3)
    for (uint32_t g = 0; g < M; ++g) CHECK(nzr[g] == (1u << g) && nzi[g] == 0, "the identity expands to the identity");
  // group by group, as the kernel: every index whose G bits are zero is the base of one group
  std::vector<cd> got(dim, cd(0, 0));
  std::vector<cd> rhoG(M * M, cd(0, 0));
  for (uint32_t base = 0; base < dim; ++base) {
    if (sub_index(base, u.g) != 0) continue;
    std::vector<cd> xg(M), yg(M, cd(0, 0));
    for (uint32_t g = 0; g < M; ++g) xg[g] = x[with_sub(base, u.g, g)];
    for (uint32_t g = 0; g < M; ++g)
      for (uint32_t g2 = 0; g2 < M; ++g2) yg[g] += cd(w[2 * (g * M + g2)], w[2 * (g * M + g2) + 1]) * xg[g2];
    for (uint32_t g = 0; g < M; ++g) got[with_sub(base, u.g, g)] = yg[g];
    for (uint32_t g = 0; g < M; ++g)
      for (uint32_t g2 = g; g2 < M; ++g2) rhoG[g * M + g2] += yg[g] * std::conj(yg[g2]);
  }
  for (uint32_t j = 0; j < dim; ++j) CHECK(std::abs(got[j] - y[j]) < 1e-13, "amplitude %u", j);
  std::vector<double> up(2 * M * M, 0.0), rho(2 * MB * MB, -7.0);
  for (uint32_t g = 0; g < M; ++g)
    for (uint32_t g2 = g; g2 < M; ++g2) {
      up[2 * (g * M + g2)] = rhoG[g * M + g2].real();
      up[2 * (g * M + g2) + 1] = g == g2 ? 0.0 : rhoG[g * M + g2].imag();
    }
  chan_trace(u, k2, up.data(), rho.data());
  for (uint32_t b = 0; b < MB; ++b)
    for (uint32_t b2 = 0; b2 < MB; ++b2) {
      const cd v(rho[2 * (b * MB + b2)], rho[2 * (b * MB + b2) + 1]);
      CHECK(std::abs(v - want[b * MB + b2]) < 1e-13, "rho[%u][%u]", b, b2);
      CHECK(rho[2 * (b * MB + b2)] == rho[2 * (b2 * MB + b)] && rho[2 * (b * MB + b2) + 1] == -rho[2 * (b2 * MB + b) + 1], "not Hermitian bit for bit");
      if (b == b2) CHECK(rho[2 * (b * MB + b) + 1] == 0.0 && !std::signbit(rho[2 * (b * MB + b) + 1]), "diagonal imaginary part");
    }
  // the branch weight against its definition |K x|^2 (here K = A, rho the density of x on A's qubits)
  std::vector<cd> rhoA(MA * MA, cd(0, 0));
  for (uint32_t j = 0; j < dim; ++j)
    for (uint32_t a2 = 0; a2 < MA; ++a2) rhoA[sub_index(j, apos) * MA + a2] += x[j] * std::conj(x[with_sub(j, apos, a2)]);
  double norm_y = 0.0;
  for (uint32_t j = 0; j < dim; ++j) norm_y += std::norm(y[j]);
  const double wgt = chan_weight(k, reinterpret_cast<const double*>(A.data()), reinterpret_cast<const double*>(rhoA.data()));
  CHECK(std::abs(wgt - norm_y) < 1e-12 * (1.0 + norm_y), "weight %g against %g", wgt, norm_y);
}

int main() {
  const uint32_t n = 5;
  int cases = 0;
  for (uint32_t k = 1; k <= 2; ++k)
    for (uint32_t k2 = 1; k2 <= 2; ++k2) {
      std::vector<std::vector<uint64_t>> as, bs;
      for (uint64_t q0 = 0; q0 < n; ++q0) {
        as.push_back({q0});
        for (uint64_t q1 = 0; q1 < n; ++q1)
          if (q1 != q0) as.push_back({q0, q1});
      }
      for (const auto& a : as)
        for (const auto& b : as) {
          if (a.size() != k || b.size() != k2) continue;
          std::vector<uint32_t> ap, bp;
          for (uint64_t q : a) ap.push_back((uint32_t)(n - 1 - q));
          for (uint64_t q : b) bp.push_back((uint32_t)(n - 1 - q));
          if (chan_union_size(ap, bp) > kChanMaxUnion) continue;
          one_case(n, a, b, cases % 4);
          ++cases;
        }
    }
  CHECK(cases > 500, "%d cases", cases);
  // refusals of the list check
  std::vector<uint32_t> pos;
  const uint64_t twice[2] = {1, 1}, far[1] = {5};
  CHECK(!chan_check_indices(n, twice, 2, &pos).empty(), "a repeated index passed");
  CHECK(!chan_check_indices(n, far, 1, &pos).empty(), "an index out of range passed");
  CHECK(!chan_check_indices(n, far, 0, &pos).empty(), "k = 0 passed");
  CHECK(!chan_check_indices(n, nullptr, 1, &pos).empty(), "a null list passed");
  // the pass plan
  {
    std::vector<std::vector<uint32_t>> chain;
    for (uint32_t p = 0; p < 7; ++p) chain.push_back({p});
    for (int f32 = 0; f32 < 2; ++f32) {
      const ChanPlan pl = chan_plan(7, f32, f32, chain);
      CHECK(pl.passes == 8 && pl.nfused == 6, "chain of 7: %llu passes, %llu fused", (unsigned long long)pl.passes, (unsigned long long)pl.nfused);
      const ChanPlan one = chan_plan(7, f32, f32, {{3}});
      CHECK(one.passes == 2 && one.nfused == 0, "one channel");
      const ChanPlan apart = chan_plan(7, f32, f32, {{0, 1}, {2, 3}});
      CHECK(apart.passes == 4 && apart.nfused == 0, "two disjoint 2-qubit channels");
      CHECK(chan_plan(7, f32, f32, {}).passes == 0, "an empty chain");
    }
    const ChanPlan over = chan_plan(7, false, false, {{0, 1}, {1, 2}, {2}});
    CHECK(over.passes == 4 && over.nfused == 2, "overlapping pairs");
    // the measured routing: Complex<f32> with three qubits in a pass, and high positions only on a large state, run composed
    const ChanPlan over32 = chan_plan(7, true, true, {{0, 1}, {1, 2}, {2}});
    CHECK(over32.passes == 5 && over32.nfused == 1, "Complex<f32>, |G| = 3");
    CHECK(chan_fuses(30, false, false, {29}, {28}) == false && chan_fuses(27, false, false, {26}, {25}) == true, "high positions, n >= 28");
    CHECK(chan_fuses(30, false, false, {29}, {5}) == true && chan_fuses(30, false, false, {29}, {6}) == false, "a lane-id position");
    CHECK(chan_fuses(30, true, true, {29}, {6}) == true && chan_fuses(30, true, true, {29}, {7}) == false, "packed: one position lower");
    CHECK(chan_fuses(30, false, false, {29, 28}, {27}) == true && chan_fuses(30, true, true, {29, 28}, {27}) == false, "|G| = 3");
    CHECK(chan_fuses(30, false, false, {29, 28}, {27, 26}) == false, "a union of four");
  }
  // the selection rule
  {
    const double w[4] = {0.0, 0.25, 0.0, 0.75};
    double W = 0;
    CHECK(chan_select(w, 4, 0.0, &W) == 1 && W == 1.0, "u = 0 takes the first branch with weight");
    CHECK(chan_select(w, 4, 0.2499, &W) == 1 && chan_select(w, 4, 0.25, &W) == 3, "the boundary belongs to the next branch");
    CHECK(chan_select(w, 4, 1.0, &W) == 3, "u = 1 takes the last branch with weight");
    const double tail[3] = {0.5, 0.5, 0.0};
    CHECK(chan_select(tail, 3, 1.0, &W) == 1, "a zero-weight tail is never taken");
    const double none[2] = {0.0, 0.0};
    CHECK(chan_select(none, 2, 0.5, &W) == -1, "no weight at all");
    const double bad[2] = {0.5, std::nan("")};
    CHECK(chan_select(bad, 2, 0.5, &W) == -1, "a weight that is not finite");
  }
  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("channel plan ok: %d cases\n", cases);
  return 0;
}
