// qip_multiplex_kernels.h — the device side of qipx_state_apply_multiplexed (include/qip_hipx.h): one in-place pass of
// |x>|t> -> |x> U_x|t> over a state.  qip_multiplex_plan.h has the walk and the descriptor; this file has the kernel alone.
//
// A wave walks `steps` steps of U items.  Per item a lane loads the H = 2^kh amplitudes of its group whose target positions lie
// outside the wave row, as H whole rows (16-byte accesses of Complex<f64>, 8-byte ones of Complex<f32>: index bit 0 may belong to
// either register, and one body then serves both precisions and every placement); the amplitudes whose target positions lie
// INSIDE the row belong to other lanes of the same wave and come by a wave shuffle.  After M = 2^k shuffles (none when every
// target is outside the row) a lane holds its whole group v[0..M) in matrix-index order, computes the H rows it loaded, and
// stores them to the addresses they came from: every amplitude is read once and written once, no LDS, no atomics, no second buffer.
//   rows     a lane keeps only the H rows of U_x that it stores (H * M table entries, contiguous per row) in registers, fetched
//            after the step's amplitude loads are issued and only at a step whose x differs from the step before (mx_refetch:
//            wave-uniform).  With the select bits above the walk that is once per wave; with select bits inside the row every lane
//            has rows of its own and still fetches them once per walk.
//   sum      y_a = p_0, then y_a += p_a' for a' ascending, p_a' = U_x[a][a'] * v[a'] as four products and two sums, never
//            contracted: every lane adds in matrix-index order, whichever of the terms is its own amplitude.
//   identity a row that is exactly the unit row e_a is not computed: the amplitude keeps its bits (a select, not a branch).
// Measured (profiles/multiplex.md, n = 30): 1.07 - 1.21 dense gate passes on the same targets for m <= 10 in Complex<f64>, 1.06 - 1.12
// in Complex<f32> with a target inside the row; two targets outside the row 1.23 - 1.32 / 1.29 - 1.37 (HM = 3 holds 16 matrix entries
// and 4 amplitudes per lane: 181 VGPRs, two waves per SIMD in Complex<f64>).  The pass loses to 4 controlled gates through apply_ops
// at m = 2, k = 1 in Complex<f64> and to one block-diagonal dense op on 3 - 5 qubits (Complex<f32>: 3 - 4).
// HM: the matrix-index bits whose target sits outside the row (a compile-time set: the lane's registers are indexed by them).
#pragma once
#include "qip_multiplex_plan.h"
#include "qip_kernels.h"

namespace qipk {

// the c-th subset of the bits of HM, as matrix-index bits (c < 2^popcount(HM))
template <int HM> __device__ __forceinline__ constexpr uint32_t mx_spread(uint32_t c) {
  return HM == 3 ? c : HM == 2 ? c << 1 : HM == 1 ? c : 0u;
}
// ... and back: the register that holds matrix index a
template <int HM> __device__ __forceinline__ constexpr uint32_t mx_pick(uint32_t a) {
  return HM == 3 ? a : HM == 2 ? a >> 1 : HM == 1 ? (a & 1u) : 0u;
}

template <typename T, int K, int HM, int U, bool NT>
__global__ __launch_bounds__(64 * kMxWaves)
void k_multiplex(amp_t<T>* __restrict__ st, uint64_t nwaves, MxDesc d, const amp_t<T>* __restrict__ tab) {
  using A = amp_t<T>;
  constexpr int M = 1 << K;
  constexpr int H = HM == 3 ? 4 : HM == 0 ? 1 : 2;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t wb = (blockIdx.x + (uint64_t)blockIdx.y * gridDim.x) * (blockDim.x >> 6) + wave;
  if (wb >= nwaves) return;
  const uint64_t base = mx_wave_base(d, wb);
  const uint32_t xb = mx_wave_x(d, base);
  const uint32_t xl = mx_lane_x(d, lane);
  const uint32_t al = mx_lane_a(d, lane);
  const bool live = lane < d.rowlen;  // (below n = 6 a row is shorter than the wave)
  int src[M];
#pragma unroll
  for (int a = 0; a < M; ++a) src[a] = (int)mx_src_lane(d, lane, (uint32_t)a);
  uint64_t hoff[H];
#pragma unroll
  for (int c = 0; c < H; ++c) hoff[c] = mx_high_off(d, mx_spread<HM>((uint32_t)c));

  A row[H][M];
  bool unit[H];
#pragma unroll
  for (int c = 0; c < H; ++c) {
    unit[c] = false;
#pragma unroll
    for (int a = 0; a < M; ++a) row[c][a] = czero<A>();
  }
  for (uint32_t t = 0; t < d.steps; ++t) {
    A own[U][H];
    uint64_t g[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      g[u] = (base | mx_walk_off(d, (t << d.lu) | (uint32_t)u)) + lane;
#pragma unroll
      for (int c = 0; c < H; ++c) own[u][c] = live ? ldg<NT>(st + (g[u] | hoff[c])) : czero<A>();
    }
    if (mx_refetch(d, t)) {  // (wave-uniform; the fetches go out behind the step's loads)
      const uint32_t x = xb | mx_walk_x(d, t << d.lu) | xl;
#pragma unroll
      for (int c = 0; c < H; ++c) {
        const uint32_t a = mx_spread<HM>((uint32_t)c) | al;
        const A* r = tab + ((((size_t)x << K) + a) << K);  // row a of U_x
        bool is_unit = true;
#pragma unroll
        for (int b = 0; b < M; ++b) {
          row[c][b] = r[b];
          is_unit = is_unit && row[c][b].x == ((uint32_t)b == a ? (T)1 : (T)0) && row[c][b].y == (T)0;
        }
        unit[c] = is_unit;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      A v[M];
#pragma unroll
      for (int a = 0; a < M; ++a) {
        const A mine = own[u][mx_pick<HM>((uint32_t)a)];
        if constexpr (HM == M - 1) v[a] = mine;  // every target outside the row: the group is the lane's own
        else v[a] = shfl_e(mine, src[a]);
      }
#pragma unroll
      for (int c = 0; c < H; ++c) {
        A y = cmul(row[c][0], v[0]);
#pragma unroll
        for (int b = 1; b < M; ++b) y = cadd(y, cmul(row[c][b], v[b]));
        y = unit[c] ? own[u][c] : y;
        if (live) stg<NT>(st + (g[u] | hoff[c]), y);
      }
    }
  }
}

}  // namespace qipk
