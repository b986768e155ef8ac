// qip_function_kernels.h — the device side of qipx_state_apply_function (include/qip_hipx.h): one in-place pass of
// |x>|y> -> w(x) |x>|y'> over a state, in the shape of k_sparse_tile (qip_kernels.h).  qip_function_plan.h has the tile and the
// descriptor; this file has the kernel alone.
//
// A block owns tiles of 2^(6+kt) amplitudes: the wave row (index positions 0..5, the lane) and kt other positions.  A wave
// loads U rows of the tile as whole 64-amplitude rows, writes every amplitude to its DESTINATION slot in LDS, and after one
// barrier reads its own slots back and stores the same rows: each amplitude is read once and written once, in place, no
// atomics, no second buffer.
//   x        = (bits of the block base) | (bits of the row) | (bits of the lane): the first two are wave-uniform and are gathered
//              with scalar arithmetic over short lists, the third once per lane.  The map keeps x, so the lane that loads index j
//              also stores index j with the same x: one table fetch serves the move and the phase.
//   table    one 32-bit word per x, fetched from global memory while the tile's loads are in flight (small, L2-resident; the
//              same address across a wave when no in-register bit sits in the row).
//              XOR: the host has already spread the value's bits over the tile's slot bits, so the destination is slot ^ word.
//              ADD: the word is the value; y is gathered (row part scalar, lane part once per lane), y' = (y + value) mod 2^k is
//              spread over the slot bits in 12 unrolled steps (k <= 12).
//   LDS      the scatter side is the write (ds_write_b128 / b64 to slot'), the read side is linear in the lane: conflict-free.
//            With one table word per wave an XOR permutes the lanes of a row or moves whole rows: conflict-free too.  With
//            in-register bits inside the row the scatter is as irregular as the table, and its conflicts are the data's.
//   phase    w(x) on the way in (x is the same at both ends of a move), one complex product in the state's precision; an entry
//            that is exactly (1, 0) is not multiplied (the amplitude keeps its bits).
//   MODE     kFnPhaseOnly: an empty out register, nothing moves and LDS is not used.
// Occupancy: kt = 6 is 64 KiB of Complex<f64> per block of 512 lanes (two blocks per CU), the filled-up kt = 5 tile 32 KiB per
// 256 lanes (five per CU); Complex<f32> half of each.  Complex<f32> is moved as 8-byte amplitudes in both cases: index bit 0 may
// be in either register, and one kernel body then serves both precisions and every placement.
#pragma once
#include "qip_function_plan.h"
#include "qip_kernels.h"

namespace qipk {

template <typename T, int U, int MODE, bool PH, bool NT>
// (fewer than 8 rows per wave: a tile of fewer than 8 rows, one wave)
__global__ __launch_bounds__(U == 8 ? 512 : 64)
void k_function_tile(amp_t<T>* __restrict__ st, uint64_t ntiles, Ins ins, FnDesc d, const uint32_t* __restrict__ tab,
                     const amp_t<T>* __restrict__ w) {
  using A = amp_t<T>;
  extern __shared__ __attribute__((aligned(16))) unsigned char function_tile_raw[];
  A* tile = reinterpret_cast<A*>(function_tile_raw);
  const uint64_t blk = blockIdx.x + (uint64_t)blockIdx.y * gridDim.x;
  if (blk >= ntiles) return;
  const uint32_t lane = threadIdx.x & 63u, nw = blockDim.x >> 6;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t base = tile_block_base(blk, ins, 5u);
  uint32_t xb = 0;
  for (uint32_t j = 0; j < d.nb; ++j) xb |= (uint32_t)((base >> d.bpos[j]) & 1ull) << d.bbit[j];
  uint32_t xl = 0, yl = 0;
#pragma unroll
  for (int b = 0; b < 6; ++b) {
    if ((lane >> b) & 1u) {
      xl |= d.lx[b];
      if constexpr (MODE == kFnAdd) yl |= d.ly[b];
    }
  }
  // (all of a lane's rows first, in straight-line code: a row bit above the tile's is zero, so every list is walked to its full
  // length with selects and no branch stands between the loads)
  uint64_t g[U];
  uint32_t x[U], yr[U];
#pragma unroll
  for (int i = 0; i < U; ++i) {
    const uint32_t r = (uint32_t)i * nw + wave;
    uint64_t off = 0;
    uint32_t xr = 0;
    yr[i] = 0;
#pragma unroll
    for (int t = 0; t < (int)kFnTileHigh; ++t) {
      const bool set = (r >> t) & 1u;
      off |= set ? d.hoff[t] : 0ull;
      xr |= set ? d.hx[t] : 0u;
      if constexpr (MODE == kFnAdd) yr[i] |= set ? d.hy[t] : 0u;
    }
    g[i] = (base | off) + lane;
    x[i] = xb | xr | xl;
  }
  if (lane < d.rowlen) {  // (below n = 6 a row is shorter than the wave)
    A a[U], ph[U];
    uint32_t v[U];
#pragma unroll
    for (int i = 0; i < U; ++i) {
      a[i] = ldg<NT>(st + g[i]);
      if constexpr (MODE != kFnPhaseOnly) v[i] = tab[x[i]];
      if constexpr (PH) ph[i] = w[x[i]];
    }
    if constexpr (PH) {
#pragma unroll
      for (int i = 0; i < U; ++i) {
        const bool unit = ph[i].x == (T)1 && ph[i].y == (T)0;
        const A e = cmul(ph[i], a[i]);
        a[i] = unit ? a[i] : e;
      }
    }
    if constexpr (MODE == kFnPhaseOnly) {
#pragma unroll
      for (int i = 0; i < U; ++i) stg<NT>(st + g[i], a[i]);
    } else {
#pragma unroll
      for (int i = 0; i < U; ++i) {
        const uint32_t slot = (((uint32_t)i * nw + wave) << 6) | lane;
        uint32_t to;
        if constexpr (MODE == kFnXor) {
          to = slot ^ v[i];
        } else {
          const uint32_t y = ((yr[i] | yl) + v[i]) & d.kmask;  // (k <= 12: bits of y above k are zero and spread nothing)
          to = slot & ~d.ymask;
#pragma unroll
          for (int b = 0; b < 6 + (int)kFnTileHigh; ++b) to |= ((y >> b) & 1u) << d.yslot[b];
        }
        tile[to] = a[i];
      }
    }
  }
  if constexpr (MODE != kFnPhaseOnly) {
    __syncthreads();
    if (lane < d.rowlen) {
#pragma unroll
      for (int i = 0; i < U; ++i) stg<NT>(st + g[i], tile[(((uint32_t)i * nw + wave) << 6) | lane]);
    }
  }
}

}  // namespace qipk
