// qip_qft_kernels.h — the device side of qipx_state_apply_qft (include/qip_hipx.h): one in-place pass of the decimation-in-
// frequency flow over a state, in the shape of k_function_tile.  qip_qft_plan.h has the passes, the tile, the steps and the
// twiddle exponents; this file has the kernel alone.
//
// A block owns one tile of 2^tbits amplitudes: the wave row (index positions 0..5) and kt other positions.  A thread holds
// 2^E amplitudes at a time.
//   load     slot = thread | j << (tbits - E): whole 64-amplitude rows, 16 (8) bytes per lane, non-temporal on a large state;
//            into LDS at qft_lds_slot(slot)
//   steps    a thread opens the step's E element bits in its number, reads the 2^E amplitudes that differ in them, runs the
//            step's stages (at most E) on them in registers and writes them back to the same LDS words: a thread only ever
//            touches its own words inside a step, so one barrier per step is enough.  The stage twiddle W_(2^L)^(v << (L-1-j))
//            is one table entry (`tw`, built by the host in double and rounded once to the state's precision, 2^(L-1) entries:
//            L2-resident); v, the register bits below the stage's, is gathered from the slot with the descriptor's short lists,
//            the thread's part once per step and the element's part from compile-time element numbers.
//   store    the rows go back to the addresses they came from.  On the way out an amplitude takes its pass's scale 2^(-L/2) and,
//            when register bits lie below the pass, the outer twiddle W_(2^hi)^(k * xlow): the exponent is an exact 64-bit integer,
//            the sine and cosine are evaluated in double (sincospi: exact reduction) for both precisions, the scale is folded in
//            and the factor rounded once to the state's precision.  The only pass of a natural-order call reads LDS through the
//            digit reversal of the register bits instead (it has no outer twiddle: lo = 0).
// Every amplitude is read once and written once per pass; no atomics, the same bits whatever the grid.
// Occupancy: kt = 6 is 64 KiB of Complex<f64> per block of 512 threads (two blocks per CU), the filled-up kt = 5 tile 32 KiB per
// 256 threads; Complex<f32> half of each, moved as 8-byte amplitudes (index bit 0 may be a register bit).
#pragma once
#include "qip_qft_plan.h"
#include "qip_kernels.h"

namespace qipk {

template <typename T, int E, bool NT>
__global__ __launch_bounds__(512)
void k_qft_tile(amp_t<T>* __restrict__ st, uint64_t ntiles, Ins ins, QftDesc d, const amp_t<T>* __restrict__ tw) {
  using A = amp_t<T>;
  constexpr int NE = 1 << E;
  extern __shared__ __attribute__((aligned(16))) unsigned char qft_tile_raw[];
  A* tile = reinterpret_cast<A*>(qft_tile_raw);
  const uint64_t blk = blockIdx.x + (uint64_t)blockIdx.y * gridDim.x;
  if (blk >= ntiles) return;
  const uint32_t t = threadIdx.x, lg = d.tbits - (uint32_t)E, L = d.hi - d.lo;
  const uint64_t base = d.kt ? tile_block_base(blk, ins, 5u) : 0ull;
  // the thread's part of the load / store slots (slot bits below lg) and the j part (slot bits lg .. lg + E - 1)
  uint64_t gt = t & 63u, xt = 0;
  uint32_t vt = 0;
#pragma unroll
  for (int b = 0; b < (int)kQftSlotBits; ++b) {
    const bool set = (uint32_t)b < lg && ((t >> b) & 1u);
    if (b >= 6) gt |= set ? d.hoff[b - 6] : 0ull;
    vt |= set ? d.vmap[b] : 0u;
    xt |= set ? d.xmap[b] : 0ull;
  }
  uint64_t jg[E], jx[E];
  uint32_t jv[E];
#pragma unroll
  for (int k = 0; k < E; ++k) {
    const uint32_t b = lg + (uint32_t)k;
    jg[k] = b >= 6u ? d.hoff[b - 6u] : 1ull << b;
    jv[k] = d.vmap[b];
    jx[k] = d.xmap[b];
  }
  uint64_t g[NE];
  A a[NE];
#pragma unroll
  for (int j = 0; j < NE; ++j) {
    uint64_t off = gt;
#pragma unroll
    for (int k = 0; k < E; ++k) off |= ((j >> k) & 1) ? jg[k] : 0ull;
    g[j] = base | off;
    a[j] = ldg<NT>(st + g[j]);
  }
#pragma unroll
  for (int j = 0; j < NE; ++j) tile[qft_lds_slot(t | ((uint32_t)j << lg))] = a[j];
  __syncthreads();

  for (uint32_t s = 0; s < d.nsteps; ++s) {
    const QftStep sp = d.step[s];
    uint32_t b0 = t;
#pragma unroll
    for (int k = 0; k < E; ++k) b0 = qft_open(b0, sp.ins[k]);
    uint32_t vb = 0;
#pragma unroll
    for (int b = 0; b < (int)kQftSlotBits; ++b) vb |= ((b0 >> b) & 1u) ? d.vmap[b] : 0u;
    uint32_t eo[NE], ev[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      eo[e] = 0, ev[e] = 0;
#pragma unroll
      for (int k = 0; k < E; ++k)
        if ((e >> k) & 1) eo[e] |= 1u << sp.ebit[k], ev[e] |= sp.evm[k];
      a[e] = tile[qft_lds_slot(b0 | eo[e])];
    }
#pragma unroll
    for (int q = 0; q < E; ++q) {
      if ((uint32_t)q < sp.r) {
        const int k = E - 1 - q;
        const uint32_t j = sp.top - (uint32_t)q, mask = (1u << j) - 1u, sh = L - 1u - j;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
          if ((e >> k) & 1) continue;
          const int e1 = e | (1 << k);
          const A w = tw[((vb | ev[e]) & mask) << sh];
          const A sum = a[e] + a[e1], dif = a[e] - a[e1];
          a[e] = sum;
          a[e1] = cmul(w, dif);
        }
      }
    }
#pragma unroll
    for (int e = 0; e < NE; ++e) tile[qft_lds_slot(b0 | eo[e])] = a[e];
    __syncthreads();
  }

  uint64_t xb = 0;
  for (uint32_t i = 0; i < d.nb; ++i) xb |= ((base >> d.bpos[i]) & 1ull) << d.bbit[i];
  const T scale = (T)d.scale;
#pragma unroll
  for (int j = 0; j < NE; ++j) {
    const uint32_t slot = t | ((uint32_t)j << lg);
    uint32_t v = vt;
    uint64_t xl = xb | xt;
#pragma unroll
    for (int k = 0; k < E; ++k) {
      v |= ((j >> k) & 1) ? jv[k] : 0u;
      xl |= ((j >> k) & 1) ? jx[k] : 0ull;
    }
    const uint32_t kdig = L ? __brev(v) >> (32u - L) : 0u;
    uint32_t src = slot;
    if (d.natural) {
      src = slot & ~d.vmask;
#pragma unroll
      for (int b = 0; b < (int)kQftSlotBits; ++b) src |= ((kdig >> b) & 1u) << d.vslot[b];
    }
    A x = tile[qft_lds_slot(src)];
    if (d.lo > 0) {
      const uint64_t tt = (uint64_t)kdig * xl;  // < 2^hi: exact
      double sn, cs;
      sincospi((double)tt * d.unit, &sn, &cs);
      A w;
      w.x = (T)(cs * d.scale);
      w.y = (T)((d.sign < 0 ? -sn : sn) * d.scale);
      x = cmul(w, x);
    } else {
      x.x *= scale;
      x.y *= scale;
    }
    stg<NT>(st + g[j], x);
  }
}

}  // namespace qipk
