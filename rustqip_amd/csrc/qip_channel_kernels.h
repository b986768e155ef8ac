// qip_channel_kernels.h — the fused pass of the noise-channel calls (qipx_state_apply_reduce / qipx_state_apply_channels,
// include/qip_hipx.h): psi <- W psi in place on the |G| <= 3 SORTED positions of G and, from the same read, the density matrix of
// the STORED result on G.
//
// The gather is k_density_small's (qip_kernels.h), unchanged: Ins / DensDesc, the high positions walked by `coff`, the low ones
// transposed in the wave, the B0 and packed f32x4 cases, one non-temporal 16-byte load per element.  After the transpose a lane
// owns whole groups of M = 2^|G| amplitudes x[a].  Per group:
//   y[a] = sum_{a'} W[a][a'] x[a']   in double for both precisions (f32 amplitudes widened first), per part ONE chain of fused
//          multiply-adds in ascending a' — Re: wr xr', then -wi xi'; Im: wr xi', then wi xr' — started from -0.0, so that the first
//          product arrives with its own bits.  DIAG (the operator is diagonal on G): only W[a][a] is looked at, and the host marks
//          which of its real and imaginary parts are not zero (ChanW::nzr / nzi, kernel arguments: the branches are uniform);
//          the others are not multiplied, so the identity returns x[a] bit for bit and a zero entry gives exactly +0.  Otherwise
//          all M entries of a row are multiplied, the zeros of the identity padding included: per-entry flags were measured and
//          lost (128 uniform branches around scalar loads per group cost more than the 2 M^2 dead multiply-adds they save:
//          profiles/noise.md); a sum of zero products is stored as +0.  A Complex<f32> result is rounded once to f32.
//   rho    the stored y (the f32-rounded value for an f32 state) goes into exactly the accumulator slots of k_density_small, by
//          the same products and the same fused multiply-adds.
//   store  the wave transpose is undone (each stage is its own inverse and the stages commute) and every element goes back to the
//          address it was loaded from with an ordinary store.  A lane stores only what it loaded; groups are disjoint, so no lane
//          writes what another lane reads.
// No atomics: one partial matrix per block in block order, k_density_small's fold.
#pragma once
#include "qip_kernels.h"

namespace qipk {

struct ChanW {
  double w[128];             // W[a][a'] at w[2 (a M + a')] and + 1, M = 2^|G|
  uint32_t nzr[8], nzi[8];   // row a: bit a' is set when Re / Im W[a][a'] is not zero
};

template <typename T, int KE, int KL, bool B0, bool DIAG, typename E = amp_t<T>>
__global__ __launch_bounds__(kBlock) void k_apply_density_small(E* st, Ins ins, DensDesc d, ChanW cw, double* __restrict__ partial) {
  constexpr bool PACKED = !SameT<E, amp_t<T>>::v;
  static_assert(PACKED || !B0, "the half bit exists in packed elements only");
  constexpr int KH = KE - KL, ME = 1 << KE, NC = 1 << KH, U = 1 << KL, R = ME >= 4 ? 1 : 4 / ME;
  constexpr int M = B0 ? 2 * ME : ME, NCOL = (PACKED && !B0) ? 2 : 1, NP = M * (M - 1) / 2, NACC = M * M;
  static_assert(M <= 8, "|G| <= 3");
  __shared__ double smem[(kBlock / 64) * NACC];
  double dg[M], re[NP], im[NP];
#pragma unroll
  for (int a = 0; a < M; ++a) dg[a] = 0.0;
#pragma unroll
  for (int p = 0; p < NP; ++p) re[p] = im[p] = 0.0;
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint64_t nwaves = (uint64_t)gridDim.x * (kBlock / 64);
  auto transpose = [&](E (&x)[U][NC]) {
#pragma unroll
    for (int i = 0; i < KL; ++i) {
      const bool up = (lane >> d.lpos[i]) & 1u;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if ((u >> i) & 1) continue;
        const int u1 = u | (1 << i);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const E e0 = x[u][c], e1 = x[u1][c];
          const E got = shfl_xor_e<E>(up ? e0 : e1, 1 << d.lpos[i]);
          x[u][c] = up ? got : e0;
          x[u1][c] = up ? e1 : got;
        }
      }
    }
  };
  for (uint64_t row0 = ((uint64_t)blockIdx.x * (kBlock / 64) + wv) * (U * R); row0 < d.nrows; row0 += nwaves * (U * R)) {
    E x[R][U][NC];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint64_t row = row0 + (uint64_t)(r * U + u);
        const bool valid = row < d.nrows && lane < d.nlane;
        const uint64_t base = insert_bits<KH>((row << 6) | lane, ins);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          E e = {};
          if (valid) e = __builtin_nontemporal_load(st + (base | d.coff[c]));
          x[r][u][c] = e;
        }
      }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      transpose(x[r]);
#pragma unroll
      for (int col = 0; col < NCOL; ++col) {
        double vr[M], vi[M];
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const E e = x[r][u][c];
            const int ie = (c << KL) | u;
            if constexpr (!PACKED) {
              vr[ie] = (double)e.x;
              vi[ie] = (double)e.y;
            } else if constexpr (B0) {
              vr[2 * ie] = (double)e.x;
              vi[2 * ie] = (double)e.y;
              vr[2 * ie + 1] = (double)e.z;
              vi[2 * ie + 1] = (double)e.w;
            } else {
              vr[ie] = (double)(col ? e.z : e.x);
              vi[ie] = (double)(col ? e.w : e.y);
            }
          }
        // y = W x, rounded once to the state's precision
        T yr[M], yi[M];
#pragma unroll
        for (int a = 0; a < M; ++a) {
          double sr = -0.0, si = -0.0;
          if constexpr (DIAG) {
            const double wr = cw.w[2 * (a * M + a)], wi = cw.w[2 * (a * M + a) + 1];
            if ((cw.nzr[a] >> a) & 1u) {
              sr = __builtin_fma(wr, vr[a], sr);
              si = __builtin_fma(wr, vi[a], si);
            }
            if ((cw.nzi[a] >> a) & 1u) {
              sr = __builtin_fma(-wi, vi[a], sr);
              si = __builtin_fma(wi, vr[a], si);
            }
            if ((((cw.nzr[a] | cw.nzi[a]) >> a) & 1u) == 0u) sr = si = 0.0;
          } else {
#pragma unroll
            for (int a2 = 0; a2 < M; ++a2) {
              const double wr = cw.w[2 * (a * M + a2)], wi = cw.w[2 * (a * M + a2) + 1];
              sr = __builtin_fma(-wi, vi[a2], __builtin_fma(wr, vr[a2], sr));
              si = __builtin_fma(wi, vr[a2], __builtin_fma(wr, vi[a2], si));
            }
            sr += 0.0;  // (a sum of zero products may be -0.0: stored as +0.0)
            si += 0.0;
          }
          yr[a] = (T)sr;
          yi[a] = (T)si;
        }
        // the density matrix of the stored result: k_density_small's slots, products and fused multiply-adds
        {
          double zr[M], zi[M];
#pragma unroll
          for (int a = 0; a < M; ++a) {
            zr[a] = (double)yr[a];
            zi[a] = (double)yi[a];
          }
#pragma unroll
          for (int a = 0; a < M; ++a) dg[a] = __builtin_fma(zi[a], zi[a], __builtin_fma(zr[a], zr[a], dg[a]));
          int p = 0;
#pragma unroll
          for (int a = 0; a < M; ++a)
#pragma unroll
            for (int a2 = a + 1; a2 < M; ++a2, ++p) {
              re[p] = __builtin_fma(zi[a], zi[a2], __builtin_fma(zr[a], zr[a2], re[p]));
              im[p] = __builtin_fma(-zr[a], zi[a2], __builtin_fma(zi[a], zr[a2], im[p]));
            }
        }
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
          for (int u = 0; u < U; ++u) {
            E& e = x[r][u][c];
            const int ie = (c << KL) | u;
            if constexpr (!PACKED) {
              e.x = yr[ie];
              e.y = yi[ie];
            } else if constexpr (B0) {
              e.x = yr[2 * ie];
              e.y = yi[2 * ie];
              e.z = yr[2 * ie + 1];
              e.w = yi[2 * ie + 1];
            } else if (col) {
              e.z = yr[ie];
              e.w = yi[ie];
            } else {
              e.x = yr[ie];
              e.y = yi[ie];
            }
          }
      }
      transpose(x[r]);
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint64_t row = row0 + (uint64_t)(r * U + u);
        const bool valid = row < d.nrows && lane < d.nlane;
        const uint64_t base = insert_bits<KH>((row << 6) | lane, ins);
        if (valid) {
#pragma unroll
          for (int c = 0; c < NC; ++c) st[base | d.coff[c]] = x[r][u][c];
        }
      }
  }
  // the wave (shuffle tree), then the block's four waves in wave order
  auto fold = [&](double v, int slot) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if (lane == 0) smem[wv * NACC + slot] = v;
  };
#pragma unroll
  for (int a = 0; a < M; ++a) fold(dg[a], a);
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    fold(re[p], M + 2 * p);
    fold(im[p], M + 2 * p + 1);
  }
  __syncthreads();
  for (int slot = threadIdx.x; slot < NACC; slot += kBlock)
    partial[(uint64_t)blockIdx.x * NACC + slot] = ((smem[slot] + smem[NACC + slot]) + smem[2 * NACC + slot]) + smem[3 * NACC + slot];
}

}  // namespace qipk
