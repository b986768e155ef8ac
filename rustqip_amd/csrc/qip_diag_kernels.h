// qip_diag_kernels.h — the device side of the diagonal Pauli-sum calls (qipx_state_apply_diagonal, qipx_state_expect_diagonal of
// include/qip_hipx.h; qip_pauli.hip is the only unit that includes this): k_diag_phase and k_diag_moments over ONE walk of a
// block's tiles (diag_walk).  Never compiled at run time.
//
// A block takes `tiles_per_block` contiguous tiles of 2^L amplitudes (qip_diag_plan.h).  Per tile h:
//   zero    the table of 2^L doubles in LDS
//   build   a_h: the groups (terms of one low mask) dealt to the lanes, a group's terms summed serially in the order of the call
//           starting from +0, (+-)k_t an exact sign flip by the parity of h & zhi_t; distinct groups own distinct entries
//   fold    the butterfly over index bits 0 .. L-1 in ascending order.  A full tile (L = kDiagTileBits): passes in which a lane
//           holds 2^(L-8) entries in registers and runs L-8 stages on them (bits B .. B+L-9 vary inside the lane, the lane id
//           fills the rest; the last pass always holds bits 8 .. L-1 and runs the stages still missing), one LDS round trip and
//           one barrier per pass.  The one short tile of a state with n < kDiagTileBits: one stage and one barrier at a time.
//           Both forms do the same additions on the same values: the table's bits do not depend on the form.
//   rows    16-byte elements, coalesced (non-temporal on full tiles, four loads in flight per lane), the energies of an element's
//           amplitudes read from the table.
// The table is padded by one double per 16 (diag_pad): with the bank rule of ds_read_b64 (bank = dword address mod 64 within a
// half-wave) a lane stride of 16 doubles — the first pass, 16 entries per lane — becomes 17 doubles = 34 dwords, which visits every
// even bank once per half-wave, and the second pass (16 neighbours, then 256 apart) lands on 2 lo + 32 hi: conflict-free as well.
// The rows read neighbours (one bank in 16 is met twice).
#pragma once
#include "qip_kernels.h"
#include "qip_diag_plan.h"
#include "qip_pauli_kernels.h"  // pauli_get, pauli_put, flip_sign

namespace qipk {

static_assert(kDiagBlock == (uint32_t)kBlock, "diag_chain_length and the lanes of a tile assume one block of kBlock lanes");

struct DiagSumDesc {
  const DiagTerm* terms;
  const uint32_t* group_start;  // ngroups + 1
  const uint32_t* group_mask;
  uint32_t ngroups, tile_bits;
  uint64_t ntiles, tiles_per_block;
};

constexpr int kDiagLaneBits = (int)kDiagTileBits - 8;  // entries of a full tile per lane: 2^kDiagLaneBits
constexpr int kDiagTableSize = (1 << kDiagTileBits) + (1 << (kDiagTileBits - 4));
__device__ __forceinline__ uint32_t diag_pad(uint32_t i) { return i + (i >> 4); }

// one register pass of a full tile: the lane holds the entries whose bits B .. B + kDiagLaneBits - 1 vary and runs the stages of
// bits FROM .. B + kDiagLaneBits - 1 on them, in ascending order
template <int B, int FROM>
__device__ __forceinline__ void diag_pass(double* tab) {
  constexpr int W = kDiagLaneBits, V = 1 << W;
  const uint32_t low = threadIdx.x & ((1u << B) - 1u), high = threadIdx.x >> B;
  const uint32_t base = low | (high << (B + W));
  double v[V];
#pragma unroll
  for (int r = 0; r < V; ++r) v[r] = tab[diag_pad(base | ((uint32_t)r << B))];
#pragma unroll
  for (int b = FROM - B; b < W; ++b)
#pragma unroll
    for (int r = 0; r < V; ++r)
      if (!((r >> b) & 1)) {
        const double u = v[r], w = v[r | (1 << b)];
        v[r] = u + w;
        v[r | (1 << b)] = u - w;
      }
#pragma unroll
  for (int r = 0; r < V; ++r) tab[diag_pad(base | ((uint32_t)r << B))] = v[r];
  __syncthreads();
}
template <int B>
__device__ __forceinline__ void diag_passes(double* tab) {
  if constexpr (B + kDiagLaneBits <= (int)kDiagTileBits) {
    diag_pass<B, B>(tab);
    diag_passes<B + kDiagLaneBits>(tab);
  } else if constexpr (B < (int)kDiagTileBits) {
    diag_pass<8, B>(tab);
  }
}

// the table of tile h: tab[diag_pad(l)] = E^((h << L) | l), complete for every lane on return
__device__ __forceinline__ void diag_table(double* tab, const DiagSumDesc& d, uint64_t h) {
  const uint32_t size = 1u << d.tile_bits;
  for (uint32_t i = threadIdx.x; i < size; i += kBlock) tab[diag_pad(i)] = 0.0;
  __syncthreads();
  for (uint32_t g = threadIdx.x; g < d.ngroups; g += kBlock) {
    double sum = 0.0;
    const uint32_t end = d.group_start[g + 1];
    uint32_t t = d.group_start[g];
    // eight terms in flight: the loads do not depend on the sum, the additions keep their order (one load at a time left a group
    // of hundreds of terms waiting a cache round trip per term: profiles/diagonal.md)
    for (; t + 8 <= end; t += 8) {
      DiagTerm term[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) term[i] = d.terms[t + i];
#pragma unroll
      for (int i = 0; i < 8; ++i) sum += flip_sign(term[i].k, (uint32_t)__popcll(h & term[i].zhi) & 1u);
    }
    for (; t < end; ++t) {
      const DiagTerm term = d.terms[t];
      sum += flip_sign(term.k, (uint32_t)__popcll(h & term.zhi) & 1u);
    }
    tab[diag_pad(d.group_mask[g])] = sum;
  }
  __syncthreads();
  if (d.tile_bits == kDiagTileBits) {
    diag_passes<0>(tab);
  } else {
    for (uint32_t s = 0; s < d.tile_bits; ++s) {
      for (uint32_t p = threadIdx.x; p < (size >> 1); p += kBlock) {
        const uint32_t i = ((p >> s) << (s + 1)) | (p & ((1u << s) - 1u));
        const uint32_t a = diag_pad(i), b = diag_pad(i | (1u << s));
        const double u = tab[a], v = tab[b];
        tab[a] = u + v;
        tab[b] = u - v;
      }
      __syncthreads();
    }
  }
}

// The walk: for every tile of the block, the table, then body(element pointer, e0, e1, streaming) for every 16-byte element of
// the tile in rows of kBlock, ascending: e0 = the energy of the element's amplitude (of its lower half, when packed), e1 = of its
// upper half.  Full tiles: four elements per lane in flight (`load` all, then `body` each, in row order).
//   load(pointer, streaming) -> E        body(pointer, E, e0, e1, streaming)
template <typename E, bool PACKED, typename P, typename L, typename F>
__device__ __forceinline__ void diag_walk(P* st, const DiagSumDesc& d, double* tab, L&& load, F&& body) {
  constexpr uint32_t SHIFT = PACKED ? 1u : 0u;
  const uint64_t first = (uint64_t)blockIdx.x * d.tiles_per_block;
  const uint64_t last = first + d.tiles_per_block < d.ntiles ? first + d.tiles_per_block : d.ntiles;
  const uint32_t elems = (1u << d.tile_bits) >> SHIFT;
  auto energies = [&](uint32_t e, double* e0, double* e1) {
    if constexpr (PACKED) {
      const uint32_t at = diag_pad(2u * e);  // (2e is even: 2e + 1 lies in the same run of 16)
      *e0 = tab[at], *e1 = tab[at + 1];
    } else {
      *e0 = tab[diag_pad(e)], *e1 = 0.0;
    }
  };
  for (uint64_t h = first; h < last; ++h) {
    diag_table(tab, d, h);
    P* tile = st + h * elems;
    if (d.tile_bits == kDiagTileBits) {
      constexpr uint32_t kRows = ((1u << kDiagTileBits) >> SHIFT) / kBlock;
      constexpr uint32_t U = kRows < 4 ? kRows : 4;
#pragma unroll 1
      for (uint32_t r = 0; r < kRows; r += U) {
        E x[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) x[u] = load(tile + (r + u) * kBlock + threadIdx.x, IntC<1>{});
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
          const uint32_t e = (r + u) * kBlock + threadIdx.x;
          double e0, e1;
          energies(e, &e0, &e1);
          body(tile + e, x[u], e0, e1, IntC<1>{});
        }
      }
    } else {
      for (uint32_t e = threadIdx.x; e < elems; e += kBlock) {
        double e0, e1;
        energies(e, &e0, &e1);
        body(tile + e, load(tile + e, IntC<0>{}), e0, e1, IntC<0>{});
      }
    }
    __syncthreads();  // the table is rewritten for the next tile
  }
}

// ---- psi[j] <- exp(-i E^(j)) psi[j] (qipx_state_apply_diagonal) --------------------------------------------------------------------
// (c, s) = (cos E^, sin E^) in double, rounded once to T; re' = fl(fl(c re) + fl(s im)), im' = fl(fl(c im) - fl(s re)), never fused
// (the file is compiled with contraction off), no special case for zeros.  Every amplitude is read once and written once.
template <typename T>
__device__ __forceinline__ void diag_turn(double e, T& re, T& im) {
  double sd, cd;
  sincos(e, &sd, &cd);
  const T c = (T)cd, s = (T)sd;
  const T r = c * re + s * im, i = c * im - s * re;
  re = r, im = i;
}

template <typename T, typename E = amp_t<T>>
__global__ __launch_bounds__(kBlock) void k_diag_phase(E* __restrict__ st, DiagSumDesc d) {
  constexpr bool PACKED = !SameT<E, amp_t<T>>::v;
  __shared__ double tab[kDiagTableSize];
  diag_walk<E, PACKED>(
      st, d, tab, [](E* p, auto streaming) { return pauli_get<decltype(streaming)::v != 0>(p); },
      [](E* p, E x, double e0, double e1, auto streaming) {
        T re = x.x, im = x.y;
        diag_turn<T>(e0, re, im);
        x.x = re, x.y = im;
        if constexpr (PACKED) {
          T re1 = x.z, im1 = x.w;
          diag_turn<T>(e1, re1, im1);
          x.z = re1, x.w = im1;
        }
        pauli_put<decltype(streaming)::v != 0>(x, p);
      });
}

// ---- sum_j |psi_j|^2 E^(j) and sum_j |psi_j|^2 E^(j)^2 (qipx_state_expect_diagonal) --------------------------------------------------
// Everything in double, f32 widened first: p = fl(fl(re re) + fl(im im)); the lane adds fl(p E^) and fl(fl(p E^) E^) to its two
// running sums, in the order of the walk (tile after tile, row after row, the lower half of a packed element first); then wave,
// block: partial[blockIdx.x] and partial[gridDim.x + blockIdx.x].  No atomics.
template <typename T, typename E = amp_t<T>>
__global__ __launch_bounds__(kBlock) void k_diag_moments(const E* __restrict__ st, DiagSumDesc d, double* __restrict__ partial) {
  constexpr bool PACKED = !SameT<E, amp_t<T>>::v;
  __shared__ double tab[kDiagTableSize];
  __shared__ double smem[kBlock / 64];
  double s1 = 0.0, s2 = 0.0;
  auto add = [&](double re, double im, double e) {
    const double p = re * re + im * im;
    const double pe = p * e;
    s1 += pe;
    s2 += pe * e;
  };
  diag_walk<E, PACKED>(
      st, d, tab, [](const E* p, auto streaming) { return pauli_get<decltype(streaming)::v != 0>(p); },
      [&](const E*, E x, double e0, double e1, auto) {
        add(x.x, x.y, e0);
        if constexpr (PACKED) add(x.z, x.w, e1);
      });
  const double t1 = block_reduce_sum(s1, smem);
  const double t2 = block_reduce_sum(s2, smem);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = t1;
    partial[gridDim.x + blockIdx.x] = t2;
  }
}

}  // namespace qipk
