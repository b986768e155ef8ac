// qip_pauli_kernels.h — the device side of the Pauli-string calls and of the vector arithmetic of resident states (qip_pauli.hip,
// the only unit that includes this; include/qip_hipx.h): k_expect_pauli, k_pauli_rotate, k_pauli_sum, k_pauli_melem over ONE walk
// of a block's chunk (pauli_walk), and k_lincomb, k_inner_many.  Never compiled at run time.
#pragma once
#include "qip_kernels.h"
#include "qip_pauli_plan.h"

namespace qipk {

static_assert(kPauliStrideShift == (uint32_t)kStrideShift, "pauli_geom's span is one round of pauli_walk's main loop");

// ---- the walk of a pass -----------------------------------------------------------------------------------------------------
// All terms of a pass share the x mask, so they share the loads; what differs per term (slot) is one sign bit per amplitude,
// sigma_j = (-1)^popcount(j & z).  The z masks arrive TRANSPOSED (PauliMasks::col): the sign bits of all slots at work index w are
// the XOR of col[b] over the set bits b of w — work that grows with the index width, not with the number of terms, and everything
// above the lane id is wave-uniform (scalar unit).  A lane's low 8 work-index bits are its id throughout, so its own share of the
// signs (pauli_lane_signs) is the same for every work item it visits.
// The XOR of col[b] over the set bits of `v`, whose bit 0 is work-index bit `b` ...
__device__ __forceinline__ uint32_t pauli_fold(const uint32_t (&col)[64], uint64_t v, uint32_t b) {
  uint32_t m = 0;
  for (; v; v >>= 1, ++b)
    if (v & 1ull) m ^= col[b];
  return m;
}
// ... and a lane's own share of it: its id is the low 8 bits of every work index it visits
__device__ __forceinline__ uint32_t pauli_lane_signs(const uint32_t (&col)[64]) {
  uint32_t m = 0;
#pragma unroll
  for (int b = 0; b < 8; ++b) m ^= ((threadIdx.x >> b) & 1u) ? col[b] : 0u;
  return m;
}

// A block takes `chunk` contiguous work items of `nwork` (pauli_geom): whole spans of U << kStrideShift items in rows of 256 with
// U accesses per lane 32 KiB apart (k_chunk_norms' shape; U = four 16-byte loads in flight per lane and vector: 2 pairs or 4
// single elements), then the tail in rows of 256.  Work item w is the element j = w (x = 0) or the pair (j, j ^ x), j = w with a
// zero inserted at x's highest bit (`ins`).  `body` is called
//   once per row of a span:  body(IntC<U>, j[U], signs, streaming = IntC<1>)
//   once per tail row:       body(IntC<1>, j[1], signs, streaming = IntC<0>)   (lanes past the end make no call)
// with signs(u) = seed ^ the wave-uniform share of the sign bits at j[u] (of its lower half, when packed).  A kernel that sums
// seeds with its own sign word and applies the lane's share once, to the finished sum (negation commutes with rounding); one that
// stores seeds with pauli_lane_signs.  `streaming` asks for non-temporal accesses (pauli_get, pauli_put).
// `signs` is a callable, to be called where the word is used, after the row's loads are issued: handed over as U values computed
// in front of the loads, the sign words stay live across them and k_expect_pauli<float, 16, false, f32x4>,
// k_pauli_rotate<T, 32, false> and k_pauli_melem<float, 16, false, f32x4> lose a wave or two per SIMD (profiles/pauli_unit.md).
template <bool PAIR, typename F>
__device__ __forceinline__ void pauli_walk(uint64_t nwork, uint64_t chunk, const Ins& ins, const uint32_t (&col)[64], uint32_t seed,
                                           F&& body) {
  constexpr int LOGU = PAIR ? 1 : 2, U = 1 << LOGU;
  constexpr uint64_t kSpan = (uint64_t)U << kStrideShift;
  auto index_of = [&](uint64_t w) { return PAIR ? insert_bits<1>(w, ins) : w; };
  const uint64_t lo = (uint64_t)blockIdx.x * chunk;
  const uint64_t hi = lo + chunk < nwork ? lo + chunk : nwork;
  uint64_t i = lo;  // (a multiple of 256 throughout: the lane id is the work index's low 8 bits)
  for (; i + kSpan <= hi; i += kSpan) {
    const uint32_t span_signs = pauli_fold(col, i >> (kStrideShift + LOGU), kStrideShift + LOGU);
#pragma unroll 1
    for (uint32_t qrow = 0; qrow < (1u << (kStrideShift - 8)); ++qrow) {
      const uint64_t w0 = i + (uint64_t)qrow * kBlock + threadIdx.x;
      const uint32_t row_signs = span_signs ^ pauli_fold(col, qrow, 8) ^ seed;  // (the seed last: it may be a lane's own)
      uint64_t j[U];
#pragma unroll
      for (int u = 0; u < U; ++u) j[u] = index_of(w0 + ((uint64_t)u << kStrideShift));
      body(IntC<U>{}, j, [&](int u) { return row_signs ^ pauli_fold(col, u, kStrideShift); }, IntC<1>{});
    }
  }
  for (; i < hi; i += kBlock) {
    const uint64_t w = i + threadIdx.x;
    if (w < hi) {
      const uint64_t j[1] = {index_of(w)};
      body(IntC<1>{}, j, [&](int) { return seed ^ pauli_fold(col, i >> 8, 8); }, IntC<0>{});
    }
  }
}
// (a compile-time choice: under a run-time flag the two loads are merged into one plain load before the flag is known)
template <bool STREAMING, typename E> __device__ __forceinline__ E pauli_get(const E* p) {
  if constexpr (STREAMING) return __builtin_nontemporal_load(p);
  else return *p;
}
template <bool STREAMING, typename E> __device__ __forceinline__ void pauli_put(E v, E* p) {
  if constexpr (STREAMING) __builtin_nontemporal_store(v, p);
  else *p = v;
}

__device__ __forceinline__ float flip_sign(float v, uint32_t bit) { return __uint_as_float(__float_as_uint(v) ^ (bit << 31)); }
__device__ __forceinline__ double flip_sign(double v, uint32_t bit) {
  return __longlong_as_double(__double_as_longlong(v) ^ (long long)((uint64_t)bit << 63));
}

// ---- expectation values of Pauli strings (qipx_state_expect_pauli, include/qip_hipx.h) -----------------------------------
// <psi|P|psi> = sum_j conj(psi[j ^ x]) i^nY (-1)^popcount(j & z) psi[j]; the terms of j and j ^ x are conjugates, so a pass
// walks the pairs and adds, per term, +-Re c or +-Im c of c = conj(psi[j ^ x]) psi[j] (the host doubles the sum).  x = 0
// (PAIR = false): every amplitude by itself, c = |psi[j]|^2.  Per term: one sign bit per pair and the choice among +-Re, +-Im:
//   flip   bit g: term g adds -(...)   (nY mod 4 = 1: -Im c, 2: -Re c): the walk's seed
//   imag   bit g: term g takes Im c    (nY odd)
// The running sums are kept with the wave-uniform share of the sign only (the sign word comes from a scalar register) and the
// lane's share is applied once, to the finished sum — the bits are those of signing every addend.  Per pair and term the vector
// unit is left with: flip, pick Re / Im, add.  Everything is widened to double before the first product.  Slot g's running sum
// sees the same addends in the same order for every capacity G and whatever the other slots hold: the value of a term does not
// depend on its company.  A block writes partial[g * gridDim.x + blockIdx.x] for g < count; no atomics.
struct ExpectDesc : PauliMasks {
  uint32_t flip, imag;
};

template <typename T, int G, bool PAIR, typename E = amp_t<T>>
__global__ __launch_bounds__(kBlock) void k_expect_pauli(const E* __restrict__ st, uint64_t nwork, uint64_t chunk, Ins ins,
                                                         ExpectDesc d, double* __restrict__ partial) {
  constexpr bool PACKED = !SameT<E, amp_t<T>>::v;
  __shared__ double smem[kBlock / 64];
  double acc[G];
#pragma unroll
  for (int g = 0; g < G; ++g) acc[g] = 0.0;
  auto add = [&](uint32_t signs, double cr, double ci) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const double v = (PAIR && ((d.imag >> g) & 1u)) ? ci : cr;
      const uint64_t sign = (uint64_t)((signs >> g) & 1u) << 63;
      acc[g] += __longlong_as_double(__double_as_longlong(v) ^ (long long)sign);
    }
  };
  // a = the element at j, b = the element at j ^ x; `signs` = the wave-uniform share of the terms' sign bits at j (its lower
  // half, when packed)
  auto take = [&](uint32_t signs, E a, E b) {
    if constexpr (PACKED) {
      const double ax = a.x, ay = a.y, az = a.z, aw = a.w;
      if constexpr (PAIR) {
        const double bx = b.x, by = b.y, bz = b.z, bw = b.w;
        add(signs, bx * ax + by * ay, bx * ay - by * ax);
        add(signs ^ d.half, bz * az + bw * aw, bz * aw - bw * az);
      } else {
        add(signs, ax * ax + ay * ay, 0.0);
        add(signs ^ d.half, az * az + aw * aw, 0.0);
      }
    } else {
      const double ax = a.x, ay = a.y;
      if constexpr (PAIR) {
        const double bx = b.x, by = b.y;
        add(signs, bx * ax + by * ay, bx * ay - by * ax);
      } else {
        add(signs, ax * ax + ay * ay, 0.0);
      }
    }
  };
  pauli_walk<PAIR>(nwork, chunk, ins, d.col, d.flip, [&](auto nelem, const uint64_t* j, auto signs, auto streaming) {
    constexpr int N = decltype(nelem)::v;
    constexpr bool NT = decltype(streaming)::v != 0;
    E a[N], b[N];
#pragma unroll
    for (int u = 0; u < N; ++u) {
      a[u] = pauli_get<NT>(st + j[u]);
      if constexpr (PAIR) b[u] = pauli_get<NT>(st + (j[u] ^ d.x));
      else b[u] = a[u];
    }
#pragma unroll
    for (int u = 0; u < N; ++u) take(signs(u), a[u], b[u]);
  });
  const uint32_t lane_signs = pauli_lane_signs(d.col);
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const double t = block_reduce_sum(((lane_signs >> g) & 1u) ? -acc[g] : acc[g], smem);
    if (threadIdx.x == 0 && (uint32_t)g < d.count) partial[(uint64_t)g * gridDim.x + blockIdx.x] = t;
  }
}

// ---- Pauli-string rotations exp(-i theta P) in place (qipx_state_apply_pauli_rotations, include/qip_hipx.h) -----------------
// exp(-i theta P) = cos theta - i sin theta P mixes psi[j] with psi[j ^ x] only, so a pass keeps a pair in registers, sends it
// through the pass's slots one after the other — consecutive terms of one x mask, in term order — and stores it: every amplitude
// is read once and written once, by the one lane that owns its pair; no LDS, no atomics, no synchronisation.  Slot g, with c = cos
// theta_g, s = sin theta_g rounded once to T on the host, p = (n_Y + 3) mod 4 (-i i^n_Y = i^p) and sigma_m = (-1)^popcount(m & z):
//   psi'[j] = c psi[j] + s i^p sigma_{j^x} psi[j ^ x],     psi'[j ^ x] = c psi[j ^ x] + s i^p sigma_j psi[j],
// i^p and sigma a swap and sign flips of components (exact), every new component fl(fl(c u) + fl(s v)), never fused (the file
// is compiled with contraction off).  sigma_j comes from the walk, seeded with the lane's share (the pair is written, not
// summed); sigma_{j^x} = sigma_j (-1)^n_Y.
//   swap   bit g: p odd — the partner's components change places
//   hi     bit g: p >= 2
//   odd    bit g: n_Y odd
// Slots >= count are skipped, not multiplied through with c = 1, s = 0 (that would turn -0 into +0 and 0 * inf into NaN).  A slot
// does the same operations on the same values whatever the capacity G and whatever its company: any grouping leaves the same bits.
template <typename T> struct RotateDesc : PauliMasks {
  uint32_t swap, hi, odd;
  T c[kRotateMaxGroup], s[kRotateMaxGroup];
};

// one amplitude's components through one slot: (ur, ui) <- c (ur, ui) + s i^P (vr, vi), `s` already signed with sigma
template <int P, typename T> __device__ __forceinline__ void pauli_mix(T c, T s, T& ur, T& ui, T vr, T vi) {
  T xr, xi;  // i^P (vr, vi): 0: (vr, vi)  1: (-vi, vr)  2: (-vr, -vi)  3: (vi, -vr); s * (-v) = (-s) * v = -(s * v), bit for bit
  if constexpr (P == 0) xr = s * vr, xi = s * vi;
  else if constexpr (P == 1) xr = -(s * vi), xi = s * vr;
  else if constexpr (P == 2) xr = -(s * vr), xi = -(s * vi);
  else xr = s * vi, xi = -(s * vr);
  ur = c * ur + xr;
  ui = c * ui + xi;
}

// K = the amplitudes a lane holds per side: U elements, twice that when packed.  Slot g on all of them; sj[k] = the sign word of
// amplitude k (bit g: sigma_j negative).  The sign goes onto s (one XOR per amplitude and side), i^P is a wave-uniform case.
template <int P, bool PAIR, int K, typename T>
__device__ __forceinline__ void pauli_slot(T c, T s, uint32_t g, uint32_t odd, const uint32_t (&sj)[K], T (&ar)[K], T (&ai)[K],
                                           T (&br)[K], T (&bi)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const uint32_t bit = (sj[k] >> g) & 1u;
    if constexpr (PAIR) {
      const T ur = ar[k], ui = ai[k];
      pauli_mix<P>(c, flip_sign(s, bit ^ odd), ar[k], ai[k], br[k], bi[k]);  // sigma_{j^x} = sigma_j (-1)^n_Y
      pauli_mix<P>(c, flip_sign(s, bit), br[k], bi[k], ur, ui);
    } else {
      pauli_mix<P>(c, flip_sign(s, bit), ar[k], ai[k], ar[k], ai[k]);
    }
  }
}

template <typename T, int G, bool PAIR, typename E = amp_t<T>>
__global__ __launch_bounds__(kBlock) void k_pauli_rotate(E* __restrict__ st, uint64_t nwork, uint64_t chunk, Ins ins, RotateDesc<T> d) {
  constexpr bool PACKED = !SameT<E, amp_t<T>>::v;
  // N elements a (at j) and b (at j ^ x) through all slots in term order; signs[u] = the sign bits of sigma_j per slot for element
  // u (of its lower half, when packed).  Capacities 1 and 4 are unrolled; the largest walks the slots in use in a loop (the
  // unrolled body of 32 slots does not fit the instruction cache), a slot's numbers coming from the descriptor by scalar loads.
  auto turn = [&](auto nelem, const uint32_t* signs, E* a, E* b) {
    constexpr int N = decltype(nelem)::v, K = PACKED ? 2 * N : N;
    T ar[K], ai[K], br[K], bi[K];
    uint32_t sj[K];
#pragma unroll
    for (int u = 0; u < N; ++u) {
      ar[u] = a[u].x, ai[u] = a[u].y, sj[u] = signs[u];
      br[u] = PAIR ? b[u].x : T(0), bi[u] = PAIR ? b[u].y : T(0);
      if constexpr (PACKED) {
        ar[N + u] = a[u].z, ai[N + u] = a[u].w, sj[N + u] = signs[u] ^ d.half;
        br[N + u] = PAIR ? b[u].z : T(0), bi[N + u] = PAIR ? b[u].w : T(0);
      }
    }
    auto one = [&](uint32_t g) {
      const T c = d.c[g], s = d.s[g];
      const uint32_t odd = (d.odd >> g) & 1u;
      switch (((d.swap >> g) & 1u) | (((d.hi >> g) & 1u) << 1)) {
        case 0: pauli_slot<0, PAIR, K>(c, s, g, odd, sj, ar, ai, br, bi); break;
        case 1: pauli_slot<1, PAIR, K>(c, s, g, odd, sj, ar, ai, br, bi); break;
        case 2: pauli_slot<2, PAIR, K>(c, s, g, odd, sj, ar, ai, br, bi); break;
        default: pauli_slot<3, PAIR, K>(c, s, g, odd, sj, ar, ai, br, bi); break;
      }
    };
    if constexpr (G <= 4) {
#pragma unroll
      for (int g = 0; g < G; ++g)
        if ((uint32_t)g < d.count) one(g);
    } else {
#pragma unroll 1
      for (uint32_t g = 0; g < d.count; ++g) one(g);
    }
#pragma unroll
    for (int u = 0; u < N; ++u) {
      a[u].x = ar[u], a[u].y = ai[u];
      if constexpr (PAIR) b[u].x = br[u], b[u].y = bi[u];
      if constexpr (PACKED) {
        a[u].z = ar[N + u], a[u].w = ai[N + u];
        if constexpr (PAIR) b[u].z = br[N + u], b[u].w = bi[N + u];
      }
    }
  };
  // (four 16-byte loads in flight per lane before the first store)
  pauli_walk<PAIR>(nwork, chunk, ins, d.col, pauli_lane_signs(d.col), [&](auto nelem, const uint64_t* j, auto signs, auto streaming) {
    constexpr int N = decltype(nelem)::v;
    constexpr bool NT = decltype(streaming)::v != 0;
    E a[N], b[N];
#pragma unroll
    for (int u = 0; u < N; ++u) {
      a[u] = pauli_get<NT>(st + j[u]);
      if constexpr (PAIR) b[u] = pauli_get<NT>(st + (j[u] ^ d.x));
      else b[u] = a[u];
    }
    uint32_t sj[N];
#pragma unroll
    for (int u = 0; u < N; ++u) sj[u] = signs(u);
    turn(nelem, sj, a, b);
#pragma unroll
    for (int u = 0; u < N; ++u) {
      pauli_put<NT>(a[u], st + j[u]);
      if constexpr (PAIR) pauli_put<NT>(b[u], st + (j[u] ^ d.x));
    }
  });
}

// ---- a Pauli sum applied to a second state: dst (+)= (sum_t c_t P_t) src (qipx_state_apply_pauli_sum, include/qip_hipx.h) -------
// (P src)[j] = i^n_Y sigma_{j^x} src[j ^ x] has one partner per amplitude, so the terms of one x mask share a pass: the lane that
// owns the pair (j, j ^ x) loads both source amplitudes, forms for each of them the signed coefficient sum
//   w(j) = sum_g sigma_g(j ^ x) k_g,     w(j ^ x) = sum_g sigma_g(j) k_g,     k_g = c_g i^n_Y,g rounded once to T on the host,
// slot after slot in term order starting from +0 (a sign flip and an add per component, slot and amplitude), then one complex
// product per amplitude, re = fl(fl(wr sr) - fl(wi si)), im = fl(fl(wr si) + fl(wi sr)), never fused, and stores it (FIRST: the
// destination is not read) or adds it to the destination's amplitude, one rounding per component.  src is read once, dst read
// and written once; no LDS, no atomics.  sigma_j comes from the walk as in k_pauli_rotate, sigma_{j^x} = sigma_j (-1)^n_Y.
//   odd    bit g: n_Y odd
template <typename T> struct SumDesc : PauliMasks {
  uint32_t odd;
  T kr[kSumMaxGroup], ki[kSumMaxGroup];
};

// (dr, di) <- [FIRST ? 0 : (dr, di)] + (wr, wi) * (sr, si)
template <bool FIRST, typename T> __device__ __forceinline__ void pauli_sum_put(T wr, T wi, T sr, T si, T& dr, T& di) {
  const T pr = wr * sr - wi * si, pi = wr * si + wi * sr;
  dr = FIRST ? pr : dr + pr;
  di = FIRST ? pi : di + pi;
}

template <typename T, int G, bool PAIR, bool FIRST, typename E = amp_t<T>>
__global__ __launch_bounds__(kBlock) void k_pauli_sum(E* __restrict__ dst, const E* __restrict__ src, uint64_t nwork, uint64_t chunk,
                                                      Ins ins, SumDesc<T> d) {
  constexpr bool PACKED = !SameT<E, amp_t<T>>::v;
  // N source elements a (at j) and b (at j ^ x) into the destination elements da (at j) and db (at j ^ x); signs[u] = the sign
  // bits of sigma_j per slot for element u (of its lower half, when packed).  Capacities 1 and 4 are unrolled, the largest walks
  // the slots in use in a loop, a slot's coefficient coming from the descriptor by scalar loads (as k_pauli_rotate does).
  auto turn = [&](auto nelem, const uint32_t* signs, const E* a, const E* b, E* da, E* db) {
    constexpr int N = decltype(nelem)::v, K = PACKED ? 2 * N : N;
    uint32_t sj[K];
    T wbr[K], wbi[K], war[K], wai[K];  // wb: sum of sigma_g(j) k_g, for the amplitude at j ^ x (at j when x = 0); wa: for the one at j
#pragma unroll
    for (int k = 0; k < K; ++k) {
      sj[k] = k < N ? signs[k] : signs[k - N] ^ d.half;
      wbr[k] = wbi[k] = war[k] = wai[k] = T(0);
    }
    auto one = [&](uint32_t g) {
      const T kr = d.kr[g], ki = d.ki[g];
      const uint32_t odd = (d.odd >> g) & 1u;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const uint32_t bit = (sj[k] >> g) & 1u;
        wbr[k] += flip_sign(kr, bit), wbi[k] += flip_sign(ki, bit);
        if constexpr (PAIR) war[k] += flip_sign(kr, bit ^ odd), wai[k] += flip_sign(ki, bit ^ odd);
      }
    };
    if constexpr (G <= 4) {
#pragma unroll
      for (int g = 0; g < G; ++g)
        if ((uint32_t)g < d.count) one(g);
    } else {
#pragma unroll 1
      for (uint32_t g = 0; g < d.count; ++g) one(g);
    }
    // one amplitude: d <- [d +] w * s through scalars (a vector's component does not bind to a reference)
    auto put = [&](T wr, T wi, T sr, T si, T dr, T di, T* outr, T* outi) {
      pauli_sum_put<FIRST>(wr, wi, sr, si, dr, di);
      *outr = dr, *outi = di;
    };
#pragma unroll
    for (int u = 0; u < N; ++u) {
      T r0, i0, r1 = T(0), i1 = T(0);
      if constexpr (PAIR) {
        put(war[u], wai[u], b[u].x, b[u].y, da[u].x, da[u].y, &r0, &i0);
        if constexpr (PACKED) put(war[N + u], wai[N + u], b[u].z, b[u].w, da[u].z, da[u].w, &r1, &i1);
        da[u].x = r0, da[u].y = i0;
        if constexpr (PACKED) da[u].z = r1, da[u].w = i1;
        put(wbr[u], wbi[u], a[u].x, a[u].y, db[u].x, db[u].y, &r0, &i0);
        if constexpr (PACKED) put(wbr[N + u], wbi[N + u], a[u].z, a[u].w, db[u].z, db[u].w, &r1, &i1);
        db[u].x = r0, db[u].y = i0;
        if constexpr (PACKED) db[u].z = r1, db[u].w = i1;
      } else {
        put(wbr[u], wbi[u], a[u].x, a[u].y, da[u].x, da[u].y, &r0, &i0);
        if constexpr (PACKED) put(wbr[N + u], wbi[N + u], a[u].z, a[u].w, da[u].z, da[u].w, &r1, &i1);
        da[u].x = r0, da[u].y = i0;
        if constexpr (PACKED) da[u].z = r1, da[u].w = i1;
      }
    }
  };
  // (k_pauli_rotate's loads in flight for the source)
  pauli_walk<PAIR>(nwork, chunk, ins, d.col, pauli_lane_signs(d.col), [&](auto nelem, const uint64_t* j, auto signs, auto streaming) {
    constexpr int N = decltype(nelem)::v;
    constexpr bool NT = decltype(streaming)::v != 0;
    E a[N], b[N], da[N], db[N];
#pragma unroll
    for (int u = 0; u < N; ++u) {
      a[u] = pauli_get<NT>(src + j[u]);
      if constexpr (PAIR) b[u] = pauli_get<NT>(src + (j[u] ^ d.x));
      else b[u] = a[u];
      if constexpr (!FIRST) {
        da[u] = pauli_get<NT>(dst + j[u]);
        if constexpr (PAIR) db[u] = pauli_get<NT>(dst + (j[u] ^ d.x));
      }
    }
    uint32_t sj[N];
#pragma unroll
    for (int u = 0; u < N; ++u) sj[u] = signs(u);
    turn(nelem, sj, a, b, da, db);
#pragma unroll
    for (int u = 0; u < N; ++u) {
      pauli_put<NT>(da[u], dst + j[u]);
      if constexpr (PAIR) pauli_put<NT>(db[u], dst + (j[u] ^ d.x));
    }
  });
}

// ---- Pauli matrix elements between two states: <bra| P_t |ket> (qipx_state_pauli_matrix_elements, include/qip_hipx.h) --------
// sum_j conj(bra[j]) i^n_Y sigma_{j^x} ket[j ^ x], the terms of one x mask in one pass over both vectors.  The two members of a
// pair (j, j ^ x) give
//   sigma_{j^x} A + sigma_j B = sigma_j ((-1)^n_Y A + B),     A = conj(bra[j]) ket[j ^ x],     B = conj(bra[j ^ x]) ket[j],
// so a pair costs two complex products, S = B + A and D = B - A once, and per slot a choice (n_Y odd: D), a sign and one complex
// add to the slot's running sum; x = 0 takes conj(bra[j]) ket[j].  i^n_Y is applied by the host to the finished sum (exact).
// Everything is widened to double before the first product.  The signs are handled as in k_expect_pauli (wave-uniform share per
// addend, the lane's share once at the end), and as there a slot sees the same addends in the same order for every capacity G
// and whatever its company.  partial[(2 g + c) * gridDim.x + blockIdx.x], c = 0 the real and 1 the imaginary part; no atomics.
struct MelemDesc : PauliMasks {
  uint32_t odd;  // bit g: n_Y odd
};

template <typename T, int G, bool PAIR, typename E = amp_t<T>>
__global__ __launch_bounds__(kBlock) void k_pauli_melem(const E* __restrict__ bra, const E* __restrict__ ket, uint64_t nwork,
                                                        uint64_t chunk, Ins ins, MelemDesc d, double* __restrict__ partial) {
  constexpr bool PACKED = !SameT<E, amp_t<T>>::v;
  __shared__ double smem[kBlock / 64];
  double accr[G], acci[G];
#pragma unroll
  for (int g = 0; g < G; ++g) accr[g] = acci[g] = 0.0;
  // one amplitude pair: (pr, pi) = bra at j, (qr, qi) = bra at j ^ x, (ar, ai) = ket at j, (br, bi) = ket at j ^ x
  auto add = [&](uint32_t signs, double pr, double pi, double qr, double qi, double ar, double ai, double br, double bi) {
    double sr, si, dr = 0.0, di = 0.0;
    if constexpr (PAIR) {
      const double Ar = pr * br + pi * bi, Ai = pr * bi - pi * br;  // conj(bra[j]) ket[j ^ x]
      const double Br = qr * ar + qi * ai, Bi = qr * ai - qi * ar;  // conj(bra[j ^ x]) ket[j]
      sr = Br + Ar, si = Bi + Ai, dr = Br - Ar, di = Bi - Ai;
    } else {
      sr = pr * ar + pi * ai, si = pr * ai - pi * ar;
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const bool odd = PAIR && ((d.odd >> g) & 1u);
      const uint64_t sign = (uint64_t)((signs >> g) & 1u) << 63;
      accr[g] += __longlong_as_double(__double_as_longlong(odd ? dr : sr) ^ (long long)sign);
      acci[g] += __longlong_as_double(__double_as_longlong(odd ? di : si) ^ (long long)sign);
    }
  };
  // p = bra at j, q = bra at j ^ x, a = ket at j, b = ket at j ^ x; `signs` = the wave-uniform share of the sign bits at j
  auto take = [&](uint32_t signs, E p, E q, E a, E b) {
    add(signs, p.x, p.y, q.x, q.y, a.x, a.y, b.x, b.y);
    if constexpr (PACKED) add(signs ^ d.half, p.z, p.w, q.z, q.w, a.z, a.w, b.z, b.w);
  };
  pauli_walk<PAIR>(nwork, chunk, ins, d.col, 0u, [&](auto nelem, const uint64_t* j, auto signs, auto streaming) {
    constexpr int N = decltype(nelem)::v;
    constexpr bool NT = decltype(streaming)::v != 0;
    E p[N], q[N], a[N], b[N];
#pragma unroll
    for (int u = 0; u < N; ++u) {
      p[u] = pauli_get<NT>(bra + j[u]);
      a[u] = pauli_get<NT>(ket + j[u]);
      if constexpr (PAIR) {
        q[u] = pauli_get<NT>(bra + (j[u] ^ d.x));
        b[u] = pauli_get<NT>(ket + (j[u] ^ d.x));
      } else {
        q[u] = p[u], b[u] = a[u];
      }
    }
#pragma unroll
    for (int u = 0; u < N; ++u) {
      take(signs(u), p[u], q[u], a[u], b[u]);
      // pairs: one element after the other.  Left to itself the scheduler interleaves the row's elements, S and D of each live
      // side by side: 18 to 72 more VGPRs at G = 16 and one or two waves per SIMD fewer (profiles/pauli_unit.md)
      if constexpr (PAIR) __builtin_amdgcn_sched_barrier(0);
    }
  });
  const uint32_t lane_signs = pauli_lane_signs(d.col);
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const bool neg = (lane_signs >> g) & 1u;
    const double tr = block_reduce_sum(neg ? -accr[g] : accr[g], smem);
    const double ti = block_reduce_sum(neg ? -acci[g] : acci[g], smem);
    if (threadIdx.x == 0 && (uint32_t)g < d.count) {
      partial[(uint64_t)(2 * g) * gridDim.x + blockIdx.x] = tr;
      partial[(uint64_t)(2 * g + 1) * gridDim.x + blockIdx.x] = ti;
    }
  }
}

// ---- vector arithmetic of resident states: dst <- sum_i c_i src_i and <bra_i|ket> (qipx_state_linear_combination,
// qipx_state_inner_products, include/qip_hipx.h) -------------------------------------------------------------------------------
// Elementwise grid-stride passes over 16-byte elements (one Complex<f64>, or two packed Complex<f32>: n >= 1, so a Complex<f32>
// state is a whole number of them).  The source pointers travel by value in the descriptor, as SumDesc's coefficients do; slot g
// of a capacity G is compiled in and skipped by a wave-uniform test when g >= count.  A lane keeps the G loads of an element in
// flight together (U elements of them when G is small: U * G >= 4 loads, k_chunk_norms' depth), then does the arithmetic, then
// stores: every source is read at j before j is stored, so `dst` may be any of the sources and no pointer is __restrict__.
// The grid depends on the number of elements only (vec_grid on the host) and a lane meets its elements in ascending order
// whatever U is, so every sum below has ONE order per n and precision.
constexpr int kVecMax = 16;
template <typename T> struct LincombDesc {
  const void* src[kVecMax];
  T cr[kVecMax], ci[kVecMax];  // c_i, rounded once to T on the host
  uint32_t count;              // slots in use
};
struct InnerDesc {
  const void* bra[kVecMax];
  uint32_t count;
};
constexpr int vec_unroll(int loads) { return loads >= 4 ? 1 : 4 / loads; }

// acc <- [FIRST ? 0 : acc] + c * s per component: two products, one difference / sum, one add, never fused
template <bool FIRST, typename T> __device__ __forceinline__ void lincomb_put(T cr, T ci, T sr, T si, T& ar, T& ai) {
  const T pr = cr * sr - ci * si, pi = cr * si + ci * sr;
  ar = FIRST ? pr : ar + pr;
  ai = FIRST ? pi : ai + pi;
}

// dst[j] <- sum_{g < count} c_g src_g[j]: acc = p_0, then acc = fl(acc + p_g) in slot order.  NORM: partial[blockIdx.x] = the
// block's share of sum_j |dst[j]|^2 of the STORED values, widened to double before the squares (k_pauli_melem's scheme: lane,
// wave, block, one partial per block; no atomics).
template <typename T, int G, bool NORM, typename E = amp_t<T>>
__global__ __launch_bounds__(kBlock) void k_lincomb(E* dst, uint64_t nelems, LincombDesc<T> d, double* __restrict__ partial) {
  constexpr bool PACKED = !SameT<E, amp_t<T>>::v;
  constexpr int U = vec_unroll(G);
  __shared__ double smem[kBlock / 64];
  double s = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i0 = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i0 < nelems; i0 += U * stride) {
    E x[U][G];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int g = 0; g < G; ++g)
        if ((uint32_t)g < d.count && i0 + u * stride < nelems)
          x[u][g] = __builtin_nontemporal_load((const E*)d.src[g] + (i0 + u * stride));
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint64_t i = i0 + u * stride;
      if (i < nelems) {
        T r0 = T(0), i0_ = T(0), r1 = T(0), i1 = T(0);
        lincomb_put<true>(d.cr[0], d.ci[0], x[u][0].x, x[u][0].y, r0, i0_);
        if constexpr (PACKED) lincomb_put<true>(d.cr[0], d.ci[0], x[u][0].z, x[u][0].w, r1, i1);
#pragma unroll
        for (int g = 1; g < G; ++g)
          if ((uint32_t)g < d.count) {
            lincomb_put<false>(d.cr[g], d.ci[g], x[u][g].x, x[u][g].y, r0, i0_);
            if constexpr (PACKED) lincomb_put<false>(d.cr[g], d.ci[g], x[u][g].z, x[u][g].w, r1, i1);
          }
        E out;
        out.x = r0, out.y = i0_;
        if constexpr (PACKED) out.z = r1, out.w = i1;
        __builtin_nontemporal_store(out, dst + i);
        if constexpr (NORM) {
          s += (double)r0 * (double)r0 + (double)i0_ * (double)i0_;
          if constexpr (PACKED) s += (double)r1 * (double)r1 + (double)i1 * (double)i1;
        }
      }
    }
  }
  if constexpr (NORM) {
    const double t = block_reduce_sum(s, smem);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
  }
}

// partial[(2 g + c) * gridDim.x + blockIdx.x], c = 0 the real and 1 the imaginary part of the block's share of
// sum_j conj(bra_g[j]) ket[j]: everything widened to double before the first product, re = fl(fl(pr ar) + fl(pi ai)),
// im = fl(fl(pr ai) - fl(pi ar)) (so bra_g == ket gives an imaginary part of exactly +0), one running complex sum per slot, which
// sees the same addends in the same order for every capacity G and whatever its company.
template <typename T, int G, typename E = amp_t<T>>
__global__ __launch_bounds__(kBlock) void k_inner_many(const E* ket, uint64_t nelems, InnerDesc d, double* __restrict__ partial) {
  constexpr bool PACKED = !SameT<E, amp_t<T>>::v;
  constexpr int U = vec_unroll(G + 1);
  __shared__ double smem[kBlock / 64];
  double accr[G], acci[G];
#pragma unroll
  for (int g = 0; g < G; ++g) accr[g] = acci[g] = 0.0;
  auto add = [&](int g, double pr, double pi, double ar, double ai) {
    accr[g] += pr * ar + pi * ai;
    acci[g] += pr * ai - pi * ar;
  };
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i0 = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i0 < nelems; i0 += U * stride) {
    E a[U], p[U][G];
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (i0 + u * stride < nelems) {
        a[u] = __builtin_nontemporal_load(ket + (i0 + u * stride));
#pragma unroll
        for (int g = 0; g < G; ++g)
          if ((uint32_t)g < d.count) p[u][g] = __builtin_nontemporal_load((const E*)d.bra[g] + (i0 + u * stride));
      }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (i0 + u * stride < nelems) {
#pragma unroll
        for (int g = 0; g < G; ++g)
          if ((uint32_t)g < d.count) {
            add(g, p[u][g].x, p[u][g].y, a[u].x, a[u].y);
            if constexpr (PACKED) add(g, p[u][g].z, p[u][g].w, a[u].z, a[u].w);
          }
      }
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const double tr = block_reduce_sum(accr[g], smem);
    const double ti = block_reduce_sum(acci[g], smem);
    if (threadIdx.x == 0 && (uint32_t)g < d.count) {
      partial[(uint64_t)(2 * g) * gridDim.x + blockIdx.x] = tr;
      partial[(uint64_t)(2 * g + 1) * gridDim.x + blockIdx.x] = ti;
    }
  }
}

}  // namespace qipk
