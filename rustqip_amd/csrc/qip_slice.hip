// qip_slice.hip — apply_op / apply_op_overwrite on DEVICE slices (qip_hip_apply_op_device): payload cache, kernels, routing.
#include "qip_internal.h"

#include <mutex>
#include <unordered_map>

// ---------------------------------------------------------------------------------------
// device-resident payloads of the slice-level calls, keyed by content
// ---------------------------------------------------------------------------------------
// An op whose payload does not fit the kernel arguments (a dense table above 64 complex / 256 real entries, every
// SparseMatrix) needs it in device memory.  qip_hip_apply_op_device has no handle to own it, so the library keeps it: one
// process-wide table, guarded by a mutex and bounded by a global option, as the run-time compiler's kernel cache is.
//   key      device, element type, op kind, n_op and the payload BYTES (the dense table, or rowptr / cols / vals).  Found by a
//            64-bit hash, confirmed by memcmp against the host copy the entry keeps: a collision never selects a wrong table,
//            and a caller who rewrites the same buffer between calls gets the new bytes (a pointer is never part of the key).
//   miss     hipMalloc + a blocking copy: not capturable.  On a capturing stream the call fails before it touches the device.
//   hit      host work only; the caller launches one kernel that reads the entry.
//   bound    option "slice_payload_cache_mb" (default 256).  A payload that would exceed it is not cached (*dev = nullptr: the
//            caller takes its per-call route, which uploads and synchronises).  Nothing is evicted — a recorded graph may still
//            read an entry; value 0 synchronises the devices involved, frees every entry and disables the cache.
struct PayloadSpan {
  const void* p;
  size_t bytes;
  size_t off;  // in the entry (16-byte aligned)
};
struct SlicePayload {
  uint64_t head[4];  // device, element type, kind (of the op, or of the device form when that is not the literal one), n_op
  PayloadSpan span[3];
  int nspans = 0;
  size_t total = 0;
  void add(const void* p, size_t bytes) {
    span[nspans++] = PayloadSpan{p, bytes, total};
    total = (total + bytes + 15) & ~(size_t)15;
  }
};
struct SliceEntry {
  int device;
  uint64_t head[4];
  size_t span_bytes[3];
  std::vector<unsigned char> host;  // the key bytes, laid out as the spans are (the device form too, unless an image was built)
  char* dev;
};
static std::mutex g_slice_mu;
static std::unordered_multimap<uint64_t, SliceEntry> g_slice_cache;
static size_t g_slice_bytes = 0;
static int64_t g_slice_cap_mb = 256;

static inline uint64_t mix64(uint64_t h, uint64_t w) {
  h = (h ^ w) * 0x9E3779B97F4A7C15ull;
  return h ^ (h >> 29);
}
static uint64_t hash_bytes(uint64_t h, const void* p, size_t bytes) {
  const unsigned char* b = (const unsigned char*)p;
  uint64_t h0 = h, h1 = ~h, h2 = h + 0x632BE59BD9B4E019ull, h3 = h ^ 0xD6E8FEB86659FD93ull;  // four chains: the multiplies overlap
  size_t i = 0;
  for (; i + 32 <= bytes; i += 32) {
    uint64_t w[4];
    memcpy(w, b + i, 32);
    h0 = mix64(h0, w[0]);
    h1 = mix64(h1, w[1]);
    h2 = mix64(h2, w[2]);
    h3 = mix64(h3, w[3]);
  }
  h = mix64(mix64(mix64(h0, h1), h2), h3);
  for (; i + 8 <= bytes; i += 8) {
    uint64_t w;
    memcpy(&w, b + i, 8);
    h = mix64(h, w);
  }
  uint64_t tail = 0;
  if (bytes > i) memcpy(&tail, b + i, bytes - i);
  return mix64(mix64(h, tail), bytes);
}

int slice_cache_set_cap_mb(int64_t mb) {
  if (mb < 0) return fail(QIP_ERR_INVALID, "slice_payload_cache_mb must be >= 0 (0 frees every entry and disables the cache)");
  std::lock_guard<std::mutex> lock(g_slice_mu);
  g_slice_cap_mb = mb;
  if (mb != 0 || g_slice_cache.empty()) return QIP_OK;
  int before = 0;
  (void)hipGetDevice(&before);
  hipError_t worst = hipSuccess;
  int synced = -1;
  for (auto& kv : g_slice_cache) {  // (entries of one device need one synchronisation: kernels that read them are behind it)
    hipError_t e = hipSetDevice(kv.second.device);
    if (e == hipSuccess && synced != kv.second.device) {
      e = hipDeviceSynchronize();
      synced = kv.second.device;
    }
    if (e == hipSuccess) e = hipFree(kv.second.dev);
    if (e != hipSuccess) worst = e;
  }
  g_slice_cache.clear();
  g_slice_bytes = 0;
  (void)hipSetDevice(before);
  if (worst != hipSuccess) {
    (void)hipGetLastError();
    return fail(QIP_ERR_DEVICE, "freeing the slice payload cache failed: %s", hipGetErrorString(worst));
  }
  return QIP_OK;
}

// *dev = the payload resident on `device` (the current one), or nullptr when it is not cached and cannot be (the bound)
// `image`: writes the device form (p.total bytes) when it is not the key bytes themselves; called on a miss only
static int slice_payload_get(int device, const SlicePayload& p, hipStream_t stream, char** dev,
                             const std::function<void(unsigned char*)>* image = nullptr) {
  *dev = nullptr;
  uint64_t h = hash_bytes(0x51C3ull, p.head, sizeof p.head);
  for (int i = 0; i < p.nspans; ++i) h = hash_bytes(h, p.span[i].p, p.span[i].bytes);
  std::lock_guard<std::mutex> lock(g_slice_mu);
  if (g_slice_cap_mb == 0) return QIP_OK;
  auto range = g_slice_cache.equal_range(h);
  for (auto it = range.first; it != range.second; ++it) {
    const SliceEntry& e = it->second;
    if (e.device != device || memcmp(e.head, p.head, sizeof p.head) != 0 || e.host.size() != p.total) continue;
    bool equal = true;
    for (int i = 0; i < p.nspans && equal; ++i)
      equal = e.span_bytes[i] == p.span[i].bytes && (p.span[i].bytes == 0 || memcmp(e.host.data() + p.span[i].off, p.span[i].p, p.span[i].bytes) == 0);
    if (equal) {
      *dev = e.dev;
      return QIP_OK;
    }
  }
  if (g_slice_bytes + p.total > ((size_t)g_slice_cap_mb << 20)) return QIP_OK;
  if (stream) {  // (the null stream cannot be captured)
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const hipError_t e = hipStreamIsCapturing(stream, &cs);
    if (e != hipSuccess || cs != hipStreamCaptureStatusNone) {
      if (e != hipSuccess) (void)hipGetLastError();
      return fail(QIP_ERR_DEVICE, "the op's payload (%zu bytes) is not on the device yet and the stream is being captured: "
                                  "issue the call once outside the capture, then it only launches", p.total);
    }
  }
  SliceEntry e;
  e.device = device;
  memcpy(e.head, p.head, sizeof p.head);
  e.host.assign(p.total, 0);
  for (int i = 0; i < 3; ++i) e.span_bytes[i] = i < p.nspans ? p.span[i].bytes : 0;
  for (int i = 0; i < p.nspans; ++i)
    if (p.span[i].bytes) memcpy(e.host.data() + p.span[i].off, p.span[i].p, p.span[i].bytes);
  e.dev = nullptr;
  HIPCHK(hipMalloc((void**)&e.dev, std::max<size_t>(p.total, 16)));
  if (p.total) {
    std::vector<unsigned char> built;
    if (image) {
      built.assign(p.total, 0);
      (*image)(built.data());
    }
    const hipError_t ce = hipMemcpy(e.dev, image ? built.data() : e.host.data(), p.total, hipMemcpyHostToDevice);  // blocking: resident when this returns
    if (ce != hipSuccess) {
      (void)hipFree(e.dev);
      (void)hipGetLastError();
      return fail(QIP_ERR_DEVICE, "uploading an op's payload failed: %s", hipGetErrorString(ce));
    }
  }
  *dev = e.dev;
  g_slice_bytes += p.total;
  g_slice_cache.emplace(h, std::move(e));
  return QIP_OK;
}

// the payload of a dense op too large for the kernel arguments or of a SparseMatrix, as the literal kernels read it:
// the dense table, or rowptr | cols | vals (each 16-byte aligned; `eb` = bytes per stored value)
static SlicePayload literal_payload(int device, int dtype, const FlatOp& f, size_t eb) {
  SlicePayload p;
  p.head[0] = (uint64_t)device;
  p.head[1] = (uint64_t)dtype;
  p.head[2] = (uint64_t)f.inner->kind;
  p.head[3] = f.n_op;
  if (f.inner->kind == QIP_OP_MATRIX) {
    p.add(f.inner->dense, eb << (2 * f.n_op));
  } else {
    const uint64_t rows = 1ull << f.n_op;
    const uint64_t nnz = f.inner->sparse_rowptr[rows];
    p.add(f.inner->sparse_rowptr, (rows + 1) * 8);
    p.add(f.inner->sparse_cols, nnz * 8);
    p.add(f.inner->sparse_vals, nnz * eb);
  }
  return p;
}
constexpr uint64_t kTransposedTableKind = 0x100;  // head[2] of a dense table stored [c][row] (k_cplx_dense_tile); no qip_op kind has this value

// ---------------------------------------------------------------------------------------
// host-side steps every route shares
// ---------------------------------------------------------------------------------------
static bool whole_vector(uint32_t n, uint64_t in_len, uint64_t out_len, uint64_t in_off, uint64_t out_off) {
  return in_off == 0 && out_off == 0 && in_len == (1ull << n) && out_len == in_len;
}
static bool aligned16(const void* a, const void* b) { return (uintptr_t)a % 16 == 0 && (uintptr_t)b % 16 == 0; }

// index position of every outer index (controls first), as the kernels order a sub-index: entry 0 = its most significant bit
static std::vector<uint32_t> index_positions(uint32_t n, const FlatOp& f) {
  std::vector<uint32_t> pos(f.k_all);
  for (uint32_t j = 0; j < f.k_all; ++j) pos[j] = (uint32_t)(n - 1 - f.outer->indices[j]);
  return pos;
}

// Tab = RealTab<R> / CplxTab<T>, for an op the caller admitted to the kernel arguments: zeroed, a dense op's entries copied in
// (a Swap travels with the zero table)
template <typename Tab> static Tab arg_table(const FlatOp& f) {
  Tab tab;
  memset(&tab, 0, sizeof tab);
  if (f.inner->kind == QIP_OP_MATRIX) memcpy(tab.v, f.inner->dense, sizeof(tab.v[0]) << (2 * f.n_op));
  return tab;
}

// A vector far beyond the caches streams (non-temporal accesses, as the state kernels' sweeps do) — only with 16-byte accesses
// and when a wave's accesses cover whole 128-byte lines, i.e. no group position within the low three positions counted in
// accesses (`lowest`: GroupGeom::lowest).  Measured at n = 28, f64, a dense op on qubits 3 and n-2 — 16-byte runs — 785 us with
// cached accesses, 1448 us with non-temporal ones.
static bool streams(uint64_t vector_bytes, bool access16, uint32_t lowest) {
  return access16 && vector_bytes >= (64ull << 20) && lowest >= 3;
}

// ---------------------------------------------------------------------------------------
// apply_op / apply_op_overwrite on DEVICE slices for any P (qip_hip_apply_op_device)
// ---------------------------------------------------------------------------------------
// qip-iterators' kernel is generic over P (matrix_ops.rs:98-107): a real or integer vector takes the same row fold as a
// complex one — acc = P::zero(); acc += val * input[col] over the iterator's columns (matrix_ops.rs:62-94, std::iter::Sum),
// then `+=` or `=` into the output row (:110 / :139).  One lane per output row, the reference's loops verbatim (index maps
// g_full_to_sub / g_sub_to_full of the complex literal kernel, the Control threshold of qubit_iterators.rs:130-169, the
// zero-skip of MatrixOpIterator :49 only), products and sums unfused (the build has -ffp-contract=off): bit-equal to the
// reference for every P.  Integers are computed in the unsigned type of their width (wrapping; the bits are two's complement).
// Algorithmic bytes per output row: sizeof(P) x (1 read of the input + 1 write, + 1 read when accumulating).
template <typename R> struct RealTab {  // a dense op on k <= 4 qubits inside the kernel arguments: no upload, no table to own
  R v[256];
};

template <typename R, int V> struct RVec { using type = R __attribute__((ext_vector_type(V))); };
template <typename R> struct RVec<R, 1> { using type = R; };

// V > 1: the lane's V consecutive rows share every index bit the op looks at (no op / control position below log2 V, windows
// and lengths multiples of V): one sub-index, one 16-byte access per term, a vector wholly inside or outside the input window
template <typename R, int V>
__device__ __forceinline__ typename RVec<R, V>::type r_term(const GatherDesc& d, uint64_t row, uint64_t col, R val, const R* __restrict__ in) {
  using X = typename RVec<R, V>::type;
  const uint64_t colbits = g_sub_to_full(d, col, row);  // matrix_ops.rs:79
  if (colbits < d.in_off) return (X)(R)0;                // :80-81
  const uint64_t vecrow = colbits - d.in_off;            // :83
  if (vecrow >= d.in_len) return (X)(R)0;                // :84-85
  return (X)val * reinterpret_cast<const X*>(in)[vecrow / V];  // :87
}

template <typename R, bool TAB, int V>
__global__ __launch_bounds__(kBlock) void k_gather_real(const R* __restrict__ in, R* __restrict__ out_, GatherDesc d,
                                                        RealTab<R> tab, const R* __restrict__ dense,
                                                        const uint64_t* __restrict__ rowptr, const uint64_t* __restrict__ cols,
                                                        const R* __restrict__ vals) {
  using X = typename RVec<R, V>::type;
  X* __restrict__ out = reinterpret_cast<X*>(out_);
  const uint64_t stride = (uint64_t)gridDim.x * kBlock, nvec = d.out_len / V;
  for (uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r < nvec; r += stride) {
    const uint64_t row = d.out_off + r * V;
    const uint64_t matrow = g_full_to_sub(d, row);
    X acc = (X)(R)0;
    uint64_t shift = 0, irow = matrow;
    bool identity_row = false;
    if (d.n_control > 0) {
      const uint64_t thr = (1ull << (d.n_control + d.n_op)) - (1ull << d.n_op);
      if (matrow >= thr) {
        shift = thr;
        irow = matrow - thr;
      } else {
        identity_row = true;
      }
    }
    if (identity_row) {
      acc = acc + r_term<R, V>(d, row, matrow, (R)1, in);
    } else if (d.inner_kind == 0) {  // MATRIX
      const uint64_t side = 1ull << d.n_op;
      for (uint64_t c = 0; c < side; ++c) {
        const R v = TAB ? tab.v[irow * side + c] : dense[irow * side + c];
        if (!(v == (R)0)) acc = acc + r_term<R, V>(d, row, c + shift, v, in);
      }
    } else if (d.inner_kind == 1) {  // SPARSE
      for (uint64_t p = rowptr[irow]; p < rowptr[irow + 1]; ++p) acc = acc + r_term<R, V>(d, row, cols[p] + shift, vals[p], in);
    } else {  // SWAP
      const uint32_t half_n = d.n_op >> 1;
      const uint64_t lower_mask = ~(~0ull << half_n);
      const uint64_t col = ((irow & lower_mask) << half_n) + (irow >> half_n);
      acc = acc + r_term<R, V>(d, row, col + shift, (R)1, in);
    }
    out[r] = d.accumulate ? (X)(out[r] + acc) : acc;
  }
}

// ---- the whole vector (both windows [0, 2^n)), a dense op or Swap on distinct qubits with k_all <= 4 indices ------------------
// One lane owns V = 16 / sizeof(P) consecutive rows of every one of the 2^K rows of a group (K = controls + op qubits; the V
// rows differ only in index bits below every op / control position): it reads each of the group's 2^K input vectors ONCE
// (16-byte accesses), folds every output row exactly as the literal kernel does — acc = 0; acc += m[row][c] * x[c] for c
// ascending, entries equal to zero skipped (the matrix sits in the kernel arguments: the skip is a scalar branch); a row outside
// the control subspace or of a Swap is 0 + 1 * x[col] — and writes 2^K output vectors.  Bit-equal to the literal kernel; HBM
// traffic = the algorithmic bytes (the literal kernel reads every input line 2^k_op times, from different lanes).
// An op with an index bit below log2(V) takes V = 1 (8- / 4-byte accesses; a 4-byte P whose lowest index bit is position 1: V = 2).
struct RealGroupDesc {
  uint64_t nitems;      // 2^n / (2^K * V)
  uint64_t off[16];     // off[m] = the index bits of sub-index m (bit K-1-j of m at position pos[j]), in units of V rows
  int32_t accumulate;
};

// The groups of one launch.  pos[0..K): the positions that form the sub-index, most significant bit first; lv: the low positions
// that live inside one access (everything is counted in accesses: positions shift down by lv).  `inside` >= 0 (the "low" form):
// pos[inside] sits inside the access — that sub-index bit adds no offset and opens no position, so ins has K - 1 entries.
struct GroupGeom {
  RealGroupDesc d;  // nitems, off[m] for every sub-index m, accumulate
  Ins ins;
  uint32_t lowest;  // the lowest group position, in accesses (64 when there is none)
};
static GroupGeom make_groups(uint32_t n, const uint32_t* pos, uint32_t K, uint32_t lv, int inside, int accumulate) {
  GroupGeom g;
  memset(&g.d, 0, sizeof g.d);
  g.d.accumulate = accumulate;
  g.lowest = 64;
  std::vector<uint32_t> opened;
  opened.reserve(K);
  for (uint32_t j = 0; j < K; ++j) {
    if ((int)j == inside) continue;
    const uint32_t at = pos[j] - lv;
    opened.push_back(at);
    g.lowest = std::min(g.lowest, at);
    for (uint32_t m = 0; m < (1u << K); ++m) g.d.off[m] |= (uint64_t)((m >> (K - 1 - j)) & 1u) << at;
  }
  g.d.nitems = 1ull << (n - opened.size() - lv);
  g.ins = make_ins(std::move(opened), 0);
  return g;
}

template <typename R, int V, int K, int NC, bool SWAP, bool NT>
__global__ __launch_bounds__(kBlock) void k_real_groups(const R* __restrict__ in, R* __restrict__ out, Ins ins, RealGroupDesc d,
                                                        RealTab<R> tab) {
  using X = typename RVec<R, V>::type;
  constexpr int M = 1 << K, KOP = K - NC, SIDE = 1 << KOP, THR = M - SIDE;
  const uint64_t w = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (w >= d.nitems) return;
  const uint64_t base = insert_bits<K>(w, ins);
  const X* inv = reinterpret_cast<const X*>(in);
  X* outv = reinterpret_cast<X*>(out);
  X x[M];
#pragma unroll
  for (int m = 0; m < M; ++m) x[m] = ldg<NT>(inv + (base | d.off[m]));
#pragma unroll
  for (int m = 0; m < M; ++m) {
    X acc = (X)(R)0;
    if (m < THR) {  // outside the control subspace: exactly one (row, 1)  (qubit_iterators.rs:160-169)
      acc = acc + (X)(R)1 * x[m];
    } else if constexpr (SWAP) {
      constexpr int HALF = KOP >> 1;
      const int irow = m - THR;
      const int col = ((irow & ((1 << HALF) - 1)) << HALF) + (irow >> HALF);
      acc = acc + (X)(R)1 * x[col + THR];
    } else {
#pragma unroll
      for (int c = 0; c < SIDE; ++c) {
        const R v = tab.v[(m - THR) * SIDE + c];
        if (!(v == (R)0)) acc = acc + (X)v * x[c + THR];
      }
    }
    const uint64_t at = base | d.off[m];
    stg<NT>(outv + at, d.accumulate ? (X)(ldg<NT>(outv + at) + acc) : acc);
  }
}

template <typename R, int V, int K, bool NT>
static int launch_real_groups_k(const FlatOp& f, const R* d_in, R* d_out, const Ins& ins, const RealGroupDesc& d, const RealTab<R>& tab,
                                hipStream_t stream) {
  const dim3 grid((unsigned)((d.nitems + kBlock - 1) / kBlock)), block(kBlock);
  const bool swap = f.inner->kind == QIP_OP_SWAP;
#define RG(NC, SW)                                                                                                       \
  hipLaunchKernelGGL((k_real_groups<R, V, K, NC, SW, NT>), grid, block, 0, stream, d_in, d_out, ins, d, tab)
  const int nc = (int)f.n_control;
  if (swap) {
    if constexpr (K == 2) { RG(0, true); }
    else if constexpr (K == 3) { RG(1, true); }
    else if constexpr (K == 4) { if (nc == 0) RG(0, true); else RG(2, true); }
  } else {
    if constexpr (K == 1) { RG(0, false); }
    else if constexpr (K == 2) { if (nc == 0) RG(0, false); else RG(1, false); }
    else if constexpr (K == 3) { if (nc == 0) RG(0, false); else if (nc == 1) RG(1, false); else RG(2, false); }
    else { if (nc == 0) RG(0, false); else if (nc == 1) RG(1, false); else if (nc == 2) RG(2, false); else RG(3, false); }
  }
#undef RG
  HIPCHK(hipGetLastError());
  return QIP_OK;
}

// ---- ... with ONE index bit inside the 16-byte vector (positions 0 / 1: an op on the last qubits) -----------------------------
// The vector then holds both values of that bit, so the group's partner rows along it sit in the SAME access: the lane reads
// 2^(K-1) vectors instead of 2^K scalars and takes them apart in registers.  MODE 0: a vector of two = the bit at position 0
// (8-byte P: 16 bytes; 4-byte P with positions 0 AND 1 in the op: 8 bytes).  4-byte P, 16-byte vectors of four: MODE 1 =
// component bit 0 is the index bit at position 0 and component bit 1 a free index bit (two independent groups per lane),
// MODE 2 = component bit 1 is the index bit at position 1, bit 0 free.  LB = which bit of the sub-index that position is.
// Same folds, same order: bit-equal to k_real_groups / the literal kernel.  K <= 3 (wider ops with a low bit: V = 1 above).
template <typename R, int K, int NC, bool SWAP, int LB, int MODE>
__global__ __launch_bounds__(kBlock) void k_real_groups_low(const R* __restrict__ in, R* __restrict__ out, Ins ins, RealGroupDesc d,
                                                            RealTab<R> tab) {
  constexpr int VW = MODE == 0 ? 2 : 4, W = VW / 2;
  using XV = typename RVec<R, VW>::type;
  using F = typename RVec<R, W>::type;
  constexpr int M = 1 << K, KOP = K - NC, SIDE = 1 << KOP, THR = M - SIDE, LOWBIT = 1 << LB;
  const uint64_t w = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (w >= d.nitems) return;
  const uint64_t base = insert_bits<K - 1>(w, ins);
  const XV* inv = reinterpret_cast<const XV*>(in);
  XV* outv = reinterpret_cast<XV*>(out);
  F x[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    if (m & LOWBIT) continue;
    const XV v = inv[base | d.off[m]];
    if constexpr (MODE == 0) {
      x[m] = v.x;
      x[m | LOWBIT] = v.y;
    } else if constexpr (MODE == 1) {
      x[m] = F{v.x, v.z};
      x[m | LOWBIT] = F{v.y, v.w};
    } else {
      x[m] = F{v.x, v.y};
      x[m | LOWBIT] = F{v.z, v.w};
    }
  }
  F o[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    F acc = (F)(R)0;
    if (m < THR) {
      acc = acc + (F)(R)1 * x[m];
    } else if constexpr (SWAP) {
      constexpr int HALF = KOP >> 1;
      const int irow = m - THR;
      const int col = ((irow & ((1 << HALF) - 1)) << HALF) + (irow >> HALF);
      acc = acc + (F)(R)1 * x[col + THR];
    } else {
#pragma unroll
      for (int c = 0; c < SIDE; ++c) {
        const R v = tab.v[(m - THR) * SIDE + c];
        if (!(v == (R)0)) acc = acc + (F)v * x[c + THR];
      }
    }
    o[m] = acc;
  }
#pragma unroll
  for (int m = 0; m < M; ++m) {
    if (m & LOWBIT) continue;
    XV v;
    if constexpr (MODE == 0) {
      v = XV{o[m], o[m | LOWBIT]};
    } else if constexpr (MODE == 1) {
      v = XV{o[m].x, o[m | LOWBIT].x, o[m].y, o[m | LOWBIT].y};
    } else {
      v = XV{o[m].x, o[m].y, o[m | LOWBIT].x, o[m | LOWBIT].y};
    }
    const uint64_t at = base | d.off[m];
    outv[at] = d.accumulate ? (XV)(outv[at] + v) : v;  // (non-temporal accesses measured here too: no gain, r06_real_p.md)
  }
}

template <typename R, int K, int NC, bool SW, int MODE>
static void launch_real_low_lb(int lb, dim3 grid, hipStream_t stream, const R* d_in, R* d_out, const Ins& ins, const RealGroupDesc& d,
                               const RealTab<R>& tab) {
#define RL(LBV) hipLaunchKernelGGL((k_real_groups_low<R, K, NC, SW, LBV, MODE>), grid, dim3(kBlock), 0, stream, d_in, d_out, ins, d, tab)
  if (lb == 0) RL(0);
  if constexpr (K >= 2) { if (lb == 1) RL(1); }
  if constexpr (K >= 3) { if (lb == 2) RL(2); }
#undef RL
}

template <typename R, int MODE>
static int launch_real_low(const FlatOp& f, int lb, const R* d_in, R* d_out, const Ins& ins, const RealGroupDesc& d, const RealTab<R>& tab,
                           hipStream_t stream) {
  const dim3 grid((unsigned)((d.nitems + kBlock - 1) / kBlock));
  const bool swap = f.inner->kind == QIP_OP_SWAP;
  const int nc = (int)f.n_control;
#define RLK(KK, NC, SW) launch_real_low_lb<R, KK, NC, SW, MODE>(lb, grid, stream, d_in, d_out, ins, d, tab)
  switch (f.k_all) {
    case 1: RLK(1, 0, false); break;
    case 2:
      if (swap) RLK(2, 0, true);
      else if (nc == 0) RLK(2, 0, false);
      else RLK(2, 1, false);
      break;
    default:
      if (swap) RLK(3, 1, true);
      else if (nc == 0) RLK(3, 0, false);
      else if (nc == 1) RLK(3, 1, false);
      else RLK(3, 2, false);
      break;
  }
#undef RLK
  HIPCHK(hipGetLastError());
  return QIP_OK;
}

// true (and launched) when the op qualifies; false: the literal kernel takes it
template <typename R>
static int launch_real_groups(uint32_t n, const FlatOp& f, const R* d_in, R* d_out, int accumulate, hipStream_t stream, bool* done) {
  *done = false;
  const uint32_t K = f.k_all;
  if (!f.distinct || K > 4 || K >= n || g_force_generic) return QIP_OK;
  if (f.inner->kind == QIP_OP_SPARSE) return QIP_OK;
  if (f.inner->kind == QIP_OP_SWAP && (f.n_op & 1u)) return QIP_OK;
  constexpr int VMAX = 16 / (int)sizeof(R);
  constexpr uint32_t LOGV = sizeof(R) == 8 ? 1u : 2u;
  const std::vector<uint32_t> pos = index_positions(n, f);
  const uint32_t lowest = *std::min_element(pos.begin(), pos.end());
  const bool aligned = aligned16(d_in, d_out);
  const bool vec = lowest >= LOGV && n >= K + LOGV && aligned;
  const RealTab<R> tab = arg_table<RealTab<R>>(f);
  if (!vec && aligned && K <= 3 && n >= K + 2) {  // one index bit inside the vector: k_real_groups_low
    bool p0 = false, p1 = false;
    for (uint32_t j = 0; j < K; ++j) {
      p0 = p0 || pos[j] == 0;
      p1 = p1 || pos[j] == 1;
    }
    const int mode = sizeof(R) == 8 ? (p0 ? 0 : -1) : (p0 && p1) ? 0 : p0 ? 1 : p1 ? 2 : -1;
    if (mode >= 0) {
      const uint32_t inpos = mode == 2 ? 1u : 0u, logvw = mode == 0 ? 1u : 2u;
      uint32_t jl = 0;
      for (uint32_t j = 0; j < K; ++j)
        if (pos[j] == inpos) jl = j;
      const GroupGeom g = make_groups(n, pos.data(), K, logvw, (int)jl, accumulate);
      *done = true;
      const int lb = (int)(K - 1 - jl);
      if (mode == 0) return launch_real_low<R, 0>(f, lb, d_in, d_out, g.ins, g.d, tab, stream);
      if constexpr (sizeof(R) == 4) {
        if (mode == 1) return launch_real_low<R, 1>(f, lb, d_in, d_out, g.ins, g.d, tab, stream);
        return launch_real_low<R, 2>(f, lb, d_in, d_out, g.ins, g.d, tab, stream);
      }
    }
  }
  // a 4-byte P with its lowest index bit at position 1: pairs of rows (8-byte accesses) instead of single ones
  const bool half = !vec && sizeof(R) == 4 && lowest == 1 && n >= K + 1 && aligned;
  const GroupGeom g = make_groups(n, pos.data(), K, vec ? LOGV : half ? 1u : 0u, -1, accumulate);
  *done = true;
  const bool nt = streams((uint64_t)sizeof(R) << n, vec, g.lowest);  // (V = 1 is the rare shape)
#define RK(KK)                                                                                                   \
  if constexpr (sizeof(R) == 4)                                                                                  \
    if (half) return launch_real_groups_k<R, 2, KK, false>(f, d_in, d_out, g.ins, g.d, tab, stream);             \
  return !vec ? launch_real_groups_k<R, 1, KK, false>(f, d_in, d_out, g.ins, g.d, tab, stream)                   \
         : nt ? launch_real_groups_k<R, VMAX, KK, true>(f, d_in, d_out, g.ins, g.d, tab, stream)                 \
              : launch_real_groups_k<R, VMAX, KK, false>(f, d_in, d_out, g.ins, g.d, tab, stream)
  switch (K) {
    case 1: RK(1);
    case 2: RK(2);
    case 3: RK(3);
    default: RK(4);
  }
#undef RK
}

template <typename R>
static int apply_op_real_device(int dtype, int device, uint32_t n, const qip_op* op, const R* d_in, uint64_t in_len, R* d_out, uint64_t out_len,
                                uint64_t in_off, uint64_t out_off, int accumulate, hipStream_t stream) {
  FlatOp f;
  QCHK(flatten_op(n, op, false, &f));
  if (out_len == 0) return QIP_OK;
  const GatherDesc d = make_gather_desc(n, f, in_len, out_len, in_off, out_off, accumulate);
  if (whole_vector(n, in_len, out_len, in_off, out_off)) {  // each input read once
    bool done = false;
    QCHK(launch_real_groups<R>(n, f, d_in, d_out, accumulate, stream, &done));
    if (done) return QIP_OK;
  }
  // the literal kernel, V rows per lane when no index bit sits inside a 16-byte vector and both windows are made of whole vectors
  constexpr int VMAX = 16 / (int)sizeof(R);
  bool wide = aligned16(d_in, d_out) && in_off % VMAX == 0 && out_off % VMAX == 0 && in_len % VMAX == 0 && out_len % VMAX == 0;
  for (uint32_t j = 0; j < f.k_all; ++j) wide = wide && d.pos[j] >= (sizeof(R) == 8 ? 1u : 2u);
  const dim3 grid(grid_stride(wide ? out_len / VMAX : out_len)), block(kBlock);
  if (f.inner->kind == QIP_OP_SWAP || (f.inner->kind == QIP_OP_MATRIX && f.n_op <= 4)) {
    const RealTab<R> tab = arg_table<RealTab<R>>(f);
    if (wide)
      hipLaunchKernelGGL((k_gather_real<R, true, VMAX>), grid, block, 0, stream, d_in, d_out, d, tab, (const R*)nullptr,
                         (const uint64_t*)nullptr, (const uint64_t*)nullptr, (const R*)nullptr);
    else
      hipLaunchKernelGGL((k_gather_real<R, true, 1>), grid, block, 0, stream, d_in, d_out, d, tab, (const R*)nullptr,
                         (const uint64_t*)nullptr, (const uint64_t*)nullptr, (const R*)nullptr);
    HIPCHK(hipGetLastError());
    return QIP_OK;
  }
  // a payload too large for the kernel arguments: resident in the payload cache (the call only launches), or — the cache
  // disabled or full — one device buffer for this call, which then synchronises
  const SlicePayload pay = literal_payload(device, dtype, f, sizeof(R));
  const size_t o_cols = pay.nspans == 3 ? pay.span[1].off : 0, o_vals = pay.nspans == 3 ? pay.span[2].off : 0;
  char* buf = nullptr;
  if (!g_force_generic) QCHK(slice_payload_get(device, pay, stream, &buf));
  const bool resident = buf != nullptr;
  if (!resident) HIPCHK(hipMalloc((void**)&buf, std::max<size_t>(pay.total, 16)));
  auto body = [&]() -> int {
    if (!resident)
      for (int i = 0; i < pay.nspans; ++i)
        if (pay.span[i].bytes) HIPCHK(hipMemcpyAsync(buf + pay.span[i].off, pay.span[i].p, pay.span[i].bytes, hipMemcpyHostToDevice, stream));
    const RealTab<R> tab = {};  // (TAB = false: never read)
    if (wide)
      hipLaunchKernelGGL((k_gather_real<R, false, VMAX>), grid, block, 0, stream, d_in, d_out, d, tab, (const R*)buf, (const uint64_t*)buf,
                         (const uint64_t*)(buf + o_cols), (const R*)(buf + o_vals));
    else
      hipLaunchKernelGGL((k_gather_real<R, false, 1>), grid, block, 0, stream, d_in, d_out, d, tab, (const R*)buf, (const uint64_t*)buf,
                         (const uint64_t*)(buf + o_cols), (const R*)(buf + o_vals));
    HIPCHK(hipGetLastError());
    if (!resident) HIPCHK(hipStreamSynchronize(stream));
    return QIP_OK;
  };
  const int rc = body();
  if (resident) return rc;
  if (rc != QIP_OK) (void)hipStreamSynchronize(stream);
  (void)hipFree(buf);
  return rc;
}

// ---- complex P: the same two kernels on Complex<f64> / Complex<f32> slices ------------------------------------------------------
// A dense op on k <= 3 qubits (64 entries: 1 KiB of Complex<f64>; a 4-qubit table is 4 KiB and does not fit the kernel-argument
// segment) or a Swap, k_all <= 4 indices with the controls: the table travels in the kernel arguments, the call only launches.
template <typename T> struct CplxTab {
  amp_t<T> v[64];
};

// ... or, for any larger payload, behind pointers into the payload cache: a dense table of any size, CSR rows in stored order
template <typename T> struct CplxPtrs {
  const amp_t<T>* dense;
  const uint64_t *rowptr, *cols;
  const amp_t<T>* vals;
};

// the literal fold of k_gather_generic, one output row per lane, any window; only the table's home differs (TabT = CplxTab<T>:
// the kernel arguments, CplxPtrs<T>: device memory)
template <typename T, typename TabT>
__global__ __launch_bounds__(kBlock) void k_gather_cplx(const amp_t<T>* __restrict__ in, amp_t<T>* __restrict__ out, GatherDesc d,
                                                        TabT tab) {
  using A = amp_t<T>;
  constexpr bool PTR = std::is_same<TabT, CplxPtrs<T>>::value;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r < d.out_len; r += stride) {
    const uint64_t row = d.out_off + r;
    const uint64_t matrow = g_full_to_sub(d, row);
    A acc = czero<A>();
    A one;
    one.x = 1;
    one.y = 0;
    const uint64_t thr = (1ull << (d.n_control + d.n_op)) - (1ull << d.n_op);  // (0 without controls)
    if (matrow < thr) {  // outside the control subspace
      acc = cadd(acc, g_term<T>(d, row, matrow, one, in));
    } else if (d.inner_kind == 0) {  // MATRIX
      const uint64_t side = 1ull << d.n_op;
      for (uint64_t c = 0; c < side; ++c) {
        A v;
        if constexpr (PTR) v = tab.dense[(matrow - thr) * side + c];
        else v = tab.v[(matrow - thr) * side + c];
        if (!(v.x == (T)0 && v.y == (T)0)) acc = cadd(acc, g_term<T>(d, row, c + thr, v, in));
      }
    } else if (PTR && d.inner_kind == 1) {  // SPARSE: every stored entry, in stored order
      if constexpr (PTR)
        for (uint64_t p = tab.rowptr[matrow - thr]; p < tab.rowptr[matrow - thr + 1]; ++p)
          acc = cadd(acc, g_term<T>(d, row, tab.cols[p] + thr, tab.vals[p], in));
    } else {  // SWAP
      const uint32_t half_n = d.n_op >> 1;
      const uint64_t irow = matrow - thr, lower_mask = ~(~0ull << half_n);
      const uint64_t col = ((irow & lower_mask) << half_n) + (irow >> half_n);
      acc = cadd(acc, g_term<T>(d, row, col + thr, one, in));
    }
    out[r] = d.accumulate ? cadd(out[r], acc) : acc;
  }
}

// k_real_groups for a complex element E: one amplitude (amp_t<T>), or f32x4 = two adjacent Complex<f32> (no index bit at
// position 0, d.off / ins in units of pairs).  The lane reads its 2^K elements once and folds every row as the literal kernel
// does: acc = 0; acc = cadd(acc, cmul(m[row][c], x[c])) for c ascending, an entry skipped only when both parts are zero (a scalar
// branch); a row outside the control subspace or of a Swap is 0 + (1 + 0i) * x[col].  Bit-equal to k_gather_generic.
template <typename T, typename E, int K, int NC, bool SWAP, bool NT>
__global__ __launch_bounds__(kBlock) void k_cplx_groups(const E* __restrict__ in, E* __restrict__ out, Ins ins, RealGroupDesc d,
                                                        CplxTab<T> tab) {
  using A = amp_t<T>;
  constexpr int M = 1 << K, KOP = K - NC, SIDE = 1 << KOP, THR = M - SIDE;
  const uint64_t w = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (w >= d.nitems) return;
  const uint64_t base = insert_bits<K>(w, ins);
  A one;
  one.x = 1;
  one.y = 0;
  E x[M];
#pragma unroll
  for (int m = 0; m < M; ++m) x[m] = ldg<NT>(in + (base | d.off[m]));
#pragma unroll
  for (int m = 0; m < M; ++m) {
    E acc = czero<E>();
    if (m < THR) {
      acc = cadd(acc, cmul(one, x[m]));
    } else if constexpr (SWAP) {
      constexpr int HALF = KOP >> 1;
      const int irow = m - THR;
      const int col = ((irow & ((1 << HALF) - 1)) << HALF) + (irow >> HALF);
      acc = cadd(acc, cmul(one, x[col + THR]));
    } else {
#pragma unroll
      for (int c = 0; c < SIDE; ++c) {
        const A v = tab.v[(m - THR) * SIDE + c];
        if (!(v.x == (T)0 && v.y == (T)0)) acc = cadd(acc, cmul(v, x[c + THR]));
      }
    }
    const uint64_t at = base | d.off[m];
    stg<NT>(out + at, d.accumulate ? cadd(ldg<NT>(out + at), acc) : acc);
  }
}

template <typename T, typename E, int K, bool NT>
static int launch_cplx_groups_k(const FlatOp& f, const E* d_in, E* d_out, const Ins& ins, const RealGroupDesc& d, const CplxTab<T>& tab,
                                hipStream_t stream) {
  const dim3 grid((unsigned)((d.nitems + kBlock - 1) / kBlock)), block(kBlock);
  const bool swap = f.inner->kind == QIP_OP_SWAP;
#define CG(NC, SW)                                                                                                       \
  hipLaunchKernelGGL((k_cplx_groups<T, E, K, NC, SW, NT>), grid, block, 0, stream, d_in, d_out, ins, d, tab)
  const int nc = (int)f.n_control;  // (the caller admits a dense op on <= 3 qubits: K - nc <= 3)
  if (swap) {
    if constexpr (K == 2) { CG(0, true); }
    else if constexpr (K == 3) { CG(1, true); }
    else if constexpr (K == 4) { if (nc == 0) CG(0, true); else CG(2, true); }
  } else {
    if constexpr (K == 1) { CG(0, false); }
    else if constexpr (K == 2) { if (nc == 0) CG(0, false); else CG(1, false); }
    else if constexpr (K == 3) { if (nc == 0) CG(0, false); else if (nc == 1) CG(1, false); else CG(2, false); }
    else { if (nc == 1) CG(1, false); else if (nc == 2) CG(2, false); else CG(3, false); }
  }
#undef CG
  HIPCHK(hipGetLastError());
  return QIP_OK;
}

// the whole vector, distinct indices, K = k_all <= 4 < n (the caller checked the op's kind and size)
template <typename T>
static int launch_cplx_groups(uint32_t n, const FlatOp& f, const amp_t<T>* d_in, amp_t<T>* d_out, const CplxTab<T>& tab, int accumulate,
                              hipStream_t stream) {
  using A = amp_t<T>;
  const uint32_t K = f.k_all;
  const std::vector<uint32_t> pos = index_positions(n, f);
  const uint32_t lowest = *std::min_element(pos.begin(), pos.end());
  // Complex<f32>: pairs of amplitudes (f32x4) when no index sits at position 0 and both slices start on a 16-byte boundary
  const bool pairs = sizeof(A) == 8 && lowest >= 1 && n >= K + 1 && aligned16(d_in, d_out);
  const GroupGeom g = make_groups(n, pos.data(), K, pairs ? 1u : 0u, -1, accumulate);
  const bool nt = streams((uint64_t)sizeof(A) << n, sizeof(A) == 16 || pairs, g.lowest);
#define CK(KK)                                                                                                               \
  if constexpr (sizeof(A) == 8) {                                                                                           \
    if (pairs)                                                                                                               \
      return nt ? launch_cplx_groups_k<T, f32x4, KK, true>(f, (const f32x4*)d_in, (f32x4*)d_out, g.ins, g.d, tab, stream)    \
                : launch_cplx_groups_k<T, f32x4, KK, false>(f, (const f32x4*)d_in, (f32x4*)d_out, g.ins, g.d, tab, stream);  \
    return launch_cplx_groups_k<T, A, KK, false>(f, d_in, d_out, g.ins, g.d, tab, stream);                                   \
  } else {                                                                                                                   \
    return nt ? launch_cplx_groups_k<T, A, KK, true>(f, d_in, d_out, g.ins, g.d, tab, stream)                                \
              : launch_cplx_groups_k<T, A, KK, false>(f, d_in, d_out, g.ins, g.d, tab, stream);                              \
  }
  switch (K) {
    case 1: CK(1)
    case 2: CK(2)
    case 3: CK(3)
    default: CK(4)
  }
#undef CK
}

// ---- the whole vector, a dense op on 4 qubits with any controls: read once, the table behind a wave-uniform pointer ---------------
// k_cplx_groups with the 16 x 16 table in the payload cache instead of the kernel arguments (every lane reads the same entry:
// scalar loads, the zero skip stays a scalar branch).  The group is the op's 16 elements alone; controls are tested bits of the
// group's base — outside their subspace every row is the iterator's single (row, 1) entry.  d.off / ins / cmask in units of E.
int64_t g_slice_read_once = 1;  // tuning option "slice_read_once": 0 = the literal pointer launch for every cached payload (A/B runs)

template <typename T, typename E, bool NT>
__global__ __launch_bounds__(kBlock) void k_cplx_dense4(const E* __restrict__ in, E* __restrict__ out, Ins ins, RealGroupDesc d,
                                                        uint64_t cmask, const amp_t<T>* __restrict__ tab) {
  using A = amp_t<T>;
  constexpr int M = 16;
  const uint64_t w = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (w >= d.nitems) return;
  const uint64_t base = insert_bits<4>(w, ins);
  A one;
  one.x = 1;
  one.y = 0;
  E x[M], y[M];
#pragma unroll
  for (int m = 0; m < M; ++m) x[m] = ldg<NT>(in + (base | d.off[m]));
  if ((base & cmask) == cmask) {
#pragma unroll
    for (int m = 0; m < M; ++m) {
      E acc = czero<E>();
#pragma unroll
      for (int c = 0; c < M; ++c) {
        const A v = tab[m * M + c];
        if (!(v.x == (T)0 && v.y == (T)0)) acc = cadd(acc, cmul(v, x[c]));
      }
      y[m] = acc;
    }
  } else {
#pragma unroll
    for (int m = 0; m < M; ++m) y[m] = cadd(czero<E>(), cmul(one, x[m]));
  }
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const uint64_t at = base | d.off[m];
    stg<NT>(out + at, d.accumulate ? cadd(ldg<NT>(out + at), y[m]) : y[m]);
  }
}

// (the caller checked: MATRIX on 4 distinct qubits, distinct controls, both windows the whole vector, k_all < n)
template <typename T>
static int launch_cplx_dense4(uint32_t n, const FlatOp& f, const amp_t<T>* d_in, amp_t<T>* d_out, const amp_t<T>* tab, int accumulate,
                              hipStream_t stream) {
  using A = amp_t<T>;
  const uint32_t nc = f.n_control;
  const std::vector<uint32_t> pos = index_positions(n, f);
  const uint32_t lowest = *std::min_element(pos.begin(), pos.end());
  const bool pairs = sizeof(A) == 8 && lowest >= 1 && n >= 5 && aligned16(d_in, d_out);
  const uint32_t lv = pairs ? 1u : 0u;
  uint64_t cmask = 0;
  for (uint32_t j = 0; j < nc; ++j) cmask |= 1ull << (pos[j] - lv);
  const GroupGeom g = make_groups(n, pos.data() + nc, 4, lv, -1, accumulate);  // the group is the op's positions alone
  const bool nt = streams((uint64_t)sizeof(A) << n, sizeof(A) == 16 || pairs, g.lowest);  // (... and so is what the rule looks at)
  const dim3 grid((unsigned)((g.d.nitems + kBlock - 1) / kBlock)), block(kBlock);
#define D4(EE, NTV) hipLaunchKernelGGL((k_cplx_dense4<T, EE, NTV>), grid, block, 0, stream, (const EE*)d_in, (EE*)d_out, g.ins, g.d, cmask, tab)
  if constexpr (sizeof(A) == 8) {
    if (pairs) {
      if (nt) D4(f32x4, true);
      else D4(f32x4, false);
    } else {
      D4(A, false);
    }
  } else {
    if (nt) D4(A, true);
    else D4(A, false);
  }
#undef D4
  HIPCHK(hipGetLastError());
  return QIP_OK;
}

// ---- ... on 5 or 6 qubits: groups staged through LDS ---------------------------------------------------------------------------
// 2^KOP elements no longer fit a lane (Complex<f64>, KOP = 6: 256 VGPRs for the inputs alone).  A block of 256 lanes owns a TILE:
// the op's KOP positions and the six lowest positions outside the op (TB = KOP + 6 tile bits; tile bits 0..5 are index positions
// 0..5 whatever the op, so every global access of a wave is one whole row of 64 consecutive elements) = 64 groups of 2^KOP.
//   load     element t of the tile -> LDS slot c * 64 + (g ^ c): c = its sub-index in matrix order, g = its group.
//   fold     lane g of wave w folds the R = 2^KOP / 4 rows [w R, (w + 1) R) of group g: for c ascending ONE LDS read of x[c] —
//            a wave reads 64 consecutive slots, conflict-free — serves R rows; the table entries m[row][c] are the same for the
//            whole wave (the table lies TRANSPOSED in the payload cache, R consecutive entries per c: scalar loads, and the zero
//            skip is a scalar branch).  acc = 0; acc = cadd(acc, cmul(v, x[c])), unfused: the literal fold bit for bit.
//            A group outside the control subspace (controls are tested bits of the group's index) takes 0 + (1 + 0i) x[row].
//   store    the rows go back through the same slots, then out in whole wave rows (read first when accumulating).
// Each input element is read from HBM once, each output element written once.  LDS: 16 B x 2^12 = 64 KiB for Complex<f64> on 6.
struct DenseTileDesc {
  uint32_t cw[12], gw[12];  // tile bit b set: cw[b] is added to c (b is an op position) or gw[b] to g (a free one); the other is 0
  uint32_t tpos[12];        // tile bit b = index position tpos[b] (ascending; tpos[b] = b for b < 6)
  uint64_t cmask;           // control positions (all must be 1)
  int32_t accumulate;
};

template <typename T, int KOP, bool NT>
__global__ __launch_bounds__(kBlock) void k_cplx_dense_tile(const amp_t<T>* __restrict__ in, amp_t<T>* __restrict__ out, Ins ins,
                                                            DenseTileDesc d, const amp_t<T>* __restrict__ tabT) {
  using A = amp_t<T>;
  constexpr int TB = KOP + 6, S = 1 << KOP, R = S / 4, NIT = (1 << TB) / kBlock;
  __shared__ A lds[1 << TB];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
  const uint64_t base = insert_bits<TB>((uint64_t)blockIdx.x, ins);
  uint32_t c_lo = 0, g_lo = 0;  // what the lane's six bits give at load / store time
#pragma unroll
  for (int b = 0; b < 6; ++b)
    if ((lane >> b) & 1u) {
      c_lo += d.cw[b];
      g_lo += d.gw[b];
    }
  uint64_t hi_off[NIT];
  uint32_t slot[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const uint32_t th = (uint32_t)it * 4u + wv;  // tile bits 6.. of this wave row
    uint32_t c = c_lo, g = g_lo;
    uint64_t o = 0;
#pragma unroll
    for (int b = 6; b < TB; ++b)
      if ((th >> (b - 6)) & 1u) {
        c += d.cw[b];
        g += d.gw[b];
        o |= 1ull << d.tpos[b];
      }
    hi_off[it] = base | o | lane;
    slot[it] = c * 64u + (g ^ (c & 63u));
  }
#pragma unroll
  for (int it = 0; it < NIT; ++it) lds[slot[it]] = ldg<NT>(in + hi_off[it]);
  __syncthreads();
  // fold: lane = group
  uint64_t gidx = base;
#pragma unroll
  for (int b = 0; b < TB; ++b)
    if (d.gw[b] & lane) gidx |= 1ull << d.tpos[b];
  A acc[R];
  if ((gidx & d.cmask) == d.cmask) {
#pragma unroll
    for (int j = 0; j < R; ++j) acc[j] = czero<A>();
#pragma unroll 2
    for (uint32_t c = 0; c < (uint32_t)S; ++c) {
      const A xc = lds[c * 64u + (lane ^ (c & 63u))];
      const A* __restrict__ col = tabT + ((size_t)c * S + wv * R);
#pragma unroll
      for (int j = 0; j < R; ++j) {
        const A v = col[j];
        if (!(v.x == (T)0 && v.y == (T)0)) acc[j] = cadd(acc[j], cmul(v, xc));
      }
    }
  } else {
    A one;
    one.x = 1;
    one.y = 0;
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const uint32_t m = wv * R + j;
      acc[j] = cadd(czero<A>(), cmul(one, lds[m * 64u + (lane ^ (m & 63u))]));
    }
  }
  __syncthreads();  // every wave has read its inputs: the slots take the rows
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const uint32_t m = wv * R + j;
    lds[m * 64u + (lane ^ (m & 63u))] = acc[j];
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const A y = lds[slot[it]];
    stg<NT>(out + hi_off[it], d.accumulate ? cadd(ldg<NT>(out + hi_off[it]), y) : y);
  }
}

constexpr uint32_t kDenseTileMinQubits[2] = {11, 12};  // KOP = 5, 6: the tile's KOP + 6 positions

// (the caller checked: MATRIX on 5 / 6 distinct qubits, distinct controls, both windows the whole vector, n >= n_op + 6)
template <typename T>
static int launch_cplx_dense_tile(uint32_t n, const FlatOp& f, const amp_t<T>* d_in, amp_t<T>* d_out, const amp_t<T>* tabT, int accumulate,
                                  hipStream_t stream) {
  const uint32_t nc = f.n_control, kop = f.n_op, tb = kop + 6;
  DenseTileDesc d;
  memset(&d, 0, sizeof d);
  d.accumulate = accumulate;
  uint64_t opmask = 0;
  for (uint32_t j = 0; j < f.k_all; ++j) {
    const uint32_t p = (uint32_t)(n - 1 - f.outer->indices[j]);
    if (j < nc) d.cmask |= 1ull << p;
    else opmask |= 1ull << p;
  }
  std::vector<uint32_t> tile;  // ascending: every op position and the six lowest others
  for (uint32_t p = 0, nfree = 0; p < n && tile.size() < tb; ++p) {
    const bool is_op = (opmask >> p) & 1ull;
    if (!is_op && nfree == 6) continue;
    if (!is_op) {
      d.gw[tile.size()] = 1u << nfree;
      nfree += 1;
    } else {
      for (uint32_t j = 0; j < kop; ++j)
        if ((uint32_t)(n - 1 - f.outer->indices[nc + j]) == p) d.cw[tile.size()] = 1u << (kop - 1 - j);
    }
    d.tpos[tile.size()] = p;
    tile.push_back(p);
  }
  if (tile.size() != tb) return fail(QIP_ERR_UNSUPPORTED, "dense tile: %zu of %u positions", tile.size(), tb);
  const Ins ins = make_ins(tile, 0);
  const bool nt = (sizeof(amp_t<T>) << n) >= (64ull << 20);  // size alone, not streams(): every access is a whole wave row whatever the op
  const dim3 grid((unsigned)(1ull << (n - tb))), block(kBlock);
#define DT(KK, NTV) hipLaunchKernelGGL((k_cplx_dense_tile<T, KK, NTV>), grid, block, 0, stream, d_in, d_out, ins, d, tabT)
  if (kop == 5) {
    if (nt) DT(5, true);
    else DT(5, false);
  } else {
    if (nt) DT(6, true);
    else DT(6, false);
  }
#undef DT
  HIPCHK(hipGetLastError());
  return QIP_OK;
}

// complex P on device slices: which kernel runs a call (option force_generic aside: today's literal kernel of the state path,
// k_gather_generic, through a handle that adopts the caller's stream and owns the payload arena; that route synchronises).
//   the table fits the kernel arguments — a dense op on <= 3 qubits or a Swap, any number of controls:
//       whole vector, distinct indices, k_all <= 4 < n      k_cplx_groups (each input read once)
//       everything else                                      k_gather_cplx, the literal fold
//   it does not — a dense op on >= 4 qubits, every SparseMatrix: the payload cache holds the table; once resident,
//       whole vector, distinct indices, dense on 4, k_all < n           k_cplx_dense4 (read once)
//       whole vector, distinct indices, dense on 5 / 6, n >= n_op + 6   k_cplx_dense_tile (read once, through LDS)
//       everything else (windows, repeated indices, wider, sparse)      k_gather_cplx behind pointers, the literal fold
//   a payload the cache cannot take (option slice_payload_cache_mb: 0, or full): the force_generic route.
// Every route but the last is ONE launch on the caller's stream and nothing else: no handle, no allocation, no copy, no
// synchronisation.  The first call with a payload uploads it (hipMalloc + a blocking copy; refused on a capturing stream).
// The read-once kernels hold their place by measurement (profiles/complex_slices.md).
template <typename T>
static int apply_op_complex_device(int dtype, int device, hipStream_t stream, uint32_t n, const qip_op* op, const void* d_in,
                                   uint64_t in_len, void* d_out, uint64_t out_len, uint64_t in_off, uint64_t out_off,
                                   int accumulate) {
  using A = amp_t<T>;
  FlatOp f;
  QCHK(flatten_op(n, op, false, &f));
  if (out_len == 0) return QIP_OK;
  const bool swap = f.inner->kind == QIP_OP_SWAP && !(f.n_op & 1u);
  const bool small = swap || (f.inner->kind == QIP_OP_MATRIX && f.n_op <= 3);
  const bool cached = !small && (f.inner->kind == QIP_OP_MATRIX || f.inner->kind == QIP_OP_SPARSE);
  const bool whole = whole_vector(n, in_len, out_len, in_off, out_off) && f.distinct && f.k_all < n;
  const GatherDesc d = make_gather_desc(n, f, in_len, out_len, in_off, out_off, accumulate);
  if (!g_force_generic && small) {
    const CplxTab<T> tab = arg_table<CplxTab<T>>(f);
    if (whole && f.k_all <= 4) return launch_cplx_groups<T>(n, f, (const A*)d_in, (A*)d_out, tab, accumulate, stream);
    hipLaunchKernelGGL((k_gather_cplx<T, CplxTab<T>>), dim3(grid_stride(out_len)), dim3(kBlock), 0, stream, (const A*)d_in, (A*)d_out, d, tab);
    HIPCHK(hipGetLastError());
    return QIP_OK;
  }
  if (!g_force_generic && cached) {
    const bool tile = g_slice_read_once && whole && f.inner->kind == QIP_OP_MATRIX && (f.n_op == 5 || f.n_op == 6) &&
                      n >= kDenseTileMinQubits[f.n_op - 5];
    const bool dense4 = g_slice_read_once && whole && f.inner->kind == QIP_OP_MATRIX && f.n_op == 4;
    // the device form: the literal kernels' (and k_cplx_dense4's) table as it is, k_cplx_dense_tile's transposed ([c][row])
    SlicePayload p = literal_payload(device, dtype, f, sizeof(A));
    if (tile) p.head[2] = kTransposedTableKind;
    const std::function<void(unsigned char*)> transposed = [&f](unsigned char* dst) {
      const uint64_t side = 1ull << f.n_op;
      const A* m = (const A*)f.inner->dense;
      A* t = (A*)dst;
      for (uint64_t r = 0; r < side; ++r)
        for (uint64_t c = 0; c < side; ++c) t[c * side + r] = m[r * side + c];
    };
    char* dev = nullptr;
    QCHK(slice_payload_get(device, p, stream, &dev, tile ? &transposed : nullptr));
    if (dev && tile) return launch_cplx_dense_tile<T>(n, f, (const A*)d_in, (A*)d_out, (const A*)dev, accumulate, stream);
    if (dev && dense4) return launch_cplx_dense4<T>(n, f, (const A*)d_in, (A*)d_out, (const A*)dev, accumulate, stream);
    if (dev) {
      CplxPtrs<T> ptrs;
      memset(&ptrs, 0, sizeof ptrs);
      if (f.inner->kind == QIP_OP_MATRIX) {
        ptrs.dense = (const A*)dev;
      } else {
        ptrs.rowptr = (const uint64_t*)dev;
        ptrs.cols = (const uint64_t*)(dev + p.span[1].off);
        ptrs.vals = (const A*)(dev + p.span[2].off);
      }
      hipLaunchKernelGGL((k_gather_cplx<T, CplxPtrs<T>>), dim3(grid_stride(out_len)), dim3(kBlock), 0, stream, (const A*)d_in, (A*)d_out, d,
                         ptrs);
      HIPCHK(hipGetLastError());
      return QIP_OK;
    }
  }
  qip_hip_state* s = nullptr;
  QCHK(qip_hip_state_wrap(n, dtype, device, d_out, nullptr, (void*)stream, &s));
  int rc = launch_gather<T>(s, f, (const amp_t<T>*)d_in, in_len, (amp_t<T>*)d_out, out_len, in_off, out_off, accumulate);
  std::string keep = g_last_error;
  qip_hip_state_destroy(s);  // (synchronises the stream: the payload arena dies with the handle)
  if (rc != QIP_OK) g_last_error = keep;
  return rc;
}

extern "C" int qip_hip_apply_op_device(int dtype, int device, void* stream, uint32_t n, const qip_op* op, const void* d_in,
                                       uint64_t in_len, void* d_out, uint64_t out_len, uint64_t in_off, uint64_t out_off,
                                       int accumulate) try {
  if (!elem_bytes(dtype)) return fail(QIP_ERR_INVALID, "bad dtype %d", dtype);
  if ((in_len && !d_in) || (out_len && !d_out)) return fail(QIP_ERR_INVALID, "null buffer");
  if (n == 0 || n > 40) return fail(QIP_ERR_INVALID, "n = %u out of range [1, 40]", n);
  if (qip_hip_device_count() <= device || device < 0)
    return fail(QIP_ERR_NO_DEVICE, "no HIP device %d visible: qip_hip has no CPU fallback", device);
  HIPCHK(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  switch (dtype) {
    case QIP_C64: return apply_op_complex_device<double>(dtype, device, st, n, op, d_in, in_len, d_out, out_len, in_off, out_off, accumulate);
    case QIP_C32: return apply_op_complex_device<float>(dtype, device, st, n, op, d_in, in_len, d_out, out_len, in_off, out_off, accumulate);
    case QIP_F64: return apply_op_real_device<double>(dtype, device, n, op, (const double*)d_in, in_len, (double*)d_out, out_len, in_off, out_off, accumulate, st);
    case QIP_F32: return apply_op_real_device<float>(dtype, device, n, op, (const float*)d_in, in_len, (float*)d_out, out_len, in_off, out_off, accumulate, st);
    case QIP_I64: return apply_op_real_device<uint64_t>(dtype, device, n, op, (const uint64_t*)d_in, in_len, (uint64_t*)d_out, out_len, in_off, out_off, accumulate, st);
    default: return apply_op_real_device<uint32_t>(dtype, device, n, op, (const uint32_t*)d_in, in_len, (uint32_t*)d_out, out_len, in_off, out_off, accumulate, st);
  }
} QIP_CATCH_ALL
