// qip_circuit.hip — apply_ops: gate fusion, tile sweeps (interpreter launches and run-time-compiled segments), hipGraph programs.
#include "qip_tile.h"

// ---------------------------------------------------------------------------------------
// gate fusion: option "fuse" = K merges consecutive small gates into dense
// gates on <= K qubits, applied in ONE sweep each.  The reference has no analogue (its apply_ops
// multi-op path is unused and inconsistent); this is pure host bookkeeping on
// 2^K x 2^K matrices.  Results equal the gate-by-gate path up to the rounding of the matrix
// products (|delta| ~ 1e-15 per fused gate), so fused runs are held to the 1e-12 bar, never to
// bit equality.  Open clusters always act on pairwise disjoint qubit sets, so they commute and
// may be flushed in any order; an op is merged only into clusters it overlaps, or into a
// disjoint one (which also commutes with every other open cluster).
// ---------------------------------------------------------------------------------------
typedef std::complex<double> cd;
struct Cluster {
  std::vector<uint32_t> pos;  // bit positions, descending: pos[0] is the MSB of the sub-index
  std::vector<cd> m;          // 2^q x 2^q, row-major
};

// dense matrix of a flattened op over its own index list (controls first), MSB-first order
template <typename T>
static bool op_to_dense(uint32_t n, const FlatOp& f, uint32_t max_k, std::vector<uint32_t>* pos,
                        std::vector<cd>* mat) {
  if (!f.distinct || f.k_all > max_k) return false;
  const uint32_t kt = f.k_all, k = f.n_op;
  const size_t S = (size_t)1 << kt, Si = (size_t)1 << k, thr = S - Si;
  pos->clear();
  for (uint32_t j = 0; j < kt; ++j) pos->push_back(n - 1 - (uint32_t)f.outer->indices[j]);
  mat->assign(S * S, cd(0, 0));
  for (size_t r = 0; r < thr; ++r) (*mat)[r * S + r] = cd(1, 0);
  const T* dense = static_cast<const T*>(f.inner->dense);
  const T* vals = static_cast<const T*>(f.inner->sparse_vals);
  for (size_t r = 0; r < Si; ++r) {
    switch (f.inner->kind) {
      case QIP_OP_MATRIX:
        for (size_t c = 0; c < Si; ++c)
          (*mat)[(thr + r) * S + thr + c] = cd(dense[2 * (r * Si + c)], dense[2 * (r * Si + c) + 1]);
        break;
      case QIP_OP_SPARSE:
        for (uint64_t e = f.inner->sparse_rowptr[r]; e < f.inner->sparse_rowptr[r + 1]; ++e)
          (*mat)[(thr + r) * S + thr + f.inner->sparse_cols[e]] += cd(vals[2 * e], vals[2 * e + 1]);
        break;
      default: {  // SWAP
        const uint32_t h = k >> 1;
        const size_t c = ((r & (((size_t)1 << h) - 1)) << h) + (r >> h);
        (*mat)[(thr + r) * S + thr + c] = cd(1, 0);
      }
    }
  }
  return true;
}

// matrix of `m` (over positions `pos`, MSB first) embedded into the space of `upos` (descending)
static std::vector<cd> embed(const std::vector<cd>& m, const std::vector<uint32_t>& pos,
                             const std::vector<uint32_t>& upos) {
  const uint32_t u = (uint32_t)upos.size(), k = (uint32_t)pos.size();
  const size_t U = (size_t)1 << u, S = (size_t)1 << k;
  std::vector<uint32_t> bit_in_u(k);
  size_t opmask = 0;
  for (uint32_t i = 0; i < k; ++i)
    for (uint32_t j = 0; j < u; ++j)
      if (upos[j] == pos[i]) {
        bit_in_u[i] = u - 1 - j;
        opmask |= (size_t)1 << (u - 1 - j);
      }
  auto sub = [&](size_t r) {
    size_t s_ = 0;
    for (uint32_t i = 0; i < k; ++i) s_ |= ((r >> bit_in_u[i]) & 1) << (k - 1 - i);
    return s_;
  };
  std::vector<cd> e(U * U, cd(0, 0));
  for (size_t r = 0; r < U; ++r)
    for (size_t c = 0; c < U; ++c)
      if ((r & ~opmask) == (c & ~opmask)) e[r * U + c] = m[sub(r) * S + sub(c)];
  return e;
}

static void cluster_apply(Cluster* cl, const std::vector<uint32_t>& pos, const std::vector<cd>& m) {
  std::vector<uint32_t> upos = cl->pos;
  for (uint32_t p : pos)
    if (std::find(upos.begin(), upos.end(), p) == upos.end()) upos.push_back(p);
  std::sort(upos.begin(), upos.end(), std::greater<uint32_t>());
  const size_t U = (size_t)1 << upos.size();
  const std::vector<cd> a = embed(m, pos, upos);              // the new gate, applied after
  const std::vector<cd> b = embed(cl->m, cl->pos, upos);      // what the cluster already holds
  std::vector<cd> out(U * U, cd(0, 0));
  for (size_t r = 0; r < U; ++r)
    for (size_t k = 0; k < U; ++k) {
      const cd v = a[r * U + k];
      if (v == cd(0, 0)) continue;
      for (size_t c = 0; c < U; ++c) out[r * U + c] += v * b[k * U + c];
    }
  cl->pos = upos;
  cl->m = out;
}

template <typename T>
static int flush_cluster(qip_hip_state* s, const BatchRun& run, const Cluster& cl) {
  const size_t S = (size_t)1 << cl.pos.size();
  std::vector<uint64_t> idx;
  for (uint32_t p : cl.pos) idx.push_back(s->n - 1 - p);
  std::vector<T> data(2 * S * S);
  for (size_t e = 0; e < S * S; ++e) {
    data[2 * e] = (T)cl.m[e].real();
    data[2 * e + 1] = (T)cl.m[e].imag();
  }
  qip_op op;
  memset(&op, 0, sizeof op);
  op.kind = QIP_OP_MATRIX;
  op.n_indices = (uint32_t)idx.size();
  op.indices = idx.data();
  op.dense = data.data();
  return apply_op_t<T>(s, &op, run);
}

template <typename T>
int apply_ops_fused(qip_hip_state* s, const BatchRun& run, const qip_op* ops, uint64_t count, uint32_t K) {
  std::vector<Cluster> open;
  auto overlaps = [](const Cluster& c, const std::vector<uint32_t>& pos) {
    for (uint32_t p : pos)
      if (std::find(c.pos.begin(), c.pos.end(), p) != c.pos.end()) return true;
    return false;
  };
  auto flush_overlapping = [&](const std::vector<uint32_t>& pos) -> int {
    for (size_t i = 0; i < open.size();) {
      if (overlaps(open[i], pos)) {
        QCHK(flush_cluster<T>(s, run, open[i]));
        open.erase(open.begin() + i);
      } else {
        ++i;
      }
    }
    return QIP_OK;
  };
  for (uint64_t i = 0; i < count; ++i) {
    FlatOp f;
    int rc = flatten_op(s->n, &ops[i], false, &f);
    if (rc != QIP_OK) {
      std::string msg = g_last_error;
      return fail(rc, "op %llu: %s", (unsigned long long)i, msg.c_str());
    }
    std::vector<uint32_t> pos;
    std::vector<cd> m;
    if (!op_to_dense<T>(s->n, f, K, &pos, &m)) {
      // not fusable (too many qubits / repeated indices): everything it touches goes first
      std::vector<uint32_t> all;
      for (uint32_t j = 0; j < f.k_all; ++j) all.push_back(s->n - 1 - (uint32_t)f.outer->indices[j]);
      QCHK(flush_overlapping(all));
      QCHK(apply_op_t<T>(s, &ops[i], run));
      continue;
    }
    std::vector<size_t> hit;
    size_t union_size = pos.size();
    for (size_t c = 0; c < open.size(); ++c)
      if (overlaps(open[c], pos)) {
        hit.push_back(c);
        for (uint32_t p : open[c].pos)
          if (std::find(pos.begin(), pos.end(), p) == pos.end()) ++union_size;
      }
    if (hit.empty()) {
      // disjoint from every open cluster: join the fullest one that still has room
      size_t best = open.size();
      for (size_t c = 0; c < open.size(); ++c)
        if (open[c].pos.size() + pos.size() <= K && (best == open.size() || open[c].pos.size() > open[best].pos.size()))
          best = c;
      if (best == open.size()) {
        Cluster cl;
        cl.pos = {};
        cl.m = {cd(1, 0)};
        open.push_back(cl);
      }
      cluster_apply(&open[best], pos, m);
    } else if (union_size <= K) {
      // merge the overlapped clusters (mutually disjoint => their product is a Kronecker product)
      for (size_t h = 1; h < hit.size(); ++h) cluster_apply(&open[hit[0]], open[hit[h]].pos, open[hit[h]].m);
      for (size_t h = hit.size(); h-- > 1;) open.erase(open.begin() + hit[h]);
      cluster_apply(&open[hit[0]], pos, m);
    } else {
      QCHK(flush_overlapping(pos));
      Cluster cl;
      cl.pos = {};
      cl.m = {cd(1, 0)};
      cluster_apply(&cl, pos, m);
      open.push_back(cl);
    }
  }
  for (const Cluster& cl : open) QCHK(flush_cluster<T>(s, run, cl));
  return QIP_OK;
}

// ---------------------------------------------------------------------------------------
// Segment-specialised tile sweeps (option "tile_jit"): the interpreter k_tile_passes spends most of its issue slots
// on decoding — per gate and per wave ~54 scalar + ~58 vector instructions that only depend on the segment
// (profiles/r01_tile_pmc.md).  Here the host writes the segment out as straight-line HIP source — the same load /
// pass / store skeleton, one call of the very same pass_* helper per gate with the gate descriptor as a constexpr
// value — and has it compiled with hiprtc against the embedded qip_kernels.h (qip_jit.hip).  Every op code, bit position, control mask,
// zero / real / X flag folds away; what is left per gate is its arithmetic, operation for operation what the
// interpreter executes, so results are bit-identical.  Kernels are cached per process by their source text, so a
// circuit replayed many times (programs, variational loops with fixed angles) compiles once (~0.3-1 s per segment).
// ---------------------------------------------------------------------------------------
template <typename T> static std::string fnum(T v) {
  char buf[64];
  if (std::is_same<T, double>::value) snprintf(buf, sizeof buf, "%.17g", (double)v);
  else snprintf(buf, sizeof buf, "%.9gf", (double)v);
  std::string r = buf;
  // a bare integer literal would not be floating point ("1" / "1f")
  if (std::is_same<T, double>::value && r.find_first_of(".eEn") == std::string::npos) r += ".0";
  if (!std::is_same<T, double>::value && r.find_first_of(".eEn") == std::string::npos) r.insert(r.size() - 1, ".0");
  return r;
}

// ---- the segment source both tile shapes write alike --------------------------------------------------------------------------
// A gate as the writers consume it, resolved against its pass: the call it makes and the register-index bits of its targets.
// SEG_OTHER: the call is the shape's own (the dense 2- and 3-qubit gates: narrow and wide read their matrices differently).
enum SegCall { SEG_OTHER, SEG_DIAG_UNIFORM, SEG_DIAG_LANE, SEG_DIAG_LANE_CTL, SEG_DIAG_REG, SEG_DENSE, SEG_DENSE_LANE, SEG_SWAP };
template <typename T> struct SegGate {
  TileGate<T> g;  // as its literal shows it: cm_reg / cm_lane = its controls on register / lane bits
  SegCall call = SEG_OTHER;
  int j[2] = {0, 0};
  const TileDiagSpec<T>* spec = nullptr;  // a kind-5 gate (diagonal on two / three op bits): its table and bits
};

template <typename T> struct SegWriter {
  // `params` (option "tile_jit" = 2, see tile_jit_source): every number that is not exactly 0 or +-1 becomes a read of P[k]
  std::vector<T>* params;
  std::string o;
  explicit SegWriter(std::vector<T>* p) : params(p) {}
  static std::string N(uint64_t v) { return std::to_string(v); }
  static std::string U(uint64_t v) { return std::to_string(v) + "ull"; }
  static constexpr const char* kLaneArgs = "g.cm_lane != 0u, (tb & g.cm_lane) == g.cm_lane";  // (the calls with lane controls)
  void L(const std::string& line) { o += line; o += "\n"; }
  std::string comp(T v) {
    if (!params || v == (T)0 || v == (T)1 || v == (T)-1) return fnum<T>(v);  // (a -0 prints as -0.0 and stays one)
    params->push_back(v);
    return "P[" + N(params->size() - 1) + "]";
  }
  std::string amp(amp_t<T> a) {
    const std::string re = comp(a.x);  // fixed evaluation order: the parameter numbering is part of the source
    const std::string im = comp(a.y);
    return "{" + re + ", " + im + "}";
  }
  std::string matrix_literal(const amp_t<T>* m, int cnt) {
    std::string r = "const A M[" + N(cnt) + "] = {";
    for (int k = 0; k < cnt; ++k) r += amp(m[k]) + (k + 1 < cnt ? ", " : "}; ");
    return r;
  }
  // a gate's 4x4 / 8x8 matrix: one contiguous block of the parameter array, or literals.  r4: read row by row through a pointer
  // like the interpreter does (wave-uniform scalar loads as they are needed).  Spelt out as 64 named components, all 128 scalars
  // of a dense 3-qubit gate were live at once: the dense-k3 Grover segments ran SLOWER compiled than interpreted (108.9 vs 101.4 ms).
  std::string matrix(const amp_t<T>* m, int cnt) {
    if (!params) return matrix_literal(m, cnt);
    if (params->size() & 1) params->push_back((T)0);  // (16-byte alignment of the block for Complex<f64>)
    const size_t off = params->size();
    for (int k = 0; k < cnt; ++k) {
      params->push_back(m[k].x);
      params->push_back(m[k].y);
    }
    return "const A* __restrict__ M = reinterpret_cast<const A*>(P + " + N(off) + "); ";
  }
  // includes, tile_base, dst_of (a packed store), the signature and the kernel's first lines up to its shared-memory buffer `buf`
  void prologue(const Ins& ins, uint32_t p5, const TileStorePerm* fold, const char* bounds, bool sliced, const std::string& buf, bool nt) {
    L("#include \"qip_kernels.h\"");
    L("using namespace qipk;");
    L(std::string("typedef ") + (std::is_same<T, double>::value ? "double" : "float") + " T;");
    L("typedef amp_t<T> A;");
    // tile number -> amplitude index of the tile's element 0: insert_bits with the positions as literals
    L("__device__ __forceinline__ uint64_t tile_base(uint64_t t) {");
    L("  uint64_t w = t << kTileLow;");
    for (uint32_t j = 0; j < ins.npos; ++j) {
      const std::string p = N(ins.pos[j]);
      L("  w = ((w >> " + p + ") << " + N(ins.pos[j] + 1) + ") | (w & ((1ull << " + p + ") - 1ull));");
    }
    if (ins.ormask) L("  w |= " + U(ins.ormask) + ";");
    if (p5 != 5u)  // split rows (see tile_block_base): `ins` was opened with 5 standing for p5; the two bits trade places now
      L("  w = (w & ~(1ull << " + N(p5) + ")) | (((w >> " + N(p5) + ") & 1ull) << 5);");
    L("  return w;");
    L("}");
    if (fold && fold->g) {
      // the tiles are stored elsewhere, packed for the multi-GPU exchange (TileStorePerm): the positions as literals.  The map
      // moves index bits, so it distributes over wave base | access bits | lane offset
      L("__device__ __forceinline__ uint64_t dst_of(uint64_t x) {");
      L("  uint64_t top = 0;");
      for (uint32_t t = 0; t < fold->g; ++t) L("  top |= ((x >> " + N(fold->sel[t]) + ") & 1ull) << " + N(fold->Lg + t) + ";");
      for (uint32_t t = 0; t < fold->g; ++t) {
        const std::string p = N(fold->sel_desc[t]);
        L("  x = ((x >> " + N(fold->sel_desc[t] + 1) + ") << " + p + ") | (x & ((1ull << " + p + ") - 1ull));");
      }
      L("  return x | top;");
      L("}");
    }
    // `sliced` (r5): the sweep is launched in parts — `ins` has the slice positions opened too, and the kernel's second parameter
    // is the part's bits at those positions (ORed into every block's base) instead of the unused tile count
    L(std::string("extern \"C\" __global__ __launch_bounds__(") + bounds + ") void qip_segment(A* __restrict__ st, uint64_t " + (sliced ? "slice_or" : "ntiles") +
      (params ? ", const T* __restrict__ P" : "") + (fold && fold->g ? ", A* __restrict__ out" : "") + ") {");
    L("  extern __shared__ __attribute__((aligned(16))) unsigned char " + buf + "_raw[];");
    L("  A* " + buf + " = reinterpret_cast<A*>(" + buf + "_raw);");
    L(std::string("  constexpr bool NT = ") + (nt ? "true" : "false") + ";");
    L("  const uint32_t tid = threadIdx.x, lane = tid & 63u;");
    L("  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);");
  }
  // the pass's table c[]: register index i of a lane's elements holds tile offset c[i] (bit j of i = tile bit bits[j])
  std::vector<uint32_t> reg_table(const uint32_t* bits, int nbits) {
    std::vector<uint32_t> c(1u << nbits, 0u);
    std::string cs = "    const uint32_t c[" + N(c.size()) + "] = {";
    for (size_t i = 0; i < c.size(); ++i) {
      for (int j = 0; j < nbits; ++j)
        if ((i >> j) & 1) c[i] |= 1u << bits[j];
      cs += N(c[i]) + "u" + (i + 1 < c.size() ? ", " : "};");
    }
    L(cs);
    return c;
  }
  // `merge_diag` (option "tile_merge", tile = 2 only: 1e-12 bar): a RUN of >= 3 consecutive diagonal gates — they all commute —
  // is applied as products.  Every gate contributes a factor (per lane: its lane-bit and outside-the-tile conditions select
  // between its entry and 1) to the SET of the lane's elements its register-bit conditions pick; factors of one set are
  // multiplied together first, then each element takes the product of its sets: QFT's 29 controlled phases after an H cost
  // ~29 + 4 complex products per lane instead of 4 x 29.  The run starts at gs[k] (gate number gi); returns how many gates it
  // took, 0 when no such run starts there.
  uint32_t diag_run(const std::vector<SegGate<T>>& gs, size_t k, uint32_t gi, const std::vector<uint32_t>& c) {
    size_t ke = k;
    while (ke < gs.size() && (gs[ke].g.kind == 1 || gs[ke].spec)) ++ke;
    if (ke - k < 3) return 0;
    std::vector<uint32_t> sets;  // element masks, in order of first appearance: F<k> is the running product of set k
    L("    {  // gates " + N(gi) + " .. " + N(gi + (ke - k) - 1) + ": one run of diagonal gates");
    // (each factor joins its product at once: short live ranges.  `ucond`: a block-uniform condition — a control outside the
    // tile — stays a BRANCH around the product, as in the gate-by-gate form: no work at all where the control reads 0)
    auto add = [&](uint32_t mask, const std::string& expr, const std::string& ucond) {
      if (!mask) return;
      const std::string open = ucond.empty() ? "" : "if (" + ucond + ") { QIP_KEEP_BRANCH(); ", close = ucond.empty() ? "" : " }";
      for (size_t s = 0; s < sets.size(); ++s)
        if (sets[s] == mask) {
          L("      " + open + "F" + N(s) + " = cmul(F" + N(s) + ", " + expr + ");" + close);
          return;
        }
      if (ucond.empty()) L("      A F" + N(sets.size()) + " = " + expr + ";");
      else L("      A F" + N(sets.size()) + " = {(T)1, (T)0}; " + open + "F" + N(sets.size()) + " = " + expr + ";" + close);
      sets.push_back(mask);
    };
    for (size_t kj = k; kj < ke; ++kj) {
      const TileGate<T>& d = gs[kj].g;
      if (gs[kj].spec) {  // diagonal on two / three op bits: every non-unit entry is a factor of the elements and lanes it belongs to
        for (const TileDiagStep<T>& st : tile_diag_steps<T>(*gs[kj].spec, d, c.back())) {
          uint32_t mask = 0;
          for (size_t i = 0; i < c.size(); ++i)
            if ((c[i] & st.reg_mask) == st.reg_val) mask |= 1u << i;
          const std::string f = "A" + amp(st.f);
          add(mask, st.lane_mask ? "tile_sel(((tb & " + N(st.lane_mask) + "u) == " + N(st.lane_val) + "u), " + f + ", A{(T)1, (T)0})" : f,
              st.omask ? "(base & " + U(st.omask) + ") == " + U(st.oval) : "");
        }
        continue;
      }
      uint32_t ok = 0;  // elements whose register-bit controls are all 1
      for (size_t i = 0; i < c.size(); ++i)
        if ((c[i] & d.cm_reg) == d.cm_reg) ok |= 1u << i;
      const std::string m0 = amp(d.m[0]), m1 = amp(d.m[1]);
      const bool u0 = d.m[0].x == (T)1 && d.m[0].y == (T)0, u1 = d.m[1].x == (T)1 && d.m[1].y == (T)0;
      // the conditions every element of the lane shares: controls outside the tile (block-uniform: a branch) and on lane
      // bits (a select between the entry and 1)
      const std::string ucond = d.omask ? "(base & " + U(d.omask) + ") == " + U(d.omask) : "";
      const std::string lcond = d.cm_lane ? "((tb & " + N(d.cm_lane) + "u) == " + N(d.cm_lane) + "u)" : "";
      auto guarded = [&](const std::string& f) { return lcond.empty() ? f : "tile_sel(" + lcond + ", " + f + ", A{(T)1, (T)0})"; };
      if (gs[kj].call == SEG_DIAG_REG) {
        uint32_t half1 = 0;
        for (size_t i = 0; i < c.size(); ++i)
          if ((i >> gs[kj].j[0]) & 1) half1 |= 1u << i;
        if (!u0) add(ok & ~half1, guarded("A" + m0), ucond);
        if (!u1) add(ok & half1, guarded("A" + m1), ucond);
      } else {  // the target is a lane bit or lies outside the tile: one factor for every element the controls pick
        const std::string one = d.b0 == kTileOutside ? "(((base >> " + N(d.tpos_out) + ") & 1ull) != 0)" : "(((tb >> " + N(d.b0) + ") & 1u) != 0)";
        add(ok, guarded("tile_sel(" + one + ", A" + m1 + ", A" + m0 + ")"), ucond);
      }
    }
    for (size_t i = 0; i < c.size(); ++i)
      for (size_t si = 0; si < sets.size(); ++si)
        if ((sets[si] >> i) & 1u) L("      e[" + N(i) + "] = cmul(F" + N(si) + ", e[" + N(i) + "]);");
    L("    }");
    return (uint32_t)(ke - k);
  }
  // A kind-5 gate: one statement per table entry that is not the unit (resolved here, as for kind 1), sub-index ascending — the
  // elements whose register bits read the entry's sub-index (and the controls 1) take cmul(f, e), f = (1, 0) on lanes whose lane
  // bits read otherwise, under a branch where bits outside the tile decide.  The statements select disjoint amplitudes: each one
  // meets its own entry once, by k_diag's unfused product.  Entries other than 0 / +-1 are kernel data.  Opens the gate's block
  // (the caller closes it with end_gate); returns true when a statement sits under a block-uniform branch.
  bool diag_item(uint32_t gi, const TileGate<T>& g, const TileDiagSpec<T>& sp, const std::vector<uint32_t>& c) {
    L("    {  // gate " + N(gi) + ": diagonal on " + N(sp.k) + " bits");
    bool uniform = false;
    for (const TileDiagStep<T>& st : tile_diag_steps<T>(sp, g, c.back())) {
      std::string body = "A f = " + amp(st.f) + "; ";
      if (st.lane_mask)
        body += "{ const bool lane_ok = (tb & " + N(st.lane_mask) + "u) == " + N(st.lane_val) + "u; f.x = lane_ok ? f.x : (T)1; f.y = lane_ok ? f.y : (T)0; } ";
      for (size_t i = 0; i < c.size(); ++i)
        if ((c[i] & st.reg_mask) == st.reg_val) body += "e[" + N(i) + "] = cmul(f, e[" + N(i) + "]); ";
      if (st.omask) L("      if ((base & " + U(st.omask) + ") == " + U(st.oval) + ") { QIP_KEEP_BRANCH(); " + body + "}");
      else L("      { " + body + "}");
      uniform = uniform || st.omask != 0;
    }
    return uniform;
  }
  void gate_literal(uint32_t gi, const TileGate<T>& g) {
    L("    {  // gate " + N(gi));
    const std::string m0 = amp(g.m[0]), m1 = amp(g.m[1]), m2 = amp(g.m[2]), m3 = amp(g.m[3]);
    L(std::string("      ") + (params ? "const" : "constexpr") + " TileGate<T> g = {" + N(g.kind) + "u, " + N(g.b0) + "u, " + N(g.b1) + "u, " + N(g.cmask) + "u, " +
      N(g.nz) + "u, " + N(g.tpos_out) + "u, " + U(g.omask) + ", " + N(g.op) + "u, " + N(g.cm_reg) + "u, " + N(g.cm_lane) + "u, 0u, {" + m0 + ", " + m1 + ", " +
      m2 + ", " + m3 + "}};");
  }
  // Diagonal gates: which entries are the unit is known HERE (a unit is always written as a literal, also in the parametrised
  // form), so the helpers' run-time "unit entries leave the amplitude untouched" tests are resolved by the generator: an entry
  // that is the unit emits nothing.  Per amplitude the products are those of pass_diag / the interpreter's switch, in the same order.
  static std::string gate_call(const SegGate<T>& r) {
    const TileGate<T>& g = r.g;
    const bool u0 = g.m[0].x == (T)1 && g.m[0].y == (T)0, u1 = g.m[1].x == (T)1 && g.m[1].y == (T)0;
    const std::string lane_guard = "{ const bool lane_ok = (tb & g.cm_lane) == g.cm_lane; f.x = lane_ok ? f.x : (T)1; f.y = lane_ok ? f.y : (T)0; } ";
    std::string out;
    switch (r.call) {
      case SEG_DIAG_UNIFORM: {
        const std::string s0 = u0 ? "" : "pass_scale<T, 0, -1>(g.m[0], e, c, g.cm_reg);", s1 = u1 ? "" : "pass_scale<T, 0, -1>(g.m[1], e, c, g.cm_reg);";
        return "if ((base >> g.tpos_out) & 1ull) { " + s1 + " } else { " + s0 + " }";
      }
      case SEG_DIAG_LANE:
      case SEG_DIAG_LANE_CTL:
        return std::string("const bool one = ") + (g.b0 == kTileOutside ? "((base >> g.tpos_out) & 1ull) != 0" : "((tb >> g.b0) & 1u) != 0") +
               "; A f = tile_sel(one, g.m[1], g.m[0]); " + (r.call == SEG_DIAG_LANE_CTL ? lane_guard : "") + "pass_scale<T, 0, -1>(f, e, c, g.cm_reg);";
      case SEG_DIAG_REG:
        for (int half = 0; half < 2; ++half)
          if (!(half == 0 ? u0 : u1))
            out += "{ A f = g.m[" + N(half) + "]; " + (g.cm_lane ? lane_guard : "") + "pass_scale<T, " + N(r.j[0]) + ", " + N(half) + ">(f, e, c, g.cm_reg); } ";
        return out;
      case SEG_DENSE: return "pass_dense<T, " + N(r.j[0]) + ">(g, e, c, g.cm_reg);";
      case SEG_DENSE_LANE: return "pass_dense_lane<T, " + N(r.j[0]) + ">(g, e, c, g.cm_reg, (tb & g.cm_lane) == g.cm_lane);";
      case SEG_SWAP: return "pass_swap<T, " + N(r.j[0]) + ", " + N(r.j[1]) + ">(e, c, g.cm_reg, " + kLaneArgs + ");";
      default: return out;
    }
  }
  void guarded(const TileGate<T>& g, const std::string& call) {
    if (g.omask) L("      if ((base & g.omask) == g.omask) { " + call + " }");  // an outside control is 0 for this whole tile
    else L("      { " + call + " }");
  }
  void end_gate() {
    // one gate at a time: left alone hipcc interleaves neighbouring gates up to the register budget of the launch bound and
    // then spills (16 - 104 bytes of scratch per lane in the configs[1] segments, 104 vs 90 ms for the circuit)
    L("      __builtin_amdgcn_sched_barrier(0);");
    L("    }");
  }
};
// The segment as HIP source (see the block comment above).  Mirrors k_tile_passes statement by statement.
// (Measured in round 3 and NOT adopted: persistent blocks that prefetch the next tile — into registers, or by LDS-DMA into a
// second tile slot.  The skeleton of a sweep already overlaps its phases through the five resident blocks per CU: with the
// passes' arithmetic scaled from 0 to 6000 f64 operations per lane the time is max(HBM time, issue time) + ~1 ms, and a
// light sweep's time is set by which five high positions the tile holds (5.2 - 6.7 ms), not by the block structure;
// tools/tune_tile.hip, profiles/r03_tile_skeleton.md.)
//
// `params` (option "tile_jit" = 2): the segment's STRUCTURE is compiled, its numbers are kernel data.  Every matrix component
// that is not exactly 0 or +-1 becomes a read of P[k] (a wave-uniform scalar load from the device arena) and its value goes
// to `params`; zeros and units stay literals, and the flags the host derives from them (non-zero mask, real / X shapes) stay
// constants, so the same folding happens and the arithmetic per amplitude is unchanged: bit-identical to "tile_jit" = 1.
// A variational loop that updates its rotation angles produces the same source every time and re-uses the compiled kernel;
// only a value that newly becomes (or stops being) 0 / +-1 changes the structure and compiles again.
template <typename T>
static std::string tile_jit_source(const TileSegmentPlan<T>& plan, const Ins& ins, bool nt, int remap = 0, std::vector<T>* params = nullptr,
                                   bool merge_diag = false, const TileStorePerm* fold = nullptr, bool sliced = false) {
  SegWriter<T> w(params);
  auto L = [&](const std::string& line) { w.L(line); };
  const auto N = SegWriter<T>::N, U = SegWriter<T>::U;
  const TilePassDesc& d = plan.pd;
  w.prologue(ins, d.p5, fold, "kTileBlock, 5", sliced, "tile", nt);
  L("  uint64_t wave_off = 0;");
  for (int j = 0; j < kTileWaveBits; ++j) L("  wave_off |= (uint64_t)((wave >> " + N(j) + ") & 1u) << " + N(d.hpos[j]) + ";");
  L("  const uint32_t slot_tid = tile_slot<A>(tid);");
  auto ub = [&](int u) {
    uint64_t off = 0;
    for (int b = 0; b < 3; ++b)
      if ((u >> b) & 1) off |= 1ull << d.hpos[kTileWaveBits + b];
    return U(off);
  };
  L("  A x[8];");
  if (!sliced) L("  (void)ntiles;");
  L("  uint64_t blk = blockIdx.x + (uint64_t)blockIdx.y * gridDim.x;");
  // (tuning aid, global option "tile_remap": the 2^r blocks one XCD receives in a row take ADJACENT tiles; measured slower)
  if (remap == 2) L("  blk = (blk & ~31ull) | ((blk & 7ull) << 2) | ((blk >> 3) & 3ull);");
  if (remap == 3) L("  blk = (blk & ~63ull) | ((blk & 7ull) << 3) | ((blk >> 3) & 7ull);");
  if (remap >= 16) {
    // XCD-aware order (global option "tile_remap" = 4; remap = 16 + J here): consecutive block numbers go round-robin over
    // the 8 XCDs, so block bits 0..2 name the XCD.  They drive three tile-number bits that stand for HIGH free positions
    // (the first three at or above amplitude position 16), the remaining block bits walk the other free positions upwards:
    // each XCD sweeps its own far-apart region with neighbouring 1-KiB rows in consecutive blocks, instead of all eight
    // interleaving on the same rows.  Tuning aid, off by default: on the bare sweep skeleton (tools/tune_tile "order") it is
    // worth 2 - 13 % on tiles whose five positions are scattered, on real segments it is not (configs[1] 69.3 -> 69.7 ms,
    // QFT 36.3 -> 37.9 ms in the HBM-bound tile mode: profiles/r03_tile_skeleton.md, section 4).
    const std::string J = std::to_string(remap - 16);
    L("  blk = ((blk >> 3) & ((1ull << " + J + ") - 1ull)) | ((blk & 7ull) << " + J + ") | (((blk >> 3) >> " + J + ") << (" + J + " + 3));");
  }
  L(std::string("  const uint64_t base = tile_base(blk)") + (sliced ? " | slice_or" : "") + ", wbase = base | wave_off;");
  L("  const uint32_t lane_off = tile_lane_off(lane, " + N(d.p5) + "u);");
  for (int u = 0; u < 8; ++u) L("  x[" + N(u) + "] = ldg<NT>(st + (wbase | " + ub(u) + ") + lane_off);");
  L("  const uint32_t tidv = tid;");
  for (int u = 0; u < 8; ++u) L("    tile[slot_tid ^ tile_slot<A>(" + N(u) + "u << kTileLaneBits)] = x[" + N(u) + "];");
  L("  __syncthreads();");
  for (uint32_t pi = 0; pi < d.npasses; ++pi) {
    const TilePass& ps = d.pass[pi];
    L("  {  // pass " + N(pi));
    // the pass's LDS addresses depend on the lane id alone: left alone hipcc computes those of EVERY pass up front and keeps
    // them live (spills in segments of many passes); an opaque copy of the id per pass pins them behind the barrier before it
    L("    uint32_t tidp = tidv;");
    L("    asm volatile(\"\" : \"+v\"(tidp));");
    L("    uint32_t tb = 0;");
    for (int k = 0; k < kTileLaneBits; ++k) L("    tb |= ((tidp >> " + N(k) + ") & 1u) << " + N((ps.lanepos >> (4 * k)) & 15ull) + ";");
    L("    const uint32_t slot_tb = tile_slot<A>(tb);");
    const std::vector<uint32_t> c = w.reg_table(ps.pb, 3);
    L("    A e[8];");
    for (int i = 0; i < 8; ++i) L("    e[" + N(i) + "] = tile[slot_tb ^ tile_slot<A>(c[" + N(i) + "])];");
    // the gates as the pass resolved them (TOP_*): the host already knows which bits are register bits
    std::vector<SegGate<T>> gs;
    for (uint32_t gi = ps.first; gi < ps.first + ps.count; ++gi) {
      const TileGate<T>& g = plan.gates[gi];
      const uint32_t op = g.op;
      static const int sa[3] = {0, 0, 1}, sb[3] = {1, 2, 2};  // TOP_SWAP_01, _02, _12
      SegGate<T> r = {g};
      if (op == TOP_DIAG_UNIFORM) r.call = SEG_DIAG_UNIFORM;
      else if (op == TOP_DIAG_LANE) r.call = SEG_DIAG_LANE;
      else if (op == TOP_DIAG_LANE_CTL) r.call = SEG_DIAG_LANE_CTL;
      else if (op >= TOP_DIAG_REG0 && op <= TOP_DIAG_REG2) r = {g, SEG_DIAG_REG, {(int)(op - TOP_DIAG_REG0)}};
      else if (op >= TOP_DENSE0 && op <= TOP_DENSE2) r = {g, SEG_DENSE, {(int)(op - TOP_DENSE0)}};
      else if (op >= TOP_DENSE_LANE0 && op <= TOP_DENSE_LANE2) r = {g, SEG_DENSE_LANE, {(int)(op - TOP_DENSE_LANE0)}};
      else if (op >= TOP_SWAP_01 && op <= TOP_SWAP_12) r = {g, SEG_SWAP, {sa[op - TOP_SWAP_01], sb[op - TOP_SWAP_01]}};
      if (g.kind == (uint32_t)kTileKindDiagK) r.spec = &plan.diags[g.nz];
      gs.push_back(r);
    }
    for (size_t k = 0; k < gs.size(); ++k) {
      const uint32_t gi = ps.first + (uint32_t)k;
      if (merge_diag)
        if (const uint32_t run = w.diag_run(gs, k, gi, c)) {
          k += run - 1;
          continue;
        }
      const TileGate<T>& g = gs[k].g;
      if (gs[k].spec) {
        w.diag_item(gi, g, *gs[k].spec, c);
        w.end_gate();
        continue;
      }
      w.gate_literal(gi, g);
      std::string call = SegWriter<T>::gate_call(gs[k]);
      static const int ja[6] = {0, 0, 1, 1, 2, 2}, jb[6] = {1, 2, 0, 2, 0, 1};
      if (g.op >= TOP_DENSE2Q_01 && g.op <= TOP_DENSE2Q_21) {
        // (the 4x4 matrix as components, also when parametrised: unlike the wide tile's block)
        const uint32_t v = g.op - TOP_DENSE2Q_01;
        call = w.matrix_literal(&plan.mats[16 * g.nz], 16) + "pass_dense2<T, " + N(ja[v]) + ", " + N(jb[v]) + ">(M, e, c, g.cm_reg, " + SegWriter<T>::kLaneArgs + ");";
      } else if (g.op >= TOP_DENSE3Q_012 && g.op <= TOP_DENSE3Q_210) {
        const uint32_t v = g.op - TOP_DENSE3Q_012;
        call = w.matrix(&plan.mats[16 * g.nz], 64) + "pass_dense3<T, " + N(ja[v]) + ", " + N(jb[v]) + ", " + N(3 - ja[v] - jb[v]) + ">(M, e, " +
               SegWriter<T>::kLaneArgs + ");";
      }
      w.guarded(g, call);
      w.end_gate();
    }
    for (int i = 0; i < 8; ++i) L("    tile[slot_tb ^ tile_slot<A>(c[" + N(i) + "])] = e[" + N(i) + "];");
    L("    __syncthreads();");
    L("  }");
  }
  for (int u = 0; u < 8; ++u)
    if (fold && fold->g)
      L("  stg<NT>(out + dst_of(wbase | " + ub(u) + ") + dst_of(lane_off), tile[slot_tid ^ tile_slot<A>(" + N(u) + "u << kTileLaneBits)]);");
    else
      L("  stg<NT>(st + (wbase | " + ub(u) + ") + lane_off, tile[slot_tid ^ tile_slot<A>(" + N(u) + "u << kTileLaneBits)]);");
  L("}");
  return w.o;
}

// ---- wide tiles (r4, option "tile_wide"): the segment's source for the register-resident 13-bit tile ------------------------------
// One array of 32 amplitudes per arrangement (straight-line code with constant indices: the arrays are names, not memory — a
// transposition costs its LDS traffic and two barriers per quarter, no register moves); the gates go through the same helpers
// as the 11-bit sweeps (pass_dense, pass_scale, pass_swap, pass_dense2, pass_dense3w over 32 elements: the products and sums of
// the gate-by-gate kernels in the same order — a circuit-order segment stays IEEE-equal to them).
// `pin` (global option "tile_wide_pin", debug mode bit 256; r4, profiles/r04_wide_tiles.md): after every gate that
// is applied under a block-uniform branch (a control / selector outside the tile) the 32 amplitudes pass through an empty asm with
// "+v" constraints.  Semantically nothing; it stops the register allocator from keeping both versions of the tile alive across the join:
// Clifford+T's first segment 175 VGPR spills -> 0 (9238 -> 8646 instructions), QFT's 32 -> 0; configs[1] (no spills) + 4 % instructions.
// On the GPU (tools/exp_wide_pin.py, n = 30, tile = 1, medians of 5): a 72-gate Clifford+T prefix 25.92 -> 23.90 ms (-7.8 %), a 60-gate
// configs[1] prefix 17.42 -> 17.49 ms (noise); results bit-identical.  Default on.
int64_t g_tile_wide_pin = 1;
// global option "tile_wide_dense3_inline" (debug mode bit 512; r4, OFF: compiled and register-checked without a GPU, never run on one):
// dense 3-qubit gates of a wide segment written out group by group instead of through pass_dense3w — the dense-k3 Grover variant's first
// wide segment: 528 B of stack per lane -> 0 (tools/jit_segment_resources.py, mode | 512).  The next round's first measurement.
int64_t g_tile_wide_dense3_inline = 1;  // r5: run on MI355X — bit-identical to pass_dense3w, dense-k3 Grover on wide tiles 109.9 -> 77.5 ms (narrow: 88.2): on
template <typename T>
static std::string wide_jit_source(const WidePlan<T>& plan, const Ins& ins, bool nt, std::vector<T>* params, bool merge_diag = false, bool pin = false,
                                   bool dense3_inline = false, bool sliced = false, const TileStorePerm* fold = nullptr) {
  constexpr uint32_t SW = sizeof(amp_t<T>) == 16 ? 4u : 5u;  // tile_slot's fold width
  auto slot = [&](uint32_t t) { return t ^ ((t >> SW) & ((1u << SW) - 1u)); };
  SegWriter<T> w(params);
  auto L = [&](const std::string& line) { w.L(line); };
  const auto N = SegWriter<T>::N, U = SegWriter<T>::U;
  w.prologue(ins, plan.p5, fold, "256, 2", sliced, "buf", nt);
  if (!sliced) L("  (void)ntiles;");
  L(std::string("  const uint64_t base = tile_base(blockIdx.x + (uint64_t)blockIdx.y * gridDim.x)") + (sliced ? " | slice_or;" : ";"));
  L("  const uint64_t wbase = base | ((uint64_t)(wave & 1u) << " + N(plan.high[0]) + ") | ((uint64_t)(wave >> 1) << " + N(plan.high[1]) + ");");
  L("  const uint32_t lane_off = tile_lane_off(lane, " + N(plan.p5) + "u);");
  auto ub = [&](int u) {
    uint64_t off = 0;
    for (int b = 0; b < kWideRegBits; ++b)
      if ((u >> b) & 1) off |= 1ull << plan.high[2 + b];
    return U(off);
  };
  L("  A e0[32];");
  for (int u = 0; u < 32; ++u) L("  e0[" + N(u) + "] = ldg<NT>(st + (wbase | " + ub(u) + ") + lane_off);");
  L("  const uint32_t tidv = tid;");
  for (size_t pi = 0; pi < plan.passes.size(); ++pi) {
    const WidePass& ps = plan.passes[pi];
    const std::string e = "e" + N(pi);
    auto jof = [&](uint32_t bit) {
      for (int j = 0; j < kWideRegBits; ++j)
        if (ps.R[j] == bit) return j;
      return -1;
    };
    if (ps.transposed) {
      const WidePass& pa = plan.passes[pi - 1];
      const std::string ea = "e" + N(pi - 1);
      L("  A " + e + "[32];");
      L("  {  // transposition into arrangement " + N(pi));
      L("    uint32_t tidp = tidv;");
      L("    asm volatile(\"\" : \"+v\"(tidp));");
      L("    uint32_t wa = 0, rb = 0;");
      for (int k = 0; k < 8; ++k) {
        L("    wa |= ((tidp >> " + N(k) + ") & 1u) << " + N(ps.bufpos[pa.L[k]]) + ";");
        L("    rb |= ((tidp >> " + N(k) + ") & 1u) << " + N(ps.bufpos[ps.L[k]]) + ";");
      }
      L("    const uint32_t swa = tile_slot<A>(wa), srb = tile_slot<A>(rb);");
      auto split = [&](const WidePass& wp, int (&jq)[2], int (&jo)[3]) {
        int no = 0;
        for (int j = 0; j < kWideRegBits; ++j) {
          if (wp.R[j] == ps.q[0]) jq[0] = j;
          else if (wp.R[j] == ps.q[1]) jq[1] = j;
          else jo[no++] = j;
        }
      };
      int jqa[2] = {0, 0}, joa[3] = {0, 0, 0}, jqb[2] = {0, 0}, job[3] = {0, 0, 0};
      split(pa, jqa, joa);
      split(ps, jqb, job);
      // two buffer halves: quarter v + 1 is written while quarter v is read (write 0 | barrier | read 0, write 1 | barrier |
      // read 1, write 2 | ... ): four barriers per transposition instead of seven
      auto emit_write = [&](int qv) {
        for (int m = 0; m < 8; ++m) {
          uint32_t r = ((uint32_t)(qv & 1) << jqa[0]) | ((uint32_t)(qv >> 1) << jqa[1]), ci = 0;
          for (int i = 0; i < 3; ++i)
            if ((m >> i) & 1) {
              r |= 1u << joa[i];
              ci |= 1u << ps.bufpos[pa.R[joa[i]]];
            }
          L("    buf[" + N((qv & 1) * 2048) + "u + (swa ^ " + N(slot(ci)) + "u)] = " + ea + "[" + N(r) + "];");
        }
      };
      auto emit_read = [&](int qv) {
        for (int m = 0; m < 8; ++m) {
          uint32_t r = ((uint32_t)(qv & 1) << jqb[0]) | ((uint32_t)(qv >> 1) << jqb[1]), ci = 0;
          for (int i = 0; i < 3; ++i)
            if ((m >> i) & 1) {
              r |= 1u << job[i];
              ci |= 1u << ps.bufpos[ps.R[job[i]]];
            }
          L("    " + e + "[" + N(r) + "] = buf[" + N((qv & 1) * 2048) + "u + (srb ^ " + N(slot(ci)) + "u)];");
        }
      };
      emit_write(0);
      for (int qv = 0; qv < 4; ++qv) {
        L("    __syncthreads();");
        emit_read(qv);
        if (qv < 3) emit_write(qv + 1);
      }
      L("  }");
      // (no barrier before the next transposition: its first write goes to half 0, whose last reads — quarter 2 — lie before
      // the fourth barrier above; half 1 is next written after the next transposition's first barrier, behind everybody's
      // reads of quarter 3)
    } else if (pi > 0) {
      return std::string();  // (cannot happen: every pass after the first is a transposition)
    }
    if (ps.count == 0) continue;
    L("  {  // pass " + N(pi) + ": register bits = tile bits " + N(ps.R[0]) + "," + N(ps.R[1]) + "," + N(ps.R[2]) + "," + N(ps.R[3]) + "," + N(ps.R[4]));
    L("    uint32_t tidq = tidv;");
    L("    asm volatile(\"\" : \"+v\"(tidq));");
    L("    uint32_t tb = 0;");
    for (int k = 0; k < 8; ++k) L("    tb |= ((tidq >> " + N(k) + ") & 1u) << " + N(ps.L[k]) + ";");
    uint32_t rmask = 0;
    for (int j = 0; j < kWideRegBits; ++j) rmask |= 1u << ps.R[j];
    const std::vector<uint32_t> c = w.reg_table(ps.R, kWideRegBits);
    L("    A (&e)[32] = " + e + ";");
    // the gates resolved against this arrangement: controls split into register and lane bits, targets looked up as register
    // bits (op stays 0: no interpreter reads it)
    std::vector<SegGate<T>> gs;
    for (uint32_t gi = ps.first; gi < ps.first + ps.count; ++gi) {
      TileGate<T> g = plan.gates[gi];
      g.cm_reg = g.cmask & rmask;
      g.cm_lane = g.cmask & ~rmask;
      g.op = 0;
      const int J = g.b0 == kTileOutside ? -1 : jof(g.b0);
      SegGate<T> r = {g};
      if (g.kind == 1 && J >= 0) r = {g, SEG_DIAG_REG, {J}};
      else if (g.kind == 1) r.call = g.b0 == kTileOutside && !g.cm_lane ? SEG_DIAG_UNIFORM : g.cm_lane ? SEG_DIAG_LANE_CTL : SEG_DIAG_LANE;
      else if (g.kind == 0) r = {g, g.cm_lane ? SEG_DENSE_LANE : SEG_DENSE, {jof(g.b0)}};
      else if (g.kind == 2) r = {g, SEG_SWAP, {jof(g.b0), jof(g.b1)}};
      if (g.kind == (uint32_t)kTileKindDiagK) r.spec = &plan.diags[g.nz];
      gs.push_back(r);
    }
    for (size_t k = 0; k < gs.size(); ++k) {
      const uint32_t gi = ps.first + (uint32_t)k;
      if (merge_diag)
        if (const uint32_t run = w.diag_run(gs, k, gi, c)) {
          k += run - 1;
          continue;
        }
      const TileGate<T>& g = gs[k].g;
      if (gs[k].spec) {
        if (w.diag_item(gi, g, *gs[k].spec, c) && pin) {
          std::string pl = "     ";
          for (int i = 0; i < 32; ++i) pl += " asm volatile(\"\" : \"+v\"(e[" + N(i) + "].x), \"+v\"(e[" + N(i) + "].y));";
          L(pl);
        }
        w.end_gate();
        continue;
      }
      w.gate_literal(gi, g);
      std::string call = SegWriter<T>::gate_call(gs[k]);
      const amp_t<T>* M = g.kind >= 3 ? plan.mats.data() + 16 * g.nz : nullptr;  // (the matrix of a dense 2- or 3-qubit gate)
      if (g.kind == 3) {
        call = w.matrix(M, 16) + "pass_dense2<T, " + N(jof(g.b0)) + ", " + N(jof(g.b1)) + ">(M, e, c, g.cm_reg, " + SegWriter<T>::kLaneArgs + ");";
      } else if (g.kind == 4 && dense3_inline) {
        // The same fold as pass_dense3w, written out for the (at most four) groups this gate really touches, every index a literal.
        // pass_dense3w's loop over the 32 elements is not unrolled by the compiler at NE = 32: `e` is indexed at run time and the whole
        // tile of the lane lives in a 528-byte stack object (profiles/r04_jit_segment_resources.txt: dense-k3 Grover on wide tiles).
        const int JA = jof(g.b0), JB = jof(g.b1), JC = jof(g.tpos_out);
        call = w.matrix(M, 64);
        for (int base = 0; base < 32; ++base) {
          if (((base >> JA) & 1) || ((base >> JB) & 1) || ((base >> JC) & 1)) continue;
          if ((c[base] & g.cm_reg) != g.cm_reg) continue;
          auto idx = [&](int r) { return base | (((r >> 2) & 1) << JA) | (((r >> 1) & 1) << JB) | ((r & 1) << JC); };
          call += "{ const A x[8] = {";
          for (int r = 0; r < 8; ++r) call += "e[" + N(idx(r)) + "]" + (r < 7 ? ", " : "}; ");
          for (int r = 0; r < 8; ++r) {
            call += "{ A acc = cmul(M[" + N(r * 8) + "], x[0]); ";
            for (int c2 = 1; c2 < 8; ++c2) call += "acc = cadd(acc, cmul(M[" + N(r * 8 + c2) + "], x[" + N(c2) + "])); ";
            call += "e[" + N(idx(r)) + "] = (g.cm_lane != 0u) ? tile_sel((tb & g.cm_lane) == g.cm_lane, acc, x[" + N(r) + "]) : acc; } __builtin_amdgcn_sched_barrier(0); ";
          }
          call += "} ";
        }
      } else if (g.kind == 4) {
        call = w.matrix(M, 64) + "pass_dense3w<T, " + N(jof(g.b0)) + ", " + N(jof(g.b1)) + ", " + N(jof(g.tpos_out)) + ">(M, e, c, g.cm_reg, " +
               SegWriter<T>::kLaneArgs + ");";
      }
      w.guarded(g, call);
      if (pin && (g.omask || call.compare(0, 9, "if ((base") == 0)) {
        std::string pl = "     ";
        for (int i = 0; i < 32; ++i) pl += " asm volatile(\"\" : \"+v\"(e[" + N(i) + "].x), \"+v\"(e[" + N(i) + "].y));";
        L(pl);
      }
      w.end_gate();
    }
    L("  }");
  }
  const std::string el = "e" + N(plan.passes.size() - 1);
  if (fold && fold->g) {
    L("  const uint64_t dlane = dst_of(lane_off);");
    for (int u = 0; u < 32; ++u) L("  stg<NT>(out + dst_of(wbase | " + ub(u) + ") + dlane, " + el + "[" + N(u) + "]);");
  } else {
    for (int u = 0; u < 32; ++u) L("  stg<NT>(st + (wbase | " + ub(u) + ") + lane_off, " + el + "[" + N(u) + "]);");
  }
  L("}");
  return w.o;
}

static constexpr int kJitMiss = -1001;  // internal status of a lookup-only pass of the batch code (never crosses the ABI)

// the Ins a tile kernel takes: the tile's high positions, and `extra` ones on top (controls taken off the grid, slice positions),
// opened in the space where p5 and 5 have traded places (tile_block_base; p5 itself is a low position and never in `high`)
static Ins tile_ins(const std::vector<uint32_t>& high, uint32_t p5, const std::vector<uint32_t>& extra = {}, uint64_t ormask = 0) {
  std::vector<uint32_t> v = high;
  v.insert(v.end(), extra.begin(), extra.end());
  for (uint32_t& h : v)
    if (h == 5u) h = p5;
  return make_ins(v, ormask);
}

// How a sweep of either tile shape runs: whether it stores its tiles packed (`fold`, the batch's last step: BatchRun::fold_request
// — the multi-GPU remap's gather rides in this sweep's store phase, TileStorePerm) and whether it runs in parts (`sl`: this step's
// request, BatchRun::slice_first / slice_last).
struct TileSweep {
  bool folding = false;
  TileSlicing* sl = nullptr;  // the accepted request to run in parts; null: one part
  uint32_t nparts() const { return sl ? 1u << sl->nbits : 1u; }
  uint64_t slice_or(uint32_t k) const {  // part k's bits at the slice positions
    uint64_t v = 0;
    for (uint32_t j = 0; sl && j < sl->nbits; ++j) v |= (uint64_t)((k >> j) & 1u) << sl->pos[j];
    return v;
  }
};
// `whole_grid`: the sweep may do either at all (an 11-bit sweep needs the pass kernel and every tile written: no blocks taken off
// the grid).  An accepted slicing opens the slice positions in `ins` too.
static int plan_sweep(qip_hip_state* s, const BatchRun& run, const TileStorePerm* fold, TileSlicing* sl, bool whole_grid, uint32_t tile_bits,
                      const std::vector<uint32_t>& high, uint32_t p5, Ins* ins, TileSweep* f) {
  // a packed store needs rows that stay rows (none of the gathered positions is a lane position of this tile) and the second
  // buffer; otherwise the sweep runs as usual and the remap gathers by itself
  bool folding = fold && fold->g && whole_grid && !s->capture_pool && !run.prepare();
  if (folding)
    for (uint32_t t = 0; t < fold->g; ++t) folding = folding && !tile_is_low(fold->sel[t], p5);
  if (folding) QCHK(ensure_alt(s));
  // r5: the sweep in 2^nbits parts (TileSlicing, qip_internal.h) — the slice positions must be block-index bits of this sweep
  // (not tile positions, not positions taken off the grid), above the rows, and with `need_fold` the store must really be packed
  bool slicing = sl && sl->nbits >= 1 && sl->nbits <= 3 && whole_grid && (!sl->need_fold || folding) && !(sl->in_place_only && folding) &&
                 s->n >= tile_bits + sl->nbits;
  if (slicing)
    for (uint32_t j = 0; j < sl->nbits; ++j) {
      slicing = slicing && sl->pos[j] > 11u && sl->pos[j] < s->n && !tile_is_low(sl->pos[j], p5) && std::find(high.begin(), high.end(), sl->pos[j]) == high.end();
      for (uint32_t i = 0; i < j; ++i) slicing = slicing && sl->pos[i] != sl->pos[j];
    }
  if (slicing) *ins = tile_ins(high, p5, std::vector<uint32_t>(sl->pos, sl->pos + sl->nbits));
  if (sl && !slicing && sl->fallback) QCHK(sl->fallback());
  f->folding = folding;
  f->sl = slicing ? sl : nullptr;
  return QIP_OK;
}
// `launch(k)` for every part of the sweep, then what every sweep ends with: the profile record closes and a packed store makes the
// second buffer current
template <typename F>
static int run_parts(qip_hip_state* s, const BatchRun& run, const TileSweep& f, ProfRec* rec, F&& launch) {
  TileSlicing* sl = f.sl;
  for (uint32_t k = 0; k < f.nparts(); ++k) {
    if (sl && sl->before) QCHK(sl->before(k, f.folding));
    QCHK(launch(k));
    if (sl && sl->after) QCHK(sl->after(k, f.folding));
    if (sl) sl->parts_done += 1;
    if (sl && s->profile) s->prof_launches[KC_TILE_PARTS] += 1;
  }
  if (sl) sl->folded = f.folding;
  if (s->profile) QCHK(prof_end(s, rec));
  if (f.folding) {
    std::swap(s->cur, s->alt);
    std::swap(s->owns_cur, s->owns_alt);
    if (run.fold_done) *run.fold_done = true;
  }
  return QIP_OK;
}
// A segment as its own kernel (either shape): looked up, and compiled on a miss, before the timed region starts; its numbers go to
// the arena (nothing else is uploaded: the descriptors are constants of the code).  Arguments: the state, the tile count or the
// part's slice bits, the parameters (`parametrised`), the packed-store destination.
template <typename T>
static int launch_compiled(qip_hip_state* s, const BatchRun& run, const TileSweep& f, const std::string& src, bool fma, bool parametrised,
                           const std::vector<T>& params, uint64_t ntiles, uint32_t block, size_t lds, double sweep_bytes) {
  const JitJob job = {src, fma};
  QCHK(jit_run(s, job, nullptr, run.jit_collect));
  if (run.prepare()) return QIP_OK;
  if (!params.empty()) QCHK(arena_upload(s, params.data(), params.size() * sizeof(T), 0));
  ProfRec rec;
  rec.cls = KC_TILE_GATES;
  if (s->profile) QCHK(prof_begin(s, KC_TILE_GATES, sweep_bytes, &rec));
  void* st_ptr = s->cur;
  uint64_t second_arg = ntiles;
  void* params_ptr = s->arena;
  void* out_ptr = s->alt;
  // (a kernel without parameters has no third argument: the packed-store destination then comes third)
  void* args_p[] = {&st_ptr, &second_arg, &params_ptr, &out_ptr};
  void* args_np[] = {&st_ptr, &second_arg, &out_ptr};
  void** args = (parametrised || !f.folding) ? args_p : args_np;
  const dim3 grid = grid2d(ntiles >> (f.sl ? f.sl->nbits : 0), 1);
  return run_parts(s, run, f, &rec, [&](uint32_t k) -> int {
    if (f.sl) second_arg = f.slice_or(k);
    return jit_run(s, job, [&](hipFunction_t fn) -> int {
      HIPCHK(hipModuleLaunchKernel(fn, grid.x, grid.y, 1, block, 1, 1, (unsigned)lds, s->stream, args, nullptr));
      return QIP_OK;
    });
  });
}

// The interpreter's lists in the wire format, packed where they are copied to the device (interpreter launches only: plans, their
// exports, compiled segments and k_tile_gates keep TileGate<T> / TileDiagItem<T>).  A run's items may pair up (wire_pack_items), so
// a run entry's first item and item count are rewritten against the packed list.
template <typename T>
static int tile_wire_pack(const std::vector<TileGate<T>>& gates, const std::vector<TileDiagItem<T>>& items, std::vector<TileWireGate<T>>* wg,
                          std::vector<TileWireItem<T>>* wi) {
  const TileWireOps ops = {TOP_DIAG_UNIFORM, TOP_DIAG_LANE, TOP_DIAG_LANE_CTL, TOP_DENSE0, TOP_DIAG_RUN};
  wg->resize(gates.size());
  wi->resize(items.size());
  size_t n = 0;
  for (size_t i = 0; i < gates.size(); ++i) {
    const TileGate<T>& g = gates[i];
    if (!wire_pack_gate<T>(g, ops, &(*wg)[i])) return fail(QIP_ERR_INVALID, "internal: a tile gate field does not fit the wire format");
    if (g.op != TOP_DIAG_RUN) continue;
    if ((size_t)g.nz + g.b1 > items.size()) return fail(QIP_ERR_INVALID, "internal: a diagonal run beyond the item list");
    const long k = wire_pack_items<T>(items.data() + g.nz, g.b1, wi->data() + n);
    if (k < 0) return fail(QIP_ERR_INVALID, "internal: a diagonal item field does not fit the wire format");
    (*wg)[i].nz = (uint32_t)n;
    (*wg)[i].b1 = (uint32_t)k;
    n += (size_t)k;
  }
  wi->resize(n);
  return QIP_OK;
}

template <typename T>
static int launch_tile_segment(qip_hip_state* s, const BatchRun& run, const std::vector<const TileItem*>& seg,
                               std::vector<uint32_t> high_in, const TileStorePerm* fold = nullptr, TileSlicing* sl = nullptr,
                               uint32_t p5_override = 0, const std::vector<uint32_t>* grid_ctl = nullptr, double alg_bytes = 0) {
  // `fold`, `sl`: see TileSweep.
  // `grid_ctl` (one-op sweeps): control positions OUTSIDE the tile that are taken off the grid — only the blocks whose base
  // reads 1 there are launched, so a controlled gate sweeps half / a quarter of the vector like the dedicated kernels do
  // (the kernel's own test of `omask` against the block's base then always passes).  `alg_bytes`: what the profile credits.
  arena_begin_group(s);
  TileSegmentPlan<T> plan;
  // a multi-gate sweep of the interpreter kernel: its uncontrolled X gates go into their neighbours and into the store's flip
  // (tile_absorb_x) before the passes are laid out.  Compiled segments, k_tile_gates and the one-op sweeps take the list as it is
  TileAbsorbedX absorbed;
  if (s->tile_passes && !run.tile_jit && !grid_ctl && !p5_override)
    QCHK(build_tile_segment_absorbed<T>(s->n, seg, std::move(high_in), &plan, run.tile >= 2 ? 2 : 1, &absorbed));
  else
    QCHK(build_tile_segment<T>(s->n, s->tile_passes != 0, seg, std::move(high_in), &plan, run.tile >= 2 ? 2 : 1, p5_override));
  const std::vector<uint32_t>& high = plan.high;
  // r5: the interpreter kernel takes runs of diagonal gates as one loop over TileDiagItem steps (tile_merge_diag_runs: the same
  // products in the same order, without the per-gate decoding); the plan itself stays what the generators and the CPU replay read
  TileInterpPlan<T> interp;
  // (a kind-5 gate has no other form in the interpreter: with the option off, the runs that hold one are still made)
  if (!s->tile_passes && !plan.diags.empty()) return fail(QIP_ERR_INVALID, "internal: a multi-qubit diagonal item in a k_tile_gates segment");
  const bool use_runs = (g_tile_diag_runs || !plan.diags.empty()) && s->tile_passes && !run.tile_jit;
  if (use_runs) tile_merge_diag_runs<T>(plan, &interp, g_tile_diag_runs ? 2u : ~0u);
  const bool has_runs = use_runs && interp.runs > 0;
  std::vector<TileGate<T>>& gates = has_runs ? interp.gates : plan.gates;
  std::vector<amp_t<T>>& mats = plan.mats;
  TilePassDesc& pd = has_runs ? interp.pd : plan.pd;
  // the interpreter kernel reads its lists in the wire format (qip_tile_wire.h: one 64-byte block per entry and per run item);
  // k_tile_gates reads the gate list as it is.  Arena and pool regions start 256-byte aligned, the items at a multiple of 64.
  const bool wire = s->tile_passes && !run.tile_jit;
  std::vector<TileWireGate<T>> wgates;
  std::vector<TileWireItem<T>> witems;
  if (wire) QCHK(tile_wire_pack<T>(gates, interp.items, &wgates, &witems));
  const size_t gates_bytes = wire ? wgates.size() * sizeof(TileWireGate<T>) : gates.size() * sizeof(TileGate<T>);
  const size_t mats_bytes = mats.size() * sizeof(amp_t<T>);
  const size_t items_bytes = has_runs ? witems.size() * sizeof(TileWireItem<T>) : 0;
  static_assert(sizeof(TileGate<T>) % 16 == 0 && sizeof(TileWireGate<T>) % 64 == 0, "the matrix block behind the gate list stays 16-byte aligned");
  static_assert(sizeof(amp_t<T>) * 16 % 16 == 0 && sizeof(TileWireItem<T>) == 64, "... and the diagonal steps behind the matrices, on a block boundary");
  const size_t items_off = (gates_bytes + mats_bytes + 63) / 64 * 64;
  auto upload_gates = [&]() -> int {
    QCHK(ensure_arena(s, items_off + items_bytes));  // one allocation: growing frees the old arena
    QCHK(arena_upload(s, wire ? (const void*)wgates.data() : (const void*)gates.data(), gates_bytes, 0));
    if (!mats.empty()) QCHK(arena_upload(s, mats.data(), mats_bytes, gates_bytes));
    if (items_bytes) QCHK(arena_upload(s, witems.data(), items_bytes, items_off));
    return QIP_OK;
  };
  TileDesc d;
  memset(&d, 0, sizeof d);
  d.ngates = (uint32_t)gates.size();
  for (int j = 0; j < kTileHigh; ++j) d.hpos[j] = high[j];
  d.p5 = plan.p5;
  Ins ins = tile_ins(high, plan.p5);  // (sorts its own copy; `high` keeps the tile-bit order)
  uint64_t ntiles = 1ull << (s->n - kTileBits);
  const bool whole_grid = !grid_ctl || grid_ctl->empty();
  if (!whole_grid) {
    uint64_t ones = 0;
    for (uint32_t c : *grid_ctl) ones |= 1ull << (c == 5u ? plan.p5 : c);
    ins = tile_ins(high, plan.p5, *grid_ctl, ones);
    ntiles >>= grid_ctl->size();
  }
  const double sweep_bytes = alg_bytes > 0 ? alg_bytes : 2.0 * (double)s->amp_bytes * (double)s->namps;
  TileSweep f;
  QCHK(plan_sweep(s, run, fold, sl, s->tile_passes && whole_grid, kTileBits, high, plan.p5, &ins, &f));
  const size_t lds = sizeof(amp_t<T>) << kTileBits;
  if (s->tile_passes && run.tile_jit) {
    const bool fma = s->tile_fma && run.tile >= 2;  // tile = 1 promises IEEE equality with the gate-by-gate path: never fused
    // structure compiled, numbers in the arena (see tile_jit_source): the default form.  tile_jit = 3 (tuning aid) writes the
    // numbers into the source as literals instead: every constant then occupies vector registers (gfx950's VOP3 takes no
    // 64-bit literal), which makes the configs[1] segments spill under the five-blocks-per-CU register bound (104 vs 90 ms),
    // and every new angle is a new kernel; its one merit is ~3 % fewer multiplies in QFT where equal constants fold
    const bool parametrised = run.tile_jit != 3;
    std::vector<T> params;
    const bool merge = s->tile_merge && run.tile >= 2;  // products of runs of diagonal gates: rounding differs (1e-12 mode only)
    int remap = ntiles % 64 == 0 ? (int)g_tile_remap : 0;
    if (remap == 4) {  // XCD-aware: tile-number bit J is the first free position at or above 16 (see tile_jit_source)
      uint32_t nb = 0, J = 0;
      while ((1ull << nb) < ntiles) ++nb;
      uint32_t seen = 0;
      for (uint32_t pp = kTileLow; pp < s->n && seen < nb; ++pp) {
        bool opened = false;
        for (uint32_t j = 0; j < ins.npos; ++j) opened = opened || ins.pos[j] == pp;
        if (opened) continue;
        if (pp < 16) ++J;
        ++seen;
      }
      if (nb < 3) remap = 0;
      else remap = 16 + (int)std::min(J, nb - 3);
    }
    if (f.sl) remap = 0;
    const std::string src = tile_jit_source<T>(plan, ins, use_nt(s), remap, parametrised ? &params : nullptr, merge, f.folding ? fold : nullptr, f.sl != nullptr);
    return launch_compiled<T>(s, run, f, src, fma, parametrised, params, ntiles, kTileBlock, lds, sweep_bytes);
  }
  if (run.prepare()) return QIP_OK;
  QCHK(upload_gates());  // descriptors up, then the timed region starts
  const TileGate<T>* dg = (const TileGate<T>*)s->arena;  // device addresses: valid only after the upload (the arena may grow / move)
  const amp_t<T>* dmats = (const amp_t<T>*)((const char*)s->arena + gates_bytes);
  const TileWireGate<T>* wg = (const TileWireGate<T>*)s->arena;
  const TileWireItem<T>* ditems = (const TileWireItem<T>*)((const char*)s->arena + items_off);
  ProfRec rec;
  rec.cls = KC_TILE_GATES;
  if (s->profile) QCHK(prof_begin(s, KC_TILE_GATES, sweep_bytes, &rec));
  if (s->tile_passes) {
    const uint64_t ntiles_part = ntiles >> (f.sl ? f.sl->nbits : 0);
    return run_parts(s, run, f, &rec, [&](uint32_t k) -> int {
      Ins ins_k = ins;
      ins_k.ormask |= f.slice_or(k);
      launch_tile_passes<T>(s->stream, grid2d(ntiles_part, 1), lds, use_nt(s), (amp_t<T>*)s->cur, ins_k, pd, wg, dmats, (amp_t<T>*)s->alt,
                            f.folding ? fold : nullptr, ditems);
      HIPCHK(hipGetLastError());
      return QIP_OK;
    });
  }
  if (use_nt(s))
    hipLaunchKernelGGL((k_tile_gates<T, true>), grid2d(ntiles, 1), dim3(kBlock), lds, s->stream, (amp_t<T>*)s->cur, ins, d, dg);
  else
    hipLaunchKernelGGL((k_tile_gates<T, false>), grid2d(ntiles, 1), dim3(kBlock), lds, s->stream, (amp_t<T>*)s->cur, ins, d, dg);
  HIPCHK(hipGetLastError());
  if (s->profile) QCHK(prof_end(s, &rec));
  return QIP_OK;
}

// a multi-gate step of a wide plan (option "tile_wide"): always its own run-time-compiled kernel
template <typename T>
static int launch_wide_segment(qip_hip_state* s, const BatchRun& run, const std::vector<const TileItem*>& seg, std::vector<uint32_t> high_in,
                               const TileStorePerm* fold = nullptr, TileSlicing* sl = nullptr) {
  arena_begin_group(s);
  WidePlan<T> plan;
  QCHK(build_wide_segment<T>(s->n, seg, std::move(high_in), &plan, run.tile >= 2 ? 2 : 1));
  Ins ins = tile_ins(plan.high, plan.p5);
  TileSweep f;
  QCHK(plan_sweep(s, run, fold, sl, true, kWideBits, plan.high, plan.p5, &ins, &f));
  const bool parametrised = run.tile_jit != 3;
  std::vector<T> params;
  const bool merge = s->tile_merge && run.tile >= 2;  // products of runs of diagonal gates: rounding differs (1e-12 mode only)
  const std::string src = wide_jit_source<T>(plan, ins, use_nt(s), parametrised ? &params : nullptr, merge, g_tile_wide_pin != 0, g_tile_wide_dense3_inline != 0,
                                             f.sl != nullptr, f.folding ? fold : nullptr);
  if (src.empty()) return fail(QIP_ERR_INVALID, "internal: wide segment source");
  const size_t lds = 2 * (sizeof(amp_t<T>) << kTileBits);  // the transposition buffer: two quarters of the tile
  return launch_compiled<T>(s, run, f, src, s->tile_fma && run.tile >= 2, parametrised, params, 1ull << (s->n - (uint32_t)kWideBits), 256, lds,
                            2.0 * (double)s->amp_bytes * (double)s->namps);
}

template <typename T>
int tile_apply_single(qip_hip_state* s, const BatchRun& run, const qip_op* op, const TileStorePerm* fold, bool* done, double alg_bytes) {
  *done = false;
  if (s->n < (uint32_t)kTileBits || !s->tile_passes) return QIP_OK;
  TileItem it;
  QCHK(classify_tile_item(s->dtype, s->n, op, &it));
  std::vector<TileItem> parts;
  if (it.tileable) {
    parts.push_back(it);
  } else if (it.swap_pairs.size() >= 2) {
    // an uncontrolled Swap(h >= 2) is h disjoint transpositions: h bit-swap items of ONE sweep (pure moves: any grouping is
    // bit-identical to the single permutation)
    for (const auto& pr : it.swap_pairs) {
      TileItem t;
      t.tileable = t.exact = true;
      t.kind = 2;
      t.t0 = std::min(pr.first, pr.second);
      t.t1 = std::max(pr.first, pr.second);
      t.pos = {t.t0, t.t1};
      t.nd_mask = (1ull << t.t0) | (1ull << t.t1);
      parts.push_back(t);
    }
  } else {
    return QIP_OK;
  }
  // Which rows for this ONE op (qip_kernels.h tile_block_base)?  With at most three positions forced above contiguous rows the
  // two free ones become 11 and 12 — the fastest tile shape measured (5.3 ms per sweep at n = 30) — so contiguous rows stay;
  // with more, the forced positions scatter the tile over the DRAM row bits and the split rows win (k = 4 on four high
  // positions: 72.9 -> 75.5 %, profiles/r04_tile_rows.md).
  // Only the positions the op EXCHANGES amplitudes across must be tile bits; its controls may sit anywhere: inside the rows they
  // are lane predicates, above them they come off the grid (r4: controlled dense k = 2, 3 take this route too).
  auto exchanged = [](const TileItem& t) {
    std::vector<uint32_t> e;
    for (uint32_t p : t.pos)
      if ((t.nd_mask >> p) & 1ull) e.push_back(p);
    return e;
  };
  uint32_t p5 = tile_p5(s->dtype, s->n);
  if (p5 != 5u) {
    std::vector<uint32_t> forced;
    for (const TileItem& t : parts)
      for (uint32_t p : exchanged(t))
        if (p >= (uint32_t)kTileLow && std::find(forced.begin(), forced.end(), p) == forced.end()) forced.push_back(p);
    if (forced.size() <= 3) p5 = 5u;
  }
  std::vector<uint32_t> hp;
  for (const TileItem& t : parts)
    for (uint32_t p : exchanged(t))
      if (!tile_is_low(p, p5) && std::find(hp.begin(), hp.end(), p) == hp.end()) hp.push_back(p);
  if (hp.size() > (size_t)kTileHigh) return QIP_OK;
  std::vector<uint32_t> grid_ctl;  // (a single item: `parts` holds several only for an uncontrolled Swap)
  if (parts.size() == 1)
    for (uint32_t c : parts[0].cpos)
      if (!tile_is_low(c, p5)) grid_ctl.push_back(c);
  if (s->n < (uint32_t)kTileBits + (uint32_t)grid_ctl.size()) return QIP_OK;
  std::vector<const TileItem*> seg;
  for (const TileItem& t : parts) seg.push_back(&t);
  // the free positions that pad the tile must not be control positions that left the grid
  if (!grid_ctl.empty()) {
    const uint32_t pad_from = std::min<uint32_t>((uint32_t)g_tile_pad_from, s->n > (uint32_t)kTileBits ? s->n - 5 : (uint32_t)kTileLow);
    for (int round = 0; round < 2; ++round)
      for (uint32_t p = round == 0 ? std::max<uint32_t>(pad_from, kTileLow) : 5u; hp.size() < (size_t)kTileHigh && p < s->n; ++p)
        if (!tile_is_low(p, p5) && std::find(hp.begin(), hp.end(), p) == hp.end() && std::find(grid_ctl.begin(), grid_ctl.end(), p) == grid_ctl.end())
          hp.push_back(p);
    if (hp.size() != (size_t)kTileHigh) return QIP_OK;
  }
  BatchRun interp = run;
  interp.tile_jit = 0;  // one op does not repay a run-time compilation: the interpreter kernel
  QCHK(launch_tile_segment<T>(s, interp, seg, hp, fold, nullptr, p5, &grid_ctl, alg_bytes));
  *done = true;
  return QIP_OK;
}
template int tile_apply_single<double>(qip_hip_state*, const BatchRun&, const qip_op*, const TileStorePerm*, bool*, double);
template int tile_apply_single<float>(qip_hip_state*, const BatchRun&, const qip_op*, const TileStorePerm*, bool*, double);

template <typename T>
static int debug_jit_t(int dtype, uint32_t n, const qip_op* ops, uint64_t count, int mode, uint64_t* nseg, uint64_t* src_bytes,
                       uint64_t* code_bytes, std::string* first) {
  TileSchedule sc;
  QCHK(make_tile_schedule(dtype, n, ops, count, mode, true, &sc));
  const std::vector<TileItem>& items = sc.items;
  *nseg = *src_bytes = *code_bytes = 0;
  std::vector<JitJob> jobs;
  for (const TileStep& st : sc.steps) {
    if (st.ops.size() < 2 || !st.perm.empty()) continue;
    std::vector<const TileItem*> seg;
    for (uint64_t i : st.ops) seg.push_back(&items[i]);
    std::vector<T> params;  // mode bit 6: parametrised (numbers as kernel data)
    std::string src;
    // mode bit 11 (2048): the SLICED + PACKED-STORE variant the sharded state's overlapped exchange launches (r5) — one position that is
    // not a tile position is gathered on top, another cuts the sweep in two parts: generated and compiled here, run on the GPU by
    // tests/dist_worker_gpu.py
    auto variant = [&](const std::vector<uint32_t>& high, uint32_t p5, Ins* ins, TileStorePerm* sp) {
      std::vector<uint32_t> spare;
      for (uint32_t pp = n; pp-- > 12u && spare.size() < 2;)
        if (!tile_is_low(pp, p5) && std::find(high.begin(), high.end(), pp) == high.end()) spare.push_back(pp);
      if (spare.size() < 2) return false;
      memset(sp, 0, sizeof *sp);
      sp->g = 1;
      sp->Lg = n - 1;
      sp->sel[0] = sp->sel_desc[0] = spare[0];
      *ins = tile_ins(high, p5, {spare[1]});
      return true;
    };
    if ((mode & 16) && n > (uint32_t)kWideBits) {  // mode bit 4: wide tiles
      WidePlan<T> wplan;
      QCHK(build_wide_segment<T>(n, seg, st.high, &wplan, mode & 3));
      Ins ins = tile_ins(wplan.high, wplan.p5);
      TileStorePerm sp;
      const bool var = (mode & 2048) && variant(wplan.high, wplan.p5, &ins, &sp);
      src = wide_jit_source<T>(wplan, ins, true, (mode & 64) ? &params : nullptr, (mode & 128) != 0, (mode & 256) != 0, (mode & 512) != 0, var, var ? &sp : nullptr);
      if (src.empty()) return fail(QIP_ERR_INVALID, "internal: wide segment source");
    } else {
      TileSegmentPlan<T> plan;
      QCHK(build_tile_segment<T>(n, true, seg, st.high, &plan, mode & 3));
      Ins ins = tile_ins(plan.high, plan.p5);
      TileStorePerm sp;
      const bool var = (mode & 2048) && variant(plan.high, plan.p5, &ins, &sp);
      src = tile_jit_source<T>(plan, ins, true, 0, (mode & 64) ? &params : nullptr, (mode & 128) != 0, var ? &sp : nullptr, var);  // bit 7: merged diagonal runs
    }
    if (*nseg == 0 && first) *first = src;
    *nseg += 1;
    *src_bytes += src.size();
    jobs.push_back({src, (mode & 32) != 0});  // mode bit 5: fused multiply-adds
  }
  std::vector<std::vector<char>> code;  // as apply_ops obtains them: disk cache, helper processes, this process
  QCHK(jit_obtain_code(jobs, &code));
  for (const auto& c : code) *code_bytes += c.size();
  return QIP_OK;
}

extern "C" int qip_hip_debug_tile_jit(int dtype, uint32_t n, const qip_op* ops, uint64_t count, int mode, uint64_t* segments,
                                      uint64_t* source_bytes, uint64_t* code_bytes, const char** first_source) try {
  static thread_local std::string first;
  if ((count && !ops) || !segments || !source_bytes || !code_bytes) return fail(QIP_ERR_INVALID, "null argument");
  if (dtype != QIP_C64 && dtype != QIP_C32) return fail(QIP_ERR_INVALID, "bad dtype %d", dtype);
  if (n < (uint32_t)kTileBits) return fail(QIP_ERR_UNSUPPORTED, "tile sweeps need n >= %d", kTileBits);
  first.clear();
  QCHK(dtype == QIP_C64 ? debug_jit_t<double>(dtype, n, ops, count, mode, segments, source_bytes, code_bytes, &first)
                        : debug_jit_t<float>(dtype, n, ops, count, mode, segments, source_bytes, code_bytes, &first));
  if (first_source) *first_source = first.c_str();
  return QIP_OK;
} QIP_CATCH_ALL

extern "C" int qip_hip_tile_bits(void) { return kTileBits; }

// option "tile_auto": from this size a program compiles its segments (below it a sweep is launch-bound and the interpreter, replayed
// as a graph, is as fast: profiles/r01_small_n_launch_bound.md)
int64_t g_debug_slice_sweeps = 0;  // global option "debug_slice_sweeps" (measuring aid, see apply_ops_tiled)
constexpr int kAutoJitMinQubits = 22;
// ... and from this size a one-shot apply_ops looks its wide plan up (r6).  The lookup plans twice and fingerprints every segment:
// ~3.5 us of host time per gate, which at n = 22 makes the compiled path host-bound and SLOWER than the interpreter (2000 gates:
// 7.4 against 6.2 ms); from n = 24 it wins (10.0 against 15.4 ms; n = 26: 36 against 57 ms).
constexpr int kAutoOneShotMinQubits = 24;
constexpr int kPairFloorMinQubits = 22;  // option "pair_floor": only where a sweep is HBM-bound (below, launches are)
static bool tile_wide_of(const qip_hip_state* s, const BatchRun& run) {  // wide tiles: run-time-compiled segments only, a state above one wide tile
  // (r5: also inside a graph capture — the launch and its parameter upload are ordinary stream work like the 11-bit segments')
  return run.tile_wide && run.tile_jit && s->tile_passes && s->n > (uint32_t)kWideBits;
}
static int tile_mode_of(const qip_hip_state* s, const BatchRun& run) {  // option tile_relabel: 1 = when it shortens the plan, 2 = always
  return (int)std::min<int64_t>(run.tile, 2) | (run.tile_relabel ? 4 : 0) | (run.tile_relabel == 2 ? 8 : 0) |  // (3 = persistent layout)
         (tile_wide_of(s, run) ? 16 : 0);
}

// (qip_dist.hip schedules the edge sweeps of a remap with it: what a plain batch on the shard plans with)
int state_tile_mode(const qip_hip_state* s) { return tile_mode_of(s, BatchRun(*s)); }

template <typename T>
static int apply_ops_tiled(qip_hip_state* s, const qip_op* ops_in, uint64_t count, const BatchRun& run) {
  TileSchedule sc;
  // tile_relabel = 3: the qubit layout persists across calls — the plan starts from the layout the previous call left and
  // does not close with the restoring sweep (that happens once, when somebody needs the caller's order: state_settle).
  // Not inside a graph capture or a compile-only pass: a recorded program must start and end in the caller's order.
  const bool persist = run.tile_relabel >= 3 && !s->capture_pool && !run.prepare();
  if (!persist && !s->layout.empty()) QCHK(state_settle(s));
  sc.init_phys = s->layout;
  sc.keep_layout = persist;
  QCHK(make_tile_schedule(s->dtype, s->n, ops_in, count, tile_mode_of(s, run), s->tile_passes != 0, &sc));
  {
    // a bit-permutation sweep is out of place: get the second buffer BEFORE the first gate runs; if HBM cannot hold it
    // (a state above half of the 288 GB), fall back to the plan without permutation sweeps instead of failing half way
    bool permutes = false;
    for (const TileStep& st : sc.steps) permutes = permutes || !st.perm.empty();
    // ... and a plan that LEAVES the state relabelled (tile_relabel = 3) commits the first reader to a settling sweep, which
    // needs that buffer too: a state too large for it would become unreadable — same fallback
    bool leaves_relabelled = false;
    if (persist)
      for (uint32_t p = 0; p < sc.final_phys.size(); ++p) leaves_relabelled = leaves_relabelled || sc.final_phys[p] != p;
    if ((permutes || leaves_relabelled) && !run.prepare() && !s->alt && ensure_alt(s) != QIP_OK) {
      (void)hipGetLastError();
      if (!s->layout.empty()) return fail(QIP_ERR_DEVICE, "no room for the second buffer a relabelled state needs");
      sc = TileSchedule();
      // (without relabelling: such a plan neither permutes nor leaves a layout behind)
      QCHK(make_tile_schedule(s->dtype, s->n, ops_in, count, tile_mode_of(s, run) & (3 | 16), s->tile_passes != 0, &sc, /*allow_permute=*/false));
    }
  }
  const qip_op* ops = sc.circuit;
  const std::vector<TileItem>& items = sc.items;
  // from here on the shard is somewhere between two layouts until the last step has been issued: single ops inside the plan
  // are already expressed in physical positions, so they must not settle (layout is cleared for the duration)
  const std::vector<uint32_t> final_phys = sc.final_phys;
  // a relabelled plan moves the qubits between its steps: if a step fails (a launch, the arena, the run-time compiler) the
  // buffer is in an order no caller can name — the handle is poisoned until it is re-initialised (the sharded
  // handle does the same).  A plain plan that fails leaves a prefix of the circuit applied in the caller's order, like the
  // gate-by-gate path: reported, not poisoned.
  bool moves_qubits = !sc.init_phys.empty() || sc.inserted > 0 || sc.absorbed > 0;
  for (const TileStep& st : sc.steps) moves_qubits = moves_qubits || !st.perm.empty();
  const bool wide = (tile_mode_of(s, run) & 16) != 0;
  // (the pre-compilation runs BEFORE the layout is cleared — a compiler failure here returns with the handle
  // exactly as it was, still naming the layout the data is in)
  // r5: every segment of the plan that is not resident yet is found FIRST (a compile-only pass that collects the sources), looked
  // up in the disk cache, and the rest compiled side by side in helper processes (jit_prepare) before anything runs.
  // A plan that has been through this once is remembered by a fingerprint of its structure (jit_plan_query), so the steady state
  // (the same circuit applied again and again) does not generate every source twice.
  if (run.tile_jit && s->tile_passes && !s->capture_pool) {
    uint64_t fp = 1469598103934665603ull;
    auto mix = [&](uint64_t v) {
      fp ^= v;
      fp *= 1099511628211ull;
    };
    mix(s->n); mix((uint64_t)s->dtype); mix((uint64_t)s->device); mix((uint64_t)tile_mode_of(s, run)); mix((uint64_t)run.tile_jit);
    mix((uint64_t)(s->tile_fma != 0) | (uint64_t)(s->tile_merge != 0) << 1 | (uint64_t)(g_tile_wide_pin != 0) << 2 |
        (uint64_t)(g_tile_wide_dense3_inline != 0) << 3 | (uint64_t)use_nt(s) << 4 | (uint64_t)g_tile_remap << 8);
    for (const TileStep& st : sc.steps) {
      if (st.ops.size() < 2 || !st.perm.empty()) continue;
      mix(0xABCDu + st.ops.size());
      for (uint32_t h : st.high) mix(h);
      for (uint64_t i : st.ops) {
        const TileItem& it = items[i];
        mix((uint64_t)it.kind | (uint64_t)it.nz << 8 | (uint64_t)it.exact << 40);
        mix(it.nd_mask);
        mix(it.d_mask);
        for (uint32_t c : it.cpos) mix(0x100u + c);
        mix(it.t0 | (uint64_t)it.t1 << 8 | (uint64_t)it.t2 << 16);
        // its width and which entries are the unit.  Like the other kinds' part of the fingerprint this is not everything a source
        // depends on (a component that becomes exactly 0 / +-1 turns from kernel data into a literal): a plan remembered as warm only
        // skips the pre-compilation pass, a segment that is not resident is still compiled when it is launched
        if (it.kind == kTileKindDiagK) {
          uint64_t units = 0;
          for (uint32_t e = 0; e < (1u << it.dk); ++e) units |= (uint64_t)(it.mat[2 * e] == 1.0 && it.mat[2 * e + 1] == 0.0) << e;
          mix(0x5D000000ull | (uint64_t)it.dk << 16 | units);
        }
      }
    }
    const JitPlanMemo memo = jit_plan_query(fp);
    // a plan seen incomplete a moment ago: its segments are still being compiled, do not look again yet
    if (memo == JitPlanMemo::kColdRecently && run.jit == BatchRun::kLookupOnly) return kJitMiss;
    if (memo != JitPlanMemo::kWarm) {
      std::vector<JitJob> jobs;
      BatchRun collect = run;
      collect.jit = BatchRun::kPrepare;
      collect.jit_collect = &jobs;
      for (const TileStep& st : sc.steps) {
        if (st.ops.size() < 2 || !st.perm.empty()) continue;
        std::vector<const TileItem*> seg;
        for (uint64_t i : st.ops) seg.push_back(&items[i]);
        QCHK(wide ? launch_wide_segment<T>(s, collect, seg, st.high) : launch_tile_segment<T>(s, collect, seg, st.high));
      }
      if (run.jit == BatchRun::kLookupOnly) {
        std::vector<JitJob> misses;
        QCHK(jit_lookup(s, jobs, &misses));
        if (!misses.empty()) {
          jit_compile_in_background(misses);
          jit_plan_mark_cold(fp);
          return kJitMiss;  // (nothing has run, the layout is untouched)
        }
      } else {
        QCHK(jit_prepare(s, jobs));
      }
      jit_plan_mark_warm(fp);
    }
  }
  s->layout.clear();
  // The multi-GPU gather may ride in the last sweep's store phase only when that sweep addresses the CALLER's bit order: the
  // request names caller-order positions (TileStorePerm.sel).  A plan that leaves the qubits relabelled (tile_relabel = 3 with
  // a non-identity final layout) ends in physical positions that mean other qubits: no fold, the layout is settled and the
  // gather runs as a sweep of its own (qip_dist.hip dist_run_steps).
  bool ends_in_callers_order = true;
  for (uint32_t p = 0; p < final_phys.size(); ++p) ends_in_callers_order = ends_in_callers_order && final_phys[p] == p;
  auto run_steps = [&]() -> int {
    size_t step_no = 0;
    // a first-step request that no step can take (an empty plan; one step that already serves the last-step request) is settled
    // BEFORE anything is enqueued: its fallback is what makes the data the batch reads complete
    TileSlicing* first = run.slice_first;
    if (first && !run.prepare() && !s->capture_pool && (sc.steps.empty() || (sc.steps.size() == 1 && run.slice_last && ends_in_callers_order))) {
      if (first->fallback) QCHK(first->fallback());
      first = nullptr;
    }
    for (const TileStep& st : sc.steps) {
      ++step_no;
      // (the batch's last step may store packed)
      const TileStorePerm* fold = ends_in_callers_order && step_no == sc.steps.size() ? run.fold_request : nullptr;
      // r5: the first / last step in parts (the sharded state's overlapped exchange); positions are caller-order positions, so
      // only a plan that starts / ends in the caller's order may take the request.  A step that is not a multi-gate tile sweep
      // (or a sweep that cannot be cut there) consumes it through its fallback.
      TileSlicing* want = nullptr;
      if (!run.prepare() && !s->capture_pool) {
        if (step_no == sc.steps.size() && run.slice_last && ends_in_callers_order) want = run.slice_last;
        else if (step_no == 1 && first && sc.init_phys.empty() && sc.inserted == 0 && sc.absorbed == 0) want = first;
        else if (step_no == 1 && first && first->fallback) QCHK(first->fallback());  // (a relabelled plan addresses other positions: settled unsliced)
      }
      TileSlicing dbg;
      if (!want && g_debug_slice_sweeps >= 2 && !run.prepare() && !s->capture_pool && st.perm.empty() && st.ops.size() >= 2) {
        // measuring aid (global option "debug_slice_sweeps" = 2 / 4 / 8): EVERY multi-gate sweep in that many parts, cut at the highest
        // index positions its tile leaves alone — what a sliced launch costs by itself, at full size on one GPU, without any exchange
        uint32_t pb = 0;
        while ((1 << pb) < g_debug_slice_sweeps) ++pb;
        dbg.nbits = 0;
        for (uint32_t pp = s->n; pp-- > 12u && dbg.nbits < pb;)
          if (std::find(st.high.begin(), st.high.end(), pp) == st.high.end()) dbg.pos[dbg.nbits++] = pp;
        if (dbg.nbits == pb) want = &dbg;
      }
      if (!st.perm.empty() || st.ops.size() == 1) {  // not a tile sweep: a request to run in parts is settled unsliced
        if (want && want->fallback) QCHK(want->fallback());
        if (st.perm.empty()) QCHK(apply_op_t<T>(s, &ops[st.ops[0]], run, fold));
        else if (!run.prepare()) QCHK(launch_permute(s, st.perm.data()));  // a run of Swap ops as one bit-permutation sweep
        continue;
      }
      std::vector<const TileItem*> seg;
      for (uint64_t i : st.ops) seg.push_back(&items[i]);
      if (wide) QCHK(launch_wide_segment<T>(s, run, seg, st.high, fold, want));
      else QCHK(launch_tile_segment<T>(s, run, seg, st.high, fold, want));
    }
    return QIP_OK;
  };
  const int rc_steps = run_steps();
  if (rc_steps != QIP_OK) {
    if (moves_qubits && !run.prepare()) {
      s->poisoned = true;
      s->poison_msg = g_last_error;
    }
    return rc_steps;
  }
  if (persist) {
    bool identity = true;
    for (uint32_t p = 0; p < final_phys.size(); ++p) identity = identity && final_phys[p] == p;
    if (!identity) s->layout = final_phys;
  }
  return QIP_OK;
}

// Option "pair_floor"'s byte rule: what one gate launched by itself moves, in sweeps of the whole vector — its algorithmic share,
// doubled for every selector (control, target of a phase-type diagonal) inside a 1-KiB wave row (whole lines / rows travel
// whichever half is needed: profiles/r02_line_bits.md), at most 1.  false: the op is not a tile item.  `floor_gate`: the doubling
// applied (the gate moves more than its algorithmic bytes).
static bool floor_share(const qip_hip_state* s, const qip_op* op, const TileItem& it, double* share, bool* floor_gate) {
  double by = 0;
  if (!it.tileable || qip_hip_op_algorithmic_bytes(s->dtype, s->n, op, &by) != QIP_OK) return false;
  const double full = 2.0 * (double)s->amp_bytes * (double)s->namps;
  const int in_row = __builtin_popcountll(it.d_mask & 63ull);
  *share = std::min(1.0, by / full * (double)(1u << in_row));
  *floor_gate = in_row && *share > by / full;
  return true;
}
// A multi-gate interpreter sweep moves one sweep and runs a little slower than a bare one: it pays from 1.3 sweeps of single
// launches (T on a low bit + H = 1 + 1; NOT two controlled phases of a QFT, 1/4 doubled = 1/2 each: 946 -> 986 ms when paired).
constexpr double kFloorFuseSweeps = 1.3;

// Option "pair_floor" on the default path (tile = 0): the WHOLE batch planned once as tile sweeps in circuit order (mode 1:
// exact commutations only, no relabelling, no permutation sweeps — the state never leaves the caller's order) and every step of
// >= 2 gates that the byte rule accepts launched as ONE interpreter sweep; every other step gate by gate through the gate's own
// kernel.  An op that launched by itself runs on matrix cores (single_route) was planned as a step of its own that no gate passes.
// The same unfused arithmetic per amplitude as one launch per gate: IEEE-equal (only the sign of a zero may differ).
// Interpreter only: nothing is compiled at run time.  A failure leaves a prefix of the (commutation-equivalent) circuit applied
// in the caller's order, as gate by gate does, and names the caller's op indices (the plan's circuit IS the caller's array).
template <typename T>
static int apply_ops_floor_plan(qip_hip_state* s, const TileSchedule& sc, const BatchRun& run) {
  BatchRun interp = run;
  interp.tile_jit = 0;  // (launch_tile_segment: the interpreter, whatever the tile options of other paths say)
  int rc = QIP_OK;
  std::string where;
  for (const TileStep& st : sc.steps) {
    bool fuse = st.ops.size() >= 2 && st.perm.empty();
    double moved = 0;
    for (size_t j = 0; fuse && j < st.ops.size(); ++j) {
      double share = 0;
      bool floor_gate = false;
      fuse = floor_share(s, &sc.circuit[st.ops[j]], sc.items[st.ops[j]], &share, &floor_gate);
      moved += share;
    }
    if (fuse && moved >= kFloorFuseSweeps) {
      std::vector<const TileItem*> seg;
      for (uint64_t i : st.ops) seg.push_back(&sc.items[i]);
      rc = launch_tile_segment<T>(s, interp, seg, st.high);  // (the profile credits ONE sweep's bytes)
      if (rc != QIP_OK) {
        for (uint64_t i : st.ops) where += (where.empty() ? "ops " : ", ") + std::to_string(i);
        break;
      }
      continue;
    }
    for (uint64_t i : st.ops) {
      rc = apply_op_t<T>(s, &sc.circuit[i], interp);
      if (rc != QIP_OK) {
        where = "op " + std::to_string(i);
        break;
      }
    }
    if (rc != QIP_OK) break;
  }
  if (rc != QIP_OK) {
    std::string msg = g_last_error;
    return fail(rc, "%s: %s", where.c_str(), msg.c_str());
  }
  return QIP_OK;
}

int apply_ops_run(qip_hip_state* s, const qip_op* ops, uint64_t count, const BatchRun& run) try {
  STATE_ENTER_RAW(s);  // (a relabelled state stays relabelled for a relabelling batch: apply_ops_tiled decides)
  if (count && !ops) return fail(QIP_ERR_INVALID, "null op array");
  auto tiled = [s](const qip_op* o, uint64_t c, const BatchRun& r) {
    return s->dtype == QIP_C64 ? apply_ops_tiled<double>(s, o, c, r) : apply_ops_tiled<float>(s, o, c, r);
  };
  if (run.tile >= 1 && !s->force_generic && !g_force_generic && s->n >= (uint32_t)kTileBits) {
    // r6, option "tile_auto" for one-shot callers: the compiled (wide) sweeps when every segment of the plan is already resident
    // or in the disk cache; otherwise the interpreter now, the misses compiled in the background for the next call.  Not for the
    // batches of a sharded state that carry a fold / slice request (their last sweep is chosen by the exchange), not while a
    // program records or pre-compiles (it compiles for itself).
    if (s->tile_auto && !run.tile_jit && s->tile_passes && s->n >= (uint32_t)kAutoOneShotMinQubits && count >= 2 && !s->capture_pool && !run.prepare() &&
        !run.fold_request && !run.slice_first && !run.slice_last && !s->profile && g_jit_disk) {
      BatchRun lookup = run;
      lookup.tile_jit = 1;
      lookup.tile_wide = s->n > (uint32_t)kWideBits ? 1 : 0;
      lookup.jit = BatchRun::kLookupOnly;
      const int rc = tiled(ops, count, lookup);
      if (rc != kJitMiss) return rc;
    }
    return tiled(ops, count, run);
  }
  // The batch plan of option pair_floor owns the batch only where nothing else decides its launches: not for a sharded state's
  // batch that carries a fold / slice request (its last sweep is chosen by the exchange), not while a program records or
  // pre-compiles, not on a state that arrives relabelled, not under force_generic or fuse
  const bool floor_plan = s->pair_floor && count >= 2 && s->n >= (uint32_t)kPairFloorMinQubits && s->tile_passes && !s->capture_pool &&
                          !run.prepare() && !s->force_generic && !g_force_generic && s->fuse < 2 && s->layout.empty() &&
                          !run.fold_request && !run.slice_first && !run.slice_last;
  // (only tile sweeps run in parts: every other path settles the request before its first launch)
  if (run.slice_first && run.slice_first->fallback) QCHK(run.slice_first->fallback());
  if (!s->layout.empty()) QCHK(state_settle(s));
  if (s->fuse >= 2 && !s->force_generic && !g_force_generic) {
    const uint32_t K = (uint32_t)std::min<int64_t>(s->fuse, kMaxMfmaK);  // both precisions have a matrix-core k = 5 kernel
    if (s->n >= K + 4)
      return s->dtype == QIP_C64 ? apply_ops_fused<double>(s, run, ops, count, K) : apply_ops_fused<float>(s, run, ops, count, K);
  }
  if (floor_plan) {
    // an op that runs on matrix cores by itself is no tile item here (in a sweep it would be the register fold, not its fma chain)
    // and no gate overtakes it (its three-product forms do not commute exactly with S or Y on other bits)
    std::vector<char> alone(count);
    for (uint64_t i = 0; i < count; ++i) alone[i] = single_route(s, &ops[i]) == SingleRoute::kMatrixCores;
    TileSchedule sc;
    if (make_tile_schedule(s->dtype, s->n, ops, count, 1, true, &sc, /*allow_permute=*/false, &alone) == QIP_OK && sc.circuit == ops && sc.origin.empty())
      return s->dtype == QIP_C64 ? apply_ops_floor_plan<double>(s, sc, run) : apply_ops_floor_plan<float>(s, sc, run);
    (void)hipGetLastError();  // (a batch the scheduler rejects goes gate by gate: its failing op is reported there)
  }
  for (uint64_t i = 0; i < count; ++i) {
    // r5, option "pair_floor" (default 1): a gate whose selectors (controls, the target of a phase-type diagonal) sit inside a
    // 1-KiB wave row sweeps the WHOLE vector for half / a quarter of the algorithmic bytes — the memory system moves whole lines
    // (T on bit 0: 41 %, CNOT with its control inside a row: 40 %, profiles/r02_line_bits.md).  When such a gate and its
    // neighbour fit one tile they go as ONE two-item tile sweep (interpreter kernel, circuit order: the same unfused arithmetic
    // per amplitude, IEEE-equal to the two launches) — the neighbour rides for free.  Everything else stays one launch per gate.
    if (s->pair_floor && i + 1 < count && s->n >= (uint32_t)kPairFloorMinQubits && s->tile_passes && !s->capture_pool && !s->force_generic &&
        !g_force_generic) {
      // What the two launches move, in sweeps of the whole vector (floor_share): worth one two-item sweep from 1.3 — T on a low
      // bit + H (1 + 1), CNOT with a low control + anything.  (Here only where a batch plan does not own the batch, see above.)
      bool floor_gate = false, both = true;
      double moved = 0;
      for (int j = 0; j < 2 && both; ++j) {
        TileItem it;
        double share = 0;
        bool fg = false;
        both = classify_tile_item(s->dtype, s->n, &ops[i + j], &it) == QIP_OK && floor_share(s, &ops[i + j], it, &share, &fg) &&
               single_route(s, &ops[i + j]) != SingleRoute::kMatrixCores;
        floor_gate = floor_gate || fg;
        moved += share;
      }
      if (both && floor_gate && moved >= kFloorFuseSweeps) {
        TileSchedule sc;
        if (make_tile_schedule(s->dtype, s->n, &ops[i], 2, 1, true, &sc) == QIP_OK && sc.steps.size() == 1 && sc.steps[0].ops.size() == 2 &&
            sc.steps[0].perm.empty()) {
          BatchRun pair = run;
          pair.tile = 1;
          pair.tile_jit = pair.tile_relabel = pair.tile_wide = 0;
          // the sharded state's requests belong to the BATCH's last step, not to this pair's: a pair in the middle of the batch
          // must not store packed (the gates after it would run on the packed buffer) — only the batch's last two ops may
          if (i + 2 < count) pair.fold_request = nullptr;
          pair.slice_first = pair.slice_last = nullptr;
          const int rc = tiled(&ops[i], 2, pair);
          if (rc != QIP_OK) {
            std::string msg = g_last_error;
            return fail(rc, "ops %llu, %llu: %s", (unsigned long long)i, (unsigned long long)i + 1, msg.c_str());
          }
          ++i;
          continue;
        }
        (void)hipGetLastError();
      }
    }
    const TileStorePerm* fold = i + 1 == count ? run.fold_request : nullptr;  // (a last op that runs as a one-op tile sweep may store packed)
    int rc = s->dtype == QIP_C64 ? apply_op_t<double>(s, &ops[i], run, fold) : apply_op_t<float>(s, &ops[i], run, fold);
    if (rc != QIP_OK) {
      std::string msg = g_last_error;
      return fail(rc, "op %llu: %s", (unsigned long long)i, msg.c_str());
    }
  }
  return QIP_OK;
} QIP_CATCH_ALL

extern "C" int qip_hip_state_apply_ops(qip_hip_state* s, const qip_op* ops, uint64_t count) try {
  if (!s) return fail(QIP_ERR_INVALID, "null state handle");
  return apply_ops_run(s, ops, count, BatchRun(*s));
} QIP_CATCH_ALL

// ---------------------------------------------------------------------------------------
// programs: a circuit PREPARED once — every op's tables packed and resident in device memory the program owns — and
// recorded into a hipGraph: a run is one graph launch of kernel nodes only (nothing is packed, uploaded or decided again).
// Ops that write the second buffer (the literal gather, k_sparse_ell, bit-permutation sweeps) are recorded like the rest:
// the ping-pong is deterministic, so a program keeps one recording per starting buffer (at most two) and follows the
// buffers on the host after every launch, the way the reference swaps `state` and `arena` (builder.rs:514).
// ---------------------------------------------------------------------------------------
struct ProgRecording {
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  void *start_cur = nullptr, *start_alt = nullptr;  // the buffers the recording reads first / writes first
  bool swaps = false;                                // an odd number of out-of-place launches: the buffers end exchanged
  bool uses_alt = false;                             // some launch writes the second buffer
  ProgPool pool;                                     // the device copy of the ops' payloads
  uint64_t jit_gen = 0;                              // run-time-compiled kernels the cache may since have unloaded
};
struct qip_hip_program {
  qip_hip_state* s = nullptr;
  const qip_op* ops = nullptr;
  uint64_t count = 0;
  ProgRecording rec[2];
  bool capture_failed = false;  // an obstacle that will not go away (profile / force_generic aside): stay eager, do not retry every run
  int last_was_graph = 0;
  // r5, option "tile_auto": a program is made to be replayed, so it repays a compilation — created on a state with tile >= 1 and
  // tile_jit = 0 (the interpreter, what apply_ops keeps using) it runs its own launches with run-time-compiled wide segments.
  // Same arithmetic, same order: the
  // results are bit-identical to the interpreter's (tile = 1) / within the mode's own bar (tile = 2).
  bool auto_jit = false, auto_wide = false;
};
// the settings ITS launches (capture, replay, eager run) are issued with: the state's options, and the automatic ones
static BatchRun program_run_of(const qip_hip_program* p) {
  BatchRun run(*p->s);
  if (p->auto_jit) {
    run.tile_jit = 1;
    run.tile_wide = p->auto_wide ? 1 : 0;
  }
  return run;
}

static void recording_drop(ProgRecording* r) {
  if (r->exec) (void)hipGraphExecDestroy(r->exec);
  if (r->graph) (void)hipGraphDestroy(r->graph);
  if (r->pool.base) (void)hipFree(r->pool.base);
  *r = ProgRecording();
}
static void program_drop_graph(qip_hip_program* p) {
  for (ProgRecording& r : p->rec) recording_drop(&r);
}
void programs_orphan(qip_hip_state* s) {
  for (qip_hip_program* p : s->programs) {
    program_drop_graph(p);
    p->s = nullptr;
  }
  s->programs.clear();
}

// Record the program for the state's CURRENT buffers into `r`; on any obstacle leave `r` empty (the run is eager then) and report
// success — only a real descriptor error is returned.
static int program_capture(qip_hip_program* p, ProgRecording* r) {
  qip_hip_state* s = p->s;
  const BatchRun run = program_run_of(p);
  recording_drop(r);
  if (s->force_generic || g_force_generic || s->profile) return QIP_OK;
  if (!s->stream) return QIP_OK;  // (the legacy default stream of a wrapped state cannot be captured)
  // the second buffer must exist BEFORE the recording starts (no allocation inside a stream capture): ask for it when any launch
  // of the plan writes out of place; a state too large for it stays eager (and fails there with the allocation's own message)
  bool out_of_place = false;
  for (uint64_t i = 0; i < p->count && !out_of_place; ++i) {
    FlatOp f;
    QCHK(flatten_op(s->n, &p->ops[i], false, &f));
    Plan pl;
    QCHK(make_plan(s->dtype, s->n, f, false, &pl));
    const uint32_t k = f.n_op;
    const bool reg_or_mfma = pl.cls == KC_GATE_KQ && (k <= kMaxRegK || (s->mfma && k <= kMaxHugeK && s->n >= f.k_all + 4));
    if (pl.cls == KC_GATHER_GENERIC && sparse_tile_applies(s, pl, f)) continue;  // (in place through k_sparse_tile)
    out_of_place = pl.cls == KC_GATHER_GENERIC || (pl.cls == KC_GATE_KQ && !reg_or_mfma);
  }
  if (!out_of_place && run.tile >= 1 && s->n >= (uint32_t)kTileBits) {  // a bit-permutation sweep is out of place too
    TileSchedule sc;
    QCHK(make_tile_schedule(s->dtype, s->n, p->ops, p->count, tile_mode_of(s, run), s->tile_passes != 0, &sc));
    for (const TileStep& st : sc.steps) out_of_place = out_of_place || !st.perm.empty();
  }
  if (out_of_place && !s->alt && ensure_alt(s) != QIP_OK) {
    (void)hipGetLastError();
    p->capture_failed = true;
    return QIP_OK;
  }
  if (run.tile >= 1 && run.tile_jit) {  // run-time compilation cannot happen inside a stream capture: do it now
    BatchRun prepare = run;
    prepare.jit = BatchRun::kPrepare;
    QCHK(apply_ops_run(s, p->ops, p->count, prepare));
  }
  void* const arena0 = s->arena;
  const size_t arena_cap0 = s->arena_cap;
  void *const cur0 = s->cur, *const alt0 = s->alt;
  const bool owns_cur0 = s->owns_cur, owns_alt0 = s->owns_alt;
  ProgPool& pool = r->pool;
  int result = QIP_OK;
  for (int attempt = 0; attempt < 2; ++attempt) {
    if (!pool.base) {
      pool.cap = std::max<size_t>(pool.cap, 1 << 16);
      if (hipMalloc(&pool.base, pool.cap) != hipSuccess) {
        (void)hipGetLastError();
        pool = ProgPool();
        p->capture_failed = true;
        break;
      }
    }
    pool.used = 0;
    pool.overflow = false;
    pool.image.clear();
    if (hipStreamBeginCapture(s->stream, hipStreamCaptureModeRelaxed) != hipSuccess) {
      (void)hipGetLastError();
      p->capture_failed = true;
      break;
    }
    s->capture_pool = &pool;
    jit_capture_scope(+1);
    const int rc = apply_ops_run(s, p->ops, p->count, run);
    s->capture_pool = nullptr;
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(s->stream, &g);
    jit_capture_scope(-1);
    // the recording ISSUED nothing: the host's view of the buffers goes back to where it was (the launch will move it)
    const bool swapped = s->cur != cur0;
    s->cur = cur0;
    s->alt = alt0;
    s->owns_cur = owns_cur0;
    s->owns_alt = owns_alt0;
    s->arena = arena0;
    s->arena_cap = arena_cap0;
    if (rc == QIP_OK && e == hipSuccess && g && !pool.overflow) {
      bool ok = true;
      if (pool.used) {
        pool.image.resize(pool.used);
        ok = hipMemcpy(pool.base, pool.image.data(), pool.used, hipMemcpyHostToDevice) == hipSuccess;
      }
      pool.image.clear();
      pool.image.shrink_to_fit();
      if (ok && hipGraphInstantiate(&r->exec, g, nullptr, nullptr, 0) == hipSuccess) {
        r->graph = g;
        r->start_cur = cur0;
        r->start_alt = alt0;
        r->swaps = swapped;
        r->uses_alt = out_of_place;
        r->jit_gen = jit_cache_generation();
        return QIP_OK;
      }
      (void)hipGetLastError();
      (void)hipGraphDestroy(g);
      r->exec = nullptr;
      p->capture_failed = true;
      break;
    }
    if (g) (void)hipGraphDestroy(g);
    (void)hipGetLastError();
    if (rc == QIP_OK && e == hipSuccess && pool.overflow) {  // the sizing pass: now the pool's size is known — once more
      (void)hipFree(pool.base);
      pool.base = nullptr;
      pool.cap = pool.used + 4096;
      continue;
    }
    if (rc != QIP_OK && rc != QIP_ERR_UNSUPPORTED) result = rc;  // a real descriptor error
    else p->capture_failed = true;
    break;
  }
  recording_drop(r);
  return result;
}

extern "C" int qip_hip_program_create(qip_hip_state* s, const qip_op* ops, uint64_t count,
                                      qip_hip_program** out) try {
  STATE_ENTER(s);
  if (!out || (count && !ops)) return fail(QIP_ERR_INVALID, "null argument");
  for (uint64_t i = 0; i < count; ++i) {
    FlatOp f;
    int rc = flatten_op(s->n, &ops[i], false, &f);
    if (rc != QIP_OK) {
      std::string msg = g_last_error;
      return fail(rc, "op %llu: %s", (unsigned long long)i, msg.c_str());
    }
  }
  qip_hip_program* p = new qip_hip_program();
  p->s = s;
  p->ops = ops;
  p->count = count;
  if (s->tile_auto && s->tile >= 1 && !s->tile_jit && s->tile_passes && s->n >= (uint32_t)kAutoJitMinQubits && !s->force_generic && !g_force_generic) {
    p->auto_jit = true;
    p->auto_wide = s->n > (uint32_t)kWideBits;  // (dense 3-qubit items included since they are written out group by group: tile_wide_dense3_inline)
  }
  int rc = program_capture(p, &p->rec[0]);
  if (rc != QIP_OK && p->auto_jit) {
    // the automatic choice must not turn a compiler problem (libhiprtc missing, a hiprtc error on one segment) into a
    // failed program_create — without it the interpreter would have served.  Drop the automatic options and record again with the
    // state's own; only options the CALLER set propagate their errors.
    p->auto_jit = p->auto_wide = false;
    p->capture_failed = false;
    rc = program_capture(p, &p->rec[0]);
  }
  if (rc != QIP_OK) {
    program_drop_graph(p);
    delete p;
    return rc;
  }
  s->programs.push_back(p);
  *out = p;
  return QIP_OK;
} QIP_CATCH_ALL

extern "C" int qip_hip_program_run(qip_hip_program* p) try {
  if (!p) return fail(QIP_ERR_INVALID, "null program");
  qip_hip_state* s = p->s;
  if (!s) return fail(QIP_ERR_INVALID, "the state this program was recorded against has been destroyed");
  STATE_ENTER(s);
  const BatchRun run = program_run_of(p);
  if (s->profile || s->force_generic || g_force_generic) {  // (profiling brackets every kernel with events; the literal kernel is a test route)
    p->last_was_graph = 0;
    return apply_ops_run(s, p->ops, p->count, run);
  }
  for (int attempt = 0; attempt < 2; ++attempt) {
    // the recording made for the buffers as they are now; none yet (the previous run left the state on its other buffer, an eager
    // op exchanged them): record into the free slot, or over the one that does not start here
    ProgRecording* r = nullptr;
    for (ProgRecording& c : p->rec)
      if (c.exec && c.start_cur == s->cur && (!c.uses_alt || c.start_alt == s->alt)) r = &c;
    if (!r) {
      if (p->capture_failed) break;
      ProgRecording* slot = !p->rec[0].exec ? &p->rec[0] : (!p->rec[1].exec ? &p->rec[1] : (p->rec[0].start_cur == s->alt ? &p->rec[1] : &p->rec[0]));
      QCHK(program_capture(p, slot));
      if (!slot->exec) break;
      r = slot;
    }
    // a graph with compiled segments names resident kernels: not launched once the cache has evicted since its recording
    const auto launch = [&]() -> int {
      HIPCHK(hipGraphLaunch(r->exec, s->stream));
      return QIP_OK;
    };
    bool stale = false;
    if (run.tile_jit) QCHK(jit_launch_if_current(r->jit_gen, launch, &stale));
    else QCHK(launch());
    if (stale) {
      recording_drop(r);
      continue;
    }
    if (r->swaps) {  // builder.rs:514
      std::swap(s->cur, s->alt);
      std::swap(s->owns_cur, s->owns_alt);
    }
    p->last_was_graph = 1;
    return QIP_OK;
  }
  p->last_was_graph = 0;
  return apply_ops_run(s, p->ops, p->count, run);
} QIP_CATCH_ALL

extern "C" int qip_hip_program_is_graph(const qip_hip_program* p) try { return p ? p->last_was_graph : 0; } QIP_CATCH_ALL

extern "C" int qip_hip_program_destroy(qip_hip_program* p) try {
  if (!p) return QIP_OK;
  if (p->s) {
    (void)hipSetDevice(p->s->device);
    (void)hipStreamSynchronize(p->s->stream);
    auto& v = p->s->programs;
    v.erase(std::remove(v.begin(), v.end(), p), v.end());
  }
  program_drop_graph(p);
  delete p;
  return QIP_OK;
} QIP_CATCH_ALL
