// qip_pauli.hip — the Pauli-string calls on device states and the vector arithmetic of resident states (include/qip_hipx.h).
//   reduce  every term to (x mask, z mask, n_Y mod 4) over amplitude-index bits (pauli_terms: the one entry check of the term arrays)
//   plan    passes of at most `group` terms of one x mask (qip_pauli_plan.h: sorted by x for expect / sum / matrix elements, runs of
//           consecutive terms for the rotations; also all that the qipx_*_passes calls run)
//   pass    one kernel launch in the geometry of its x mask (pauli_geom), the descriptor = the shared head (pauli_masks) + the
//           family's own tail; the kernel instantiation (packed / pair / slot capacity) is chosen by pauli_dispatch
// The geometry depends on n, the precision and the class of the x mask only, never on the group: together with the kernels'
// per-slot arithmetic that makes a result a function of the states and its term.
// The diagonal sums (apply_diagonal, expect_diagonal) take all their terms in ONE pass of their own: see their section.
#include "qip_internal.h"
#include "../../include/qip_hipx.h"
#include "qip_pauli_kernels.h"
#include "qip_diag_kernels.h"

// ---- shared by every call -----------------------------------------------------------------------------------------------------
// `what`: the call's name in a refusal
static int pauli_terms(const char* what, uint32_t n, const uint64_t* term_start, const uint64_t* qubits, const uint8_t* paulis,
                       uint64_t count, std::vector<PauliTerm>* terms) {
  if (count > 0xffffffffull) return fail(QIP_ERR_UNSUPPORTED, "%s: more than 2^32 - 1 terms", what);
  if (n > 63) return fail(QIP_ERR_INVALID, "%s: %u qubits", what, n);
  if (!term_start || !qubits || !paulis) return fail(QIP_ERR_INVALID, "%s: null term array", what);
  if (term_start[0] != 0) return fail(QIP_ERR_INVALID, "%s: term_start[0] is not 0", what);
  terms->resize(count);
  for (uint64_t t = 0; t < count; ++t) {
    if (term_start[t + 1] < term_start[t]) return fail(QIP_ERR_INVALID, "%s: term_start decreases at term %llu", what, (unsigned long long)t);
    PauliTerm pt{0, 0, 0};
    uint64_t seen = 0;
    for (uint64_t i = term_start[t]; i < term_start[t + 1]; ++i) {
      if (qubits[i] >= n) return fail(QIP_ERR_INVALID, "%s: qubit %llu of term %llu out of range", what, (unsigned long long)qubits[i], (unsigned long long)t);
      if (paulis[i] > 3) return fail(QIP_ERR_INVALID, "%s: Pauli code %u in term %llu", what, (unsigned)paulis[i], (unsigned long long)t);
      const uint64_t bit = 1ull << (n - 1 - qubits[i]);
      if (seen & bit) return fail(QIP_ERR_INVALID, "%s: qubit %llu repeated in term %llu", what, (unsigned long long)qubits[i], (unsigned long long)t);
      seen |= bit;
      if (paulis[i] == 1 || paulis[i] == 2) pt.x |= bit;
      if (paulis[i] == 2 || paulis[i] == 3) pt.z |= bit;
      if (paulis[i] == 2) pt.ny = (pt.ny + 1) & 3u;
    }
    (*terms)[t] = pt;
  }
  return QIP_OK;
}

// the three qipx_*_passes calls: the planner of the call, run on the host alone
static int pauli_passes(const char* what, const char* option, int max_group, int64_t default_group, bool sorted, uint32_t n,
                        const uint64_t* term_start, const uint64_t* qubits, const uint8_t* paulis, uint64_t count, uint32_t group,
                        uint64_t* passes) {
  if (!passes) return fail(QIP_ERR_INVALID, "null output");
  if (group > (uint32_t)max_group) return fail(QIP_ERR_INVALID, "%s is 1 to %d", option, max_group);
  *passes = 0;
  if (count == 0) return QIP_OK;
  std::vector<PauliTerm> terms;
  QCHK(pauli_terms(what, n, term_start, qubits, paulis, count, &terms));
  std::vector<uint32_t> order;
  std::vector<PauliPass> plan;
  if (sorted) pauli_plan_sorted(terms, group ? group : (uint32_t)default_group, &order, &plan);
  else pauli_plan_in_order(terms, group ? group : (uint32_t)default_group, &plan);
  *passes = plan.size();
  return QIP_OK;
}

template <typename T>
static PauliGeom geom_of(const qip_hip_state* s, uint64_t x) {
  return pauli_geom(s->n, std::is_same<T, float>::value && s->packed_f32, x);
}

static Ins pauli_ins(const PauliGeom& g) { return g.pair ? make_ins({g.hbit}, 0) : make_ins({}, 0); }

// The kernel instantiation of a pass: launch(TypeC<E>, IntC<PAIR>, IntC<G>) with E = the element the pass reads (f32x4: two packed
// Complex<f32>), PAIR = x != 0 and G = the smallest capacity of the family's list (ascending) that holds `count` slots.
namespace {
template <typename E> struct TypeC { using type = E; };
template <int... G> struct Caps {};
}  // namespace

template <typename E, int PAIR, int G0, int... GS, typename F>
static void pauli_capacity(uint32_t count, Caps<G0, GS...>, F&& launch) {
  if constexpr (sizeof...(GS) == 0) {
    launch(TypeC<E>{}, IntC<PAIR>{}, IntC<G0>{});
  } else {
    if (count <= (uint32_t)G0) launch(TypeC<E>{}, IntC<PAIR>{}, IntC<G0>{});
    else pauli_capacity<E, PAIR>(count, Caps<GS...>{}, launch);
  }
}

template <typename T, int... GS, typename F>
static void pauli_dispatch(const PauliGeom& g, uint32_t count, Caps<GS...> caps, F&& launch) {
  if constexpr (std::is_same<T, float>::value) {
    if (g.packed) {
      if (g.pair) pauli_capacity<f32x4, 1>(count, caps, launch);
      else pauli_capacity<f32x4, 0>(count, caps, launch);
      return;
    }
  }
  if (g.pair) pauli_capacity<amp_t<T>, 1>(count, caps, launch);
  else pauli_capacity<amp_t<T>, 0>(count, caps, launch);
}

// The reducing calls (expect_pauli, pauli_matrix_elements): every pass leaves W doubles per slot and block in the scratch of `s`,
// slot-major (partial[(W slot + c) nblocks + block]).  As many passes share a synchronise as keep their partial sums within 2^20
// doubles (one pass needs at most 32 * 4096); the host adds a slot's partial sums in block order and hands them to `finish`.
//   launch(geometry, ids, count, partial)   queues one pass on s->stream: slot g holds terms[ids[g]]
//   finish(geometry, term id, sums[W])      a finished slot becomes the caller's value
template <typename T, int W, typename Launch, typename Finish>
static int pauli_reduce_passes(qip_hip_state* s, const std::vector<PauliTerm>& terms, uint32_t group, Launch&& launch, Finish&& finish) {
  std::vector<uint32_t> order;
  std::vector<PauliPass> plan;
  pauli_plan_sorted(terms, group, &order, &plan);
  std::vector<PauliGeom> geom(plan.size());
  size_t total = 0;
  for (size_t p = 0; p < plan.size(); ++p) {
    geom[p] = geom_of<T>(s, terms[order[plan[p].first]].x);
    total += W * (size_t)plan[p].count * geom[p].nblocks;
  }
  const size_t cap = std::min<size_t>(total, (size_t)1 << 20);
  QCHK(ensure_partial(s, cap));
  std::vector<double> part(cap);
  for (size_t p = 0; p < plan.size();) {
    size_t used = 0, q = p;
    for (; q < plan.size(); ++q) {
      const size_t need = W * (size_t)plan[q].count * geom[q].nblocks;
      if (used + need > cap) break;
      launch(geom[q], order.data() + plan[q].first, plan[q].count, s->d_partial + used);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(part.data() + used, s->d_partial + used, need * sizeof(double), hipMemcpyDeviceToHost, s->stream));
      used += need;
    }
    HIPCHK(hipStreamSynchronize(s->stream));
    for (size_t at = 0; p < q; ++p) {
      const uint32_t nb = geom[p].nblocks;
      for (uint32_t slot = 0; slot < plan[p].count; ++slot, at += W * (size_t)nb) {
        double sums[W] = {};
        for (uint32_t b = 0; b < nb; ++b)
          for (int c = 0; c < W; ++c) sums[c] += part[at + (size_t)c * nb + b];
        finish(geom[p], order[plan[p].first + slot], sums);
      }
    }
  }
  return QIP_OK;
}

// ---- expectation values of Pauli strings ----------------------------------------------------------------------------------------
extern "C" int qipx_expect_pauli_passes(uint32_t n, const uint64_t* term_start, const uint64_t* qubits, const uint8_t* paulis,
                                        uint64_t count, uint32_t group, uint64_t* passes) try {
  return pauli_passes("expect_pauli", "expect_group", kExpectMaxGroup, kExpectGroupDefault, true, n, term_start, qubits, paulis, count, group, passes);
} QIP_CATCH_ALL

template <typename T>
static int expect_pauli_t(qip_hip_state* s, const std::vector<PauliTerm>& terms, double* values) {
  return pauli_reduce_passes<T, 1>(
      s, terms, (uint32_t)s->expect_group,
      [&](const PauliGeom& g, const uint32_t* ids, uint32_t count, double* partial) {
        ExpectDesc d;
        memset(&d, 0, sizeof d);
        static_cast<PauliMasks&>(d) = pauli_masks(g, s->n, terms.data(), ids, count);
        for (uint32_t slot = 0; slot < count; ++slot) {
          const uint32_t ny = terms[ids[slot]].ny;
          if (ny == 1 || ny == 2) d.flip |= 1u << slot;
          if (ny & 1u) d.imag |= 1u << slot;
        }
        pauli_dispatch<T>(g, count, Caps<1, 4, 16, kExpectMaxGroup>{}, [&](auto e, auto pair, auto cap) {
          using E = typename decltype(e)::type;
          hipLaunchKernelGGL((k_expect_pauli<T, decltype(cap)::v, decltype(pair)::v != 0, E>), dim3(g.nblocks), dim3(kBlock), 0, s->stream,
                             (const E*)s->cur, g.nwork, g.chunk, pauli_ins(g), d, partial);
        });
      },
      [&](const PauliGeom& g, uint32_t id, const double* sum) { values[id] = g.pair ? 2.0 * sum[0] : sum[0]; });  // (j and j ^ x: conjugates)
}

extern "C" int qipx_state_expect_pauli(qip_hip_state* s, const uint64_t* term_start, const uint64_t* qubits, const uint8_t* paulis,
                                       uint64_t count, double* values) try {
  STATE_ENTER(s);
  if (count == 0) return QIP_OK;
  if (!values) return fail(QIP_ERR_INVALID, "expect_pauli: null result array");
  std::vector<PauliTerm> terms;
  QCHK(pauli_terms("expect_pauli", s->n, term_start, qubits, paulis, count, &terms));
  return s->dtype == QIP_C64 ? expect_pauli_t<double>(s, terms, values) : expect_pauli_t<float>(s, terms, values);
} QIP_CATCH_ALL

// ---- Pauli-string rotations exp(-i theta P) in place ------------------------------------------------------------------------------
// The angles: finite, cos and sin in double.  The terms keep their order (they do not commute in general): one k_pauli_rotate launch
// per run of consecutive terms of one x mask, queued on the stream.  Everything is checked before the first launch; nothing is
// waited for.
extern "C" int qipx_pauli_rotation_passes(uint32_t n, const uint64_t* term_start, const uint64_t* qubits, const uint8_t* paulis,
                                          uint64_t count, uint32_t group, uint64_t* passes) try {
  return pauli_passes("pauli_rotations", "rotate_group", kRotateMaxGroup, kRotateGroupDefault, false, n, term_start, qubits, paulis, count, group, passes);
} QIP_CATCH_ALL

template <typename T>
static int rotate_t(qip_hip_state* s, const std::vector<PauliTerm>& terms, const double* angles) {
  std::vector<PauliPass> plan;
  pauli_plan_in_order(terms, (uint32_t)s->rotate_group, &plan);
  for (const PauliPass& pass : plan) {
    const PauliGeom g = geom_of<T>(s, terms[pass.first].x);
    RotateDesc<T> d;
    memset(&d, 0, sizeof d);
    static_cast<PauliMasks&>(d) = pauli_masks(g, s->n, terms.data() + pass.first, nullptr, pass.count);
    for (uint32_t slot = 0; slot < pass.count; ++slot) {
      const PauliTerm& t = terms[pass.first + slot];
      const uint32_t p = (t.ny + 3u) & 3u;  // -i i^n_Y = i^p
      if (p & 1u) d.swap |= 1u << slot;
      if (p & 2u) d.hi |= 1u << slot;
      if (t.ny & 1u) d.odd |= 1u << slot;
      d.c[slot] = (T)cos(angles[pass.first + slot]);  // in double, rounded once to the state's precision
      d.s[slot] = (T)sin(angles[pass.first + slot]);
    }
    // (the largest capacity is a loop over the slots in use: one kernel for 5 to 32 terms)
    pauli_dispatch<T>(g, pass.count, Caps<1, 4, kRotateMaxGroup>{}, [&](auto e, auto pair, auto cap) {
      using E = typename decltype(e)::type;
      hipLaunchKernelGGL((k_pauli_rotate<T, decltype(cap)::v, decltype(pair)::v != 0, E>), dim3(g.nblocks), dim3(kBlock), 0, s->stream,
                         (E*)s->cur, g.nwork, g.chunk, pauli_ins(g), d);
    });
    HIPCHK(hipGetLastError());
  }
  return QIP_OK;
}

extern "C" int qipx_state_apply_pauli_rotations(qip_hip_state* s, const uint64_t* term_start, const uint64_t* qubits,
                                                const uint8_t* paulis, const double* angles, uint64_t count) try {
  STATE_ENTER_RAW(s);
  if (count == 0) return QIP_OK;
  if (!angles) return fail(QIP_ERR_INVALID, "pauli_rotations: null angle array");
  std::vector<PauliTerm> terms;
  QCHK(pauli_terms("pauli_rotations", s->n, term_start, qubits, paulis, count, &terms));
  for (uint64_t t = 0; t < count; ++t)
    if (!std::isfinite(angles[t])) return fail(QIP_ERR_INVALID, "pauli_rotations: the angle of term %llu is not finite", (unsigned long long)t);
  if (!s->layout.empty()) QCHK(state_settle(s));  // (a relabelled state: the caller's order first, as by STATE_ENTER)
  return s->dtype == QIP_C64 ? rotate_t<double>(s, terms, angles) : rotate_t<float>(s, terms, angles);
} QIP_CATCH_ALL

// ---- diagonal Pauli sums D = sum_t c_t Z-string_t in one pass: exp(-i gamma D) in place, <D> and <D^2> ---------------------------------
//   check   the terms as every call above (pauli_terms), then: no X or Y factor, finite coefficients, k_t = fl(gamma c_t) finite
//   plan    qip_diag_plan.h: every z mask split at the tile boundary, the terms sorted stably by low mask into groups
//   table   terms, group starts and group masks in ONE handle-owned device buffer, uploaded through one of two handle-owned pinned
//           copies, taken in turn
//   launch  ONE k_diag_phase / k_diag_moments launch whatever the number of terms (qip_diag_kernels.h)
// The upload is stream-ordered and the phase call returns without waiting, so two things must hold.  The device table is rewritten
// only by a copy queued on the stream behind the kernel that read it.  A pinned copy is rewritten by the host only after the
// event recorded behind ITS last upload has passed (diag_upload waits for it: with two copies taken in turn that is the upload of
// the call before the previous one, so one call's work can still be queued while the next one is prepared).
// Growing the buffers waits for the stream first.
static int diag_check(const char* what, qip_hip_state* s, const uint64_t* term_start, const uint64_t* qubits, const uint8_t* paulis,
                      const double* coeffs, uint64_t count, double gamma, DiagPlan* plan) {
  if (count > kDiagMaxTerms)
    return fail(QIP_ERR_UNSUPPORTED, "%s: %llu terms, at most %llu are supported", what, (unsigned long long)count, (unsigned long long)kDiagMaxTerms);
  if (!coeffs) return fail(QIP_ERR_INVALID, "%s: null coefficient array", what);
  std::vector<PauliTerm> terms;
  QCHK(pauli_terms(what, s->n, term_start, qubits, paulis, count, &terms));
  for (uint64_t t = 0; t < count; ++t)
    if (terms[t].x != 0) return fail(QIP_ERR_INVALID, "%s: term %llu is not diagonal", what, (unsigned long long)t);
  if (!std::isfinite(gamma)) return fail(QIP_ERR_INVALID, "%s: gamma is not finite", what);
  std::vector<uint64_t> z(count);
  std::vector<double> k(count);
  for (uint64_t t = 0; t < count; ++t) {
    if (!std::isfinite(coeffs[t])) return fail(QIP_ERR_INVALID, "%s: the coefficient of term %llu is not finite", what, (unsigned long long)t);
    z[t] = terms[t].z;
    k[t] = gamma * coeffs[t];
    if (!std::isfinite(k[t])) return fail(QIP_ERR_INVALID, "%s: gamma times the coefficient of term %llu is not finite", what, (unsigned long long)t);
  }
  *plan = diag_plan(s->n, z.data(), k.data(), (size_t)count);
  return QIP_OK;
}

// The handle's table buffer (qip_internal.h: d_diag, h_diag): what every call that ships a table built on the host shares — the
// diagonal sums here and qipx_state_apply_function (qip_function.hip).  table_stage: room for `bytes` (grown after waiting for the
// stream), the pinned copy whose turn it is, free to be written; table_commit: its upload queued, the event behind it recorded.
int table_stage(qip_hip_state* s, size_t bytes, char** host, uint32_t* turn_out) {
  if (bytes > s->diag_cap) {
    HIPCHK(hipStreamSynchronize(s->stream));  // (a kernel may still read the old table, a copy the old host buffers)
    if (s->d_diag) HIPCHK(hipFree(s->d_diag));
    s->d_diag = nullptr;
    for (int i = 0; i < 2; ++i) {
      if (s->h_diag[i]) HIPCHK(hipHostFree(s->h_diag[i]));
      s->h_diag[i] = nullptr;
    }
    s->diag_cap = 0;
    const size_t cap = std::max<size_t>(bytes + bytes / 2, 1 << 16);
    HIPCHK(hipMalloc(&s->d_diag, cap));
    for (int i = 0; i < 2; ++i) HIPCHK(hipHostMalloc(&s->h_diag[i], cap, hipHostMallocDefault));
    s->diag_cap = cap;
  }
  const uint32_t turn = s->diag_turn;
  s->diag_turn ^= 1u;
  if (s->diag_uploaded[turn]) HIPCHK(hipEventSynchronize(s->diag_uploaded[turn]));  // this copy's last upload has left it
  else HIPCHK(hipEventCreateWithFlags(&s->diag_uploaded[turn], hipEventDisableTiming));
  *host = (char*)s->h_diag[turn];
  *turn_out = turn;
  return QIP_OK;
}

int table_commit(qip_hip_state* s, uint32_t turn, size_t bytes) {
  HIPCHK(hipMemcpyAsync(s->d_diag, s->h_diag[turn], bytes, hipMemcpyHostToDevice, s->stream));
  HIPCHK(hipEventRecord(s->diag_uploaded[turn], s->stream));
  return QIP_OK;
}

static int diag_upload(qip_hip_state* s, const DiagPlan& plan, const DiagGeom& g, DiagSumDesc* d) {
  const size_t nterms = plan.terms.size(), ngroups = plan.group_mask.size();
  const size_t off_start = nterms * sizeof(DiagTerm), off_mask = off_start + (ngroups + 1) * sizeof(uint32_t);
  const size_t bytes = off_mask + ngroups * sizeof(uint32_t);
  char* h = nullptr;
  uint32_t turn = 0;
  QCHK(table_stage(s, bytes, &h, &turn));
  memcpy(h, plan.terms.data(), nterms * sizeof(DiagTerm));
  memcpy(h + off_start, plan.group_start.data(), (ngroups + 1) * sizeof(uint32_t));
  memcpy(h + off_mask, plan.group_mask.data(), ngroups * sizeof(uint32_t));
  QCHK(table_commit(s, turn, bytes));
  d->terms = (const DiagTerm*)s->d_diag;
  d->group_start = (const uint32_t*)((const char*)s->d_diag + off_start);
  d->group_mask = (const uint32_t*)((const char*)s->d_diag + off_mask);
  d->ngroups = (uint32_t)ngroups;
  d->tile_bits = g.tile_bits;
  d->ntiles = g.ntiles;
  d->tiles_per_block = g.tiles_per_block;
  return QIP_OK;
}

static DiagGeom diag_geom_of(const qip_hip_state* s) {
#ifdef QIP_HIP_TUNING
  return diag_geom(s->n, s->dtype == QIP_C32 && s->packed_f32);
#else
  return diag_geom(s->n, s->dtype == QIP_C32);  // (Complex<f32> is always read in 16-byte elements of two amplitudes)
#endif
}

extern "C" int qipx_state_apply_diagonal(qip_hip_state* s, const uint64_t* term_start, const uint64_t* qubits, const uint8_t* paulis,
                                         const double* coeffs, uint64_t count, double gamma) try {
  STATE_ENTER_RAW(s);
  if (count == 0) return QIP_OK;
  DiagPlan plan;
  QCHK(diag_check("apply_diagonal", s, term_start, qubits, paulis, coeffs, count, gamma, &plan));
  if (!s->layout.empty()) QCHK(state_settle(s));  // (a relabelled state: the caller's order first, as by STATE_ENTER)
  const DiagGeom g = diag_geom_of(s);
  DiagSumDesc d;
  QCHK(diag_upload(s, plan, g, &d));
  const dim3 grid(g.nblocks), block(kBlock);
  if (s->dtype == QIP_C64) hipLaunchKernelGGL((k_diag_phase<double>), grid, block, 0, s->stream, (amp_t<double>*)s->cur, d);
  else if (g.shift) hipLaunchKernelGGL((k_diag_phase<float, f32x4>), grid, block, 0, s->stream, (f32x4*)s->cur, d);
#ifdef QIP_HIP_TUNING  // (option "packed_f32" = 0 exists in a tuning build only: the product build has no plain Complex<f32> walk)
  else hipLaunchKernelGGL((k_diag_phase<float>), grid, block, 0, s->stream, (amp_t<float>*)s->cur, d);
#endif
  HIPCHK(hipGetLastError());
  return QIP_OK;
} QIP_CATCH_ALL

extern "C" int qipx_state_expect_diagonal(qip_hip_state* s, const uint64_t* term_start, const uint64_t* qubits, const uint8_t* paulis,
                                          const double* coeffs, uint64_t count, double* moments) try {
  STATE_ENTER(s);
  if (count == 0) {
    if (moments) moments[0] = moments[1] = 0.0;
    return QIP_OK;
  }
  if (!moments) return fail(QIP_ERR_INVALID, "expect_diagonal: null result array");
  DiagPlan plan;
  QCHK(diag_check("expect_diagonal", s, term_start, qubits, paulis, coeffs, count, 1.0, &plan));  // (k_t = c_t: 1.0 * c is exact)
  const DiagGeom g = diag_geom_of(s);
  QCHK(ensure_partial(s, 2 * (size_t)g.nblocks));
  DiagSumDesc d;
  QCHK(diag_upload(s, plan, g, &d));
  const dim3 grid(g.nblocks), block(kBlock);
  if (s->dtype == QIP_C64) hipLaunchKernelGGL((k_diag_moments<double>), grid, block, 0, s->stream, (const amp_t<double>*)s->cur, d, s->d_partial);
  else if (g.shift) hipLaunchKernelGGL((k_diag_moments<float, f32x4>), grid, block, 0, s->stream, (const f32x4*)s->cur, d, s->d_partial);
#ifdef QIP_HIP_TUNING
  else hipLaunchKernelGGL((k_diag_moments<float>), grid, block, 0, s->stream, (const amp_t<float>*)s->cur, d, s->d_partial);
#endif
  HIPCHK(hipGetLastError());
  std::vector<double> part(2 * (size_t)g.nblocks);
  HIPCHK(hipMemcpyAsync(part.data(), s->d_partial, part.size() * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  double m1 = 0, m2 = 0;
  for (uint32_t b = 0; b < g.nblocks; ++b) m1 += part[b], m2 += part[g.nblocks + b];
  moments[0] = m1, moments[1] = m2;
  return QIP_OK;
} QIP_CATCH_ALL

// ---- two states and Pauli strings: dst (+)= (sum_t c_t P_t) src and <bra| P_t |ket> ---------------------------------------------
//   meet    the two handles as copy_from and max_abs_diff meet theirs (pair_meet: the checks; pair_settle: the caller's order and
//           the other handle's stream drained), everything that can refuse the call before anything is queued
// Both calls are complete when they return.
int pair_meet(const char* what, qip_hip_state* own, qip_hip_state* other) {
  if (!other) return fail(QIP_ERR_INVALID, "%s: null state handle", what);
  if (other->poisoned) return fail(QIP_ERR_DEVICE, "%s: the other state is unusable: %s", what, other->poison_msg.c_str());
  if (own->n != other->n || own->dtype != other->dtype) return fail(QIP_ERR_INVALID, "%s: states differ in size or precision", what);
  if (own->device != other->device) return fail(QIP_ERR_UNSUPPORTED, "%s: states live on different devices", what);
  return QIP_OK;
}

// both in the caller's order, and everything queued on `other` has landed: the work then runs on `own`'s stream
int pair_settle(qip_hip_state* own, qip_hip_state* other) {
  if (!own->layout.empty()) QCHK(state_settle(own));
  if (other != own) {
    if (!other->layout.empty()) QCHK(state_settle(other));
    HIPCHK(hipStreamSynchronize(other->stream));
  }
  return QIP_OK;
}

extern "C" int qipx_pauli_sum_passes(uint32_t n, const uint64_t* term_start, const uint64_t* qubits, const uint8_t* paulis,
                                     uint64_t count, uint32_t group, uint64_t* passes) try {
  return pauli_passes("pauli_sum", "sum_group", kSumMaxGroup, kSumGroupDefault, true, n, term_start, qubits, paulis, count, group, passes);
} QIP_CATCH_ALL

template <typename T>
static int pauli_sum_t(qip_hip_state* dst, const qip_hip_state* src, const std::vector<PauliTerm>& terms, const double* coeffs,
                       bool accumulate) {
  std::vector<uint32_t> order;
  std::vector<PauliPass> plan;
  pauli_plan_sorted(terms, (uint32_t)dst->sum_group, &order, &plan);
  if (plan.empty() && !accumulate) HIPCHK(hipMemsetAsync(dst->cur, 0, dst->namps * dst->amp_bytes, dst->stream));
  bool first = !accumulate;  // the first pass of a storing call does not read the destination
  for (const PauliPass& pass : plan) {
    const uint32_t* ids = order.data() + pass.first;
    const PauliGeom g = geom_of<T>(dst, terms[ids[0]].x);
    SumDesc<T> d;
    memset(&d, 0, sizeof d);
    static_cast<PauliMasks&>(d) = pauli_masks(g, dst->n, terms.data(), ids, pass.count);
    for (uint32_t slot = 0; slot < pass.count; ++slot) {
      const PauliTerm& t = terms[ids[slot]];
      if (t.ny & 1u) d.odd |= 1u << slot;
      const double cr = coeffs[2 * (size_t)ids[slot]], ci = coeffs[2 * (size_t)ids[slot] + 1];
      // k = c i^n_Y: a swap and sign flips in double, then rounded once to the state's precision
      d.kr[slot] = (T)(t.ny == 0 ? cr : t.ny == 1 ? -ci : t.ny == 2 ? -cr : ci);
      d.ki[slot] = (T)(t.ny == 0 ? ci : t.ny == 1 ? cr : t.ny == 2 ? -ci : -cr);
    }
    // (the largest capacity is a loop over the slots in use: one kernel for 5 to 32 terms)
    pauli_dispatch<T>(g, pass.count, Caps<1, 4, kSumMaxGroup>{}, [&](auto e, auto pair, auto cap) {
      using E = typename decltype(e)::type;
      constexpr int G = decltype(cap)::v;
      constexpr bool PAIR = decltype(pair)::v != 0;
      const dim3 grid(g.nblocks), block(kBlock);
      if (first) hipLaunchKernelGGL((k_pauli_sum<T, G, PAIR, true, E>), grid, block, 0, dst->stream, (E*)dst->cur, (const E*)src->cur, g.nwork, g.chunk, pauli_ins(g), d);
      else hipLaunchKernelGGL((k_pauli_sum<T, G, PAIR, false, E>), grid, block, 0, dst->stream, (E*)dst->cur, (const E*)src->cur, g.nwork, g.chunk, pauli_ins(g), d);
    });
    HIPCHK(hipGetLastError());
    first = false;
  }
  HIPCHK(hipStreamSynchronize(dst->stream));  // complete on return: the caller may touch `src` at once
  return QIP_OK;
}

extern "C" int qipx_state_apply_pauli_sum(qip_hip_state* dst, qip_hip_state* src, const uint64_t* term_start, const uint64_t* qubits,
                                          const uint8_t* paulis, const double* coeffs, uint64_t count, int accumulate) try {
  STATE_ENTER_RAW(dst);
  QCHK(pair_meet("pauli_sum", dst, src));
  if (dst == src) return fail(QIP_ERR_INVALID, "pauli_sum: the destination is the source (later passes need the source intact)");
  std::vector<PauliTerm> terms;
  if (count > 0) {
    if (!coeffs) return fail(QIP_ERR_INVALID, "pauli_sum: null coefficient array");
    QCHK(pauli_terms("pauli_sum", dst->n, term_start, qubits, paulis, count, &terms));
    for (uint64_t t = 0; t < count; ++t)
      if (!std::isfinite(coeffs[2 * t]) || !std::isfinite(coeffs[2 * t + 1]))
        return fail(QIP_ERR_INVALID, "pauli_sum: the coefficient of term %llu is not finite", (unsigned long long)t);
  }
  QCHK(pair_settle(dst, src));
  return dst->dtype == QIP_C64 ? pauli_sum_t<double>(dst, src, terms, coeffs, accumulate != 0)
                               : pauli_sum_t<float>(dst, src, terms, coeffs, accumulate != 0);
} QIP_CATCH_ALL

template <typename T>
static int pauli_melem_t(qip_hip_state* ket, const qip_hip_state* bra, const std::vector<PauliTerm>& terms, double* values) {
  return pauli_reduce_passes<T, 2>(
      ket, terms, (uint32_t)std::min<int64_t>(ket->expect_group, kMelemMaxGroup),
      [&](const PauliGeom& g, const uint32_t* ids, uint32_t count, double* partial) {
        MelemDesc d;
        memset(&d, 0, sizeof d);
        static_cast<PauliMasks&>(d) = pauli_masks(g, ket->n, terms.data(), ids, count);
        for (uint32_t slot = 0; slot < count; ++slot)
          if (terms[ids[slot]].ny & 1u) d.odd |= 1u << slot;
        pauli_dispatch<T>(g, count, Caps<1, 4, kMelemMaxGroup>{}, [&](auto e, auto pair, auto cap) {
          using E = typename decltype(e)::type;
          hipLaunchKernelGGL((k_pauli_melem<T, decltype(cap)::v, decltype(pair)::v != 0, E>), dim3(g.nblocks), dim3(kBlock), 0, ket->stream,
                             (const E*)bra->cur, (const E*)ket->cur, g.nwork, g.chunk, pauli_ins(g), d, partial);
        });
      },
      [&](const PauliGeom&, uint32_t id, const double* sum) {
        const uint32_t ny = terms[id].ny;  // times i^n_Y: exact
        const double re = sum[0], im = sum[1];
        values[2 * (size_t)id] = ny == 0 ? re : ny == 1 ? -im : ny == 2 ? -re : im;
        values[2 * (size_t)id + 1] = ny == 0 ? im : ny == 1 ? re : ny == 2 ? -im : -re;
      });
}

extern "C" int qipx_state_pauli_matrix_elements(qip_hip_state* bra, qip_hip_state* ket, const uint64_t* term_start,
                                                const uint64_t* qubits, const uint8_t* paulis, uint64_t count, double* values) try {
  STATE_ENTER_RAW(ket);
  QCHK(pair_meet("pauli_matrix_elements", ket, bra));
  if (count == 0) return QIP_OK;
  if (!values) return fail(QIP_ERR_INVALID, "pauli_matrix_elements: null result array");
  std::vector<PauliTerm> terms;
  QCHK(pauli_terms("pauli_matrix_elements", ket->n, term_start, qubits, paulis, count, &terms));
  QCHK(pair_settle(ket, bra));
  return ket->dtype == QIP_C64 ? pauli_melem_t<double>(ket, bra, terms, values) : pauli_melem_t<float>(ket, bra, terms, values);
} QIP_CATCH_ALL

// ---- vector arithmetic of resident states: dst <- sum_i c_i src_i and <bra_i|ket> (include/qip_hipx.h) -------------------
//   meet    every handle as the two-state calls above meet theirs (pair_meet, pair_settle), all refusals before anything is queued
//   launch  ONE k_lincomb / k_inner_many launch in a grid that depends on the number of 16-byte elements only (vec_grid), in the
//           smallest capacity of kVecCaps that holds the call
//   fold    per-block partials in the own state's reduction scratch, added on the host in block order
// Both calls are complete when they return.
static unsigned vec_grid(uint64_t nelems) { return (unsigned)std::min<uint64_t>(std::max<uint64_t>(nelems / (kBlock * 4), 1), 4096); }
// 16-byte elements of a state: one Complex<f64>, two Complex<f32> (n >= 1: never half an element)
static uint64_t vec_elems(const qip_hip_state* s) { return s->dtype == QIP_C64 ? s->namps : s->namps / 2; }

template <typename T, int G, bool NORM>
static void lincomb_launch_g(qip_hip_state* dst, const LincombDesc<T>& d, unsigned gx, uint64_t nelems) {
  using E = typename std::conditional<std::is_same<T, float>::value, f32x4, amp_t<T>>::type;
  hipLaunchKernelGGL((k_lincomb<T, G, NORM, E>), dim3(gx), dim3(kBlock), 0, dst->stream, (E*)dst->cur, nelems, d, dst->d_partial);
}

template <typename T, bool NORM>
static void lincomb_launch(qip_hip_state* dst, const LincombDesc<T>& d, unsigned gx, uint64_t nelems) {
  // the capacities: 1 to 4 sources each have their own (scale, axpy, the Lanczos update of three), then 8 and 16
  if (d.count <= 1) lincomb_launch_g<T, 1, NORM>(dst, d, gx, nelems);
  else if (d.count == 2) lincomb_launch_g<T, 2, NORM>(dst, d, gx, nelems);
  else if (d.count == 3) lincomb_launch_g<T, 3, NORM>(dst, d, gx, nelems);
  else if (d.count == 4) lincomb_launch_g<T, 4, NORM>(dst, d, gx, nelems);
  else if (d.count <= 8) lincomb_launch_g<T, 8, NORM>(dst, d, gx, nelems);
  else lincomb_launch_g<T, kVecMax, NORM>(dst, d, gx, nelems);
}

template <typename T>
static int lincomb_t(qip_hip_state* dst, qip_hip_state* const* srcs, const double* coeffs, uint32_t count, double* norm_sqr) {
  const uint64_t nelems = vec_elems(dst);
  const unsigned gx = vec_grid(nelems);
  LincombDesc<T> d;
  memset(&d, 0, sizeof d);
  d.count = count;
  for (uint32_t i = 0; i < count; ++i) {
    d.src[i] = srcs[i]->cur;
    d.cr[i] = (T)coeffs[2 * (size_t)i];
    d.ci[i] = (T)coeffs[2 * (size_t)i + 1];
  }
  if (norm_sqr) {
    QCHK(ensure_partial(dst, gx));
    lincomb_launch<T, true>(dst, d, gx, nelems);
  } else {
    lincomb_launch<T, false>(dst, d, gx, nelems);
  }
  HIPCHK(hipGetLastError());
  std::vector<double> part(norm_sqr ? gx : 0);
  if (norm_sqr) HIPCHK(hipMemcpyAsync(part.data(), dst->d_partial, gx * sizeof(double), hipMemcpyDeviceToHost, dst->stream));
  HIPCHK(hipStreamSynchronize(dst->stream));  // complete on return: the caller may change a source at once
  if (norm_sqr) {
    double t = 0;
    for (double v : part) t += v;
    *norm_sqr = t;
  }
  return QIP_OK;
}

extern "C" int qipx_state_linear_combination(qip_hip_state* dst, qip_hip_state* const* srcs, const double* coeffs, uint32_t count,
                                             double* norm_sqr) try {
  STATE_ENTER_RAW(dst);
  if (count > (uint32_t)kVecMax) return fail(QIP_ERR_UNSUPPORTED, "linear_combination: %u sources, at most %d are supported", count, kVecMax);
  if (count > 0 && (!srcs || !coeffs)) return fail(QIP_ERR_INVALID, "linear_combination: null source or coefficient array");
  for (uint32_t i = 0; i < count; ++i) QCHK(pair_meet("linear_combination", dst, srcs[i]));
  for (uint32_t i = 0; i < count; ++i)
    if (!std::isfinite(coeffs[2 * (size_t)i]) || !std::isfinite(coeffs[2 * (size_t)i + 1]))
      return fail(QIP_ERR_INVALID, "linear_combination: the coefficient of source %u is not finite", i);
  QCHK(pair_settle(dst, dst));
  for (uint32_t i = 0; i < count; ++i) QCHK(pair_settle(dst, srcs[i]));
  if (count == 0) {
    HIPCHK(hipMemsetAsync(dst->cur, 0, dst->namps * dst->amp_bytes, dst->stream));
    HIPCHK(hipStreamSynchronize(dst->stream));
    if (norm_sqr) *norm_sqr = 0.0;
    return QIP_OK;
  }
  return dst->dtype == QIP_C64 ? lincomb_t<double>(dst, srcs, coeffs, count, norm_sqr) : lincomb_t<float>(dst, srcs, coeffs, count, norm_sqr);
} QIP_CATCH_ALL

template <typename T, int G>
static void inner_launch_g(qip_hip_state* ket, const InnerDesc& d, unsigned gx, uint64_t nelems) {
  using E = typename std::conditional<std::is_same<T, float>::value, f32x4, amp_t<T>>::type;
  hipLaunchKernelGGL((k_inner_many<T, G, E>), dim3(gx), dim3(kBlock), 0, ket->stream, (const E*)ket->cur, nelems, d, ket->d_partial);
}

template <typename T>
static int inner_many_t(qip_hip_state* ket, qip_hip_state* const* bras, uint32_t count, double* values) {
  const uint64_t nelems = vec_elems(ket);
  const unsigned gx = vec_grid(nelems);
  InnerDesc d;
  memset(&d, 0, sizeof d);
  d.count = count;
  for (uint32_t i = 0; i < count; ++i) d.bra[i] = bras[i]->cur;
  const size_t need = 2 * (size_t)count * gx;
  QCHK(ensure_partial(ket, need));
  if (count <= 1) inner_launch_g<T, 1>(ket, d, gx, nelems);
  else if (count <= 2) inner_launch_g<T, 2>(ket, d, gx, nelems);
  else if (count <= 4) inner_launch_g<T, 4>(ket, d, gx, nelems);
  else if (count <= 8) inner_launch_g<T, 8>(ket, d, gx, nelems);
  else inner_launch_g<T, kVecMax>(ket, d, gx, nelems);
  HIPCHK(hipGetLastError());
  std::vector<double> part(need);
  HIPCHK(hipMemcpyAsync(part.data(), ket->d_partial, need * sizeof(double), hipMemcpyDeviceToHost, ket->stream));
  HIPCHK(hipStreamSynchronize(ket->stream));
  for (uint32_t i = 0; i < count; ++i) {
    double re = 0, im = 0;
    for (unsigned b = 0; b < gx; ++b) re += part[(size_t)(2 * i) * gx + b], im += part[(size_t)(2 * i + 1) * gx + b];
    values[2 * (size_t)i] = re, values[2 * (size_t)i + 1] = im;
  }
  return QIP_OK;
}

extern "C" int qipx_state_inner_products(qip_hip_state* const* bras, uint32_t count, qip_hip_state* ket, double* values) try {
  STATE_ENTER_RAW(ket);
  if (count == 0) return QIP_OK;
  if (count > (uint32_t)kVecMax) return fail(QIP_ERR_UNSUPPORTED, "inner_products: %u bras, at most %d are supported", count, kVecMax);
  if (!bras || !values) return fail(QIP_ERR_INVALID, "inner_products: null bra or result array");
  for (uint32_t i = 0; i < count; ++i) QCHK(pair_meet("inner_products", ket, bras[i]));
  for (uint32_t i = 0; i < count; ++i) QCHK(pair_settle(ket, bras[i]));
  return ket->dtype == QIP_C64 ? inner_many_t<double>(ket, bras, count, values) : inner_many_t<float>(ket, bras, count, values);
} QIP_CATCH_ALL
