// qip_tile_wire.h — the device-side wire format of the interpreter kernel's lists (k_tile_passes, qip_kernels.h), and the host
// function that packs the host lists (TileGate<T>, TileDiagItem<T>) into it at the point where they are copied to the device.
//
// Why a second format: the sweep is latency-bound per wave, and what a wave waits for between two gates is scalar memory.  Read
// field by field from a TileGate<T> (0x70 bytes, the fields of one code path spread over all of it) the compiler issues the loads
// where each is first needed — `omask`, wait, branch; op / flags / masks, wait, a compare tree; the matrix, wait — two to three
// serialised round trips in front of 32 - 48 vector instructions.  Here everything a path needs before its first product sits in
// ONE naturally aligned 64-byte block that the kernel fetches with one load and waits for once.
//
// Plain C++ as well as HIP: the packer and the accessors compile without the HIP headers (tests/test_tile_wire_pack_cpu.py builds
// them into a stand-alone program), so the source lists are template parameters: anything with TileGate's / TileDiagItem's fields.
// Host lists, plans and everything exported from them are untouched: only interpreter launches see this format.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define QIP_WIRE_HD __host__ __device__ __forceinline__
#else
#define QIP_WIRE_HD inline
#endif

namespace qipk {

// The bounds the narrow fields rely on (checked against the kernel's own constants where both headers are seen: qip_kernels.h).
constexpr uint32_t kWireTileBits = 11;     // tile-index bits: masks over them fit 16 bits, bit indices fit 8
constexpr uint32_t kWireMaxPos = 64;       // amplitude-index positions
constexpr uint32_t kWireMaxGates = 256;    // gates per launch
constexpr uint32_t kWireItemsPerGate = 8;  // run items a gate can become (a 3-qubit diagonal: one per table entry)
constexpr uint32_t kWireOutside = 0xffu;   // TileGate::b0 == kTileOutside (0xffffffff) in 8 bits: no tile bit has that index
static_assert(kWireTileBits <= 16, "cm_reg, cm_lane, lane_mask, lane_val: 16 bits each");
static_assert(kWireTileBits < kWireOutside && kWireMaxPos <= 256, "b0 (or the outside mark) and tpos_out: 8 bits each");
static_assert(kWireMaxGates * kWireItemsPerGate < (1u << 24), "a run's first item and item count: below the form byte");

// Dispatch codes: the paths of an H / X / Rz circuit first, so that they resolve in the first compares; everything else keeps its
// TileOp value behind kWireOther.  (TOP_* values themselves do not move: plans and exports carry those.)
enum TileWireOp : uint32_t {
  WOP_SIGNS0 = 0, WOP_SIGNS1, WOP_SIGNS2,  // dense 1-qubit, real sign-symmetric rows, no pass-bit control, on pass bit J
  WOP_RUN,                                 // TOP_DIAG_RUN
  WOP_DIAG_UNIFORM,                        // TOP_DIAG_UNIFORM
  WOP_DIAG_LANE,                           // TOP_DIAG_LANE and TOP_DIAG_LANE_CTL (cm_lane = 0 without lane controls)
  kWireOther = 8,                          // kWireOther + TileOp: the general switch
};

// Element forms of a run item: which of the lane's eight elements take the factor, as straight-line code where the mask is regular.
enum TileWireForm : uint32_t {
  WF_MASK = 0,                             // any mask: one test per element
  WF_ALL,                                  // all eight
  WF_LO0, WF_HI0, WF_LO1, WF_HI1, WF_LO2, WF_HI2,  // the half with pass bit J = 0 / 1
  WF_BOTH0, WF_BOTH1, WF_BOTH2,            // two items in one: f0 on the half with pass bit J = 0, f1 on the other
};

template <typename T> struct TileWireGate;
// Complex<f64>: block 0 = everything but the second matrix row; block 1 = m[2], m[3] (read by the generic dense paths only)
template <> struct alignas(64) TileWireGate<double> {
  uint32_t code, b1, nz, cm, bits, pad_;
  uint64_t omask;
  double m01[4];
  double m23[4];
  uint32_t pad1_[8];
};
// Complex<f32>: one block
template <> struct alignas(64) TileWireGate<float> {
  uint32_t code, b1, nz, cm, bits, pad_;
  uint64_t omask;
  float m01[4];
  float m23[4];
};
static_assert(sizeof(TileWireGate<double>) == 128 && sizeof(TileWireGate<float>) == 64, "one / two 64-byte blocks");

template <typename T> struct alignas(64) TileWireItem {
  T f0[2], f1[2];
  uint64_t omask, oval;
  uint32_t lane;  // lane_mask | lane_val << 16
  uint32_t ctl;   // emask | form << 8 | (sel bit + 1) << 16
};
static_assert(sizeof(TileWireItem<double>) == 64 && sizeof(TileWireItem<float>) == 64, "one 64-byte block per run item");

// ---- accessors: the kernel and the tests read the words through these, and only these -----------------------------------------
// (`w` = the block's 16 words as loaded; the words of 64-bit fields are little-endian pairs)
constexpr int kWireWCode = 0, kWireWB1 = 1, kWireWNz = 2, kWireWCm = 3, kWireWBits = 4, kWireWOmask = 6, kWireWM = 8;
QIP_WIRE_HD uint32_t wire_cm_reg(uint32_t cm) { return cm & 0xffffu; }
QIP_WIRE_HD uint32_t wire_cm_lane(uint32_t cm) { return cm >> 16; }
QIP_WIRE_HD uint32_t wire_b0(uint32_t bits) { return bits & 0xffu; }  // kWireOutside: outside the tile
QIP_WIRE_HD uint32_t wire_tpos_out(uint32_t bits) { return bits >> 8; }
// word index of m[k] in a gate's blocks (Complex<f64>: m[2], m[3] are words 0 and 4 of block 1 = 16 and 20), and of an item's fields
template <typename T> struct TileWireWords {
  static constexpr int amp = (int)sizeof(T) / 2;  // words per amplitude
  static constexpr int m0 = kWireWM, m1 = kWireWM + amp, m2 = kWireWM + 2 * amp, m3 = kWireWM + 3 * amp;
  static constexpr int f0 = 0, f1 = amp, omask = 2 * amp, oval = 2 * amp + 2, lane = 2 * amp + 4, ctl = 2 * amp + 5;
};
QIP_WIRE_HD uint32_t wire_lane_mask(uint32_t lane) { return lane & 0xffffu; }
QIP_WIRE_HD uint32_t wire_lane_val(uint32_t lane) { return lane >> 16; }
QIP_WIRE_HD uint32_t wire_emask(uint32_t ctl) { return ctl & 0xffu; }
QIP_WIRE_HD uint32_t wire_form(uint32_t ctl) { return (ctl >> 8) & 0xffu; }
QIP_WIRE_HD uint32_t wire_sel(uint32_t ctl) { return ctl >> 16; }  // lane-bit index of the selecting target + 1, 0 = none

// ---- the packer (host) ---------------------------------------------------------------------------------------------------------
// G: TileGate<T>'s fields (op, b0, b1, nz, tpos_out, omask, cm_reg, cm_lane, m[4] with .x / .y).  kTileSignRows = 4, X = 2,
// real = 1 in b1 of a dense 1-qubit gate; TOP_* values as arguments so that this header needs no other.
struct TileWireOps {
  uint32_t diag_uniform, diag_lane, diag_lane_ctl, dense0, diag_run;  // TOP_DIAG_UNIFORM, _LANE, _LANE_CTL, TOP_DENSE0, TOP_DIAG_RUN
};
// false: a field does not fit (never for lists the scheduler builds: the static_asserts above and in qip_kernels.h)
template <typename T, typename G> inline bool wire_pack_gate(const G& g, const TileWireOps& ops, TileWireGate<T>* w) {
  *w = TileWireGate<T>();
  const bool outside = g.b0 == 0xffffffffu;
  if ((!outside && g.b0 >= kWireOutside) || g.tpos_out >= (1u << 24) || g.cm_reg > 0xffffu || g.cm_lane > 0xffffu) return false;
  uint32_t code = kWireOther + g.op;
  if (g.op >= ops.dense0 && g.op < ops.dense0 + 3u && (g.b1 & 2u) == 0u && (g.b1 & 1u) != 0u && (g.b1 & 4u) != 0u && g.cm_reg == 0u)
    code = WOP_SIGNS0 + (g.op - ops.dense0);
  else if (g.op == ops.diag_run) code = WOP_RUN;
  else if (g.op == ops.diag_uniform) code = WOP_DIAG_UNIFORM;
  else if (g.op == ops.diag_lane || g.op == ops.diag_lane_ctl) code = WOP_DIAG_LANE;
  w->code = code;
  w->b1 = g.b1;
  w->nz = g.nz;
  // (TOP_DIAG_LANE reads no lane control: whatever cm_lane holds there must not reach the shared path)
  w->cm = g.cm_reg | ((g.op == ops.diag_lane ? 0u : g.cm_lane) << 16);
  w->bits = (outside ? kWireOutside : g.b0) | (g.tpos_out << 8);
  w->omask = g.omask;
  for (int k = 0; k < 2; ++k) {
    w->m01[2 * k] = g.m[k].x;
    w->m01[2 * k + 1] = g.m[k].y;
    w->m23[2 * k] = g.m[2 + k].x;
    w->m23[2 * k + 1] = g.m[2 + k].y;
  }
  return true;
}

// the form of an element mask alone (no pairing)
inline uint32_t wire_form_of(uint32_t emask) {
  static const uint32_t lo[3] = {0x55u, 0x33u, 0x0fu};
  if (emask == 0xffu) return WF_ALL;
  for (uint32_t j = 0; j < 3; ++j) {
    if (emask == lo[j]) return WF_LO0 + 2u * j;
    if (emask == (lo[j] ^ 0xffu)) return WF_HI0 + 2u * j;
  }
  return WF_MASK;
}

// I: TileDiagItem<T>'s fields (f0, f1 with .x / .y, omask, oval, lane_mask, lane_val, emask_sel).  Packs items[0 .. count) of ONE
// gate list entry (a run) behind `out` and returns how many wire items that made: two consecutive items with complementary half
// masks on one pass bit, no selector, and equal outside / lane conditions become one WF_BOTH item — the two entries of an Rz on a
// pass bit.  Each element still meets exactly the product it met before: the halves are disjoint, so the order between the two
// items never mattered.  Returns -1 if a field does not fit.
template <typename T, typename I> inline long wire_pack_items(const I* items, uint32_t count, TileWireItem<T>* out) {
  long n = 0;
  for (uint32_t k = 0; k < count; ++k) {
    const I& a = items[k];
    const uint32_t emask = a.emask_sel & 0xffu, sel = a.emask_sel >> 24;
    if (a.lane_mask > 0xffffu || a.lane_val > 0xffffu || (a.emask_sel & 0x00ffff00u) != 0u) return -1;
    TileWireItem<T> w = TileWireItem<T>();
    w.f0[0] = a.f0.x, w.f0[1] = a.f0.y, w.f1[0] = a.f1.x, w.f1[1] = a.f1.y;
    w.omask = a.omask;
    w.oval = a.oval;
    w.lane = a.lane_mask | (a.lane_val << 16);
    uint32_t form = wire_form_of(emask);
    if (sel == 0u && form >= WF_LO0 && form <= WF_HI2 && k + 1 < count) {
      const I& b = items[k + 1];
      const bool lo_first = ((form - WF_LO0) & 1u) == 0u;
      if ((b.emask_sel >> 24) == 0u && (b.emask_sel & 0xffu) == (emask ^ 0xffu) && b.omask == a.omask && b.oval == a.oval &&
          b.lane_mask == a.lane_mask && b.lane_val == a.lane_val) {
        // without a selector an item's factor is f1: the low half's goes to f0, the high half's to f1
        const I& lo = lo_first ? a : b;
        const I& hi = lo_first ? b : a;
        w.f0[0] = lo.f1.x, w.f0[1] = lo.f1.y, w.f1[0] = hi.f1.x, w.f1[1] = hi.f1.y;
        form = WF_BOTH0 + (form - WF_LO0) / 2u;
        ++k;
      }
    }
    w.ctl = (form == WF_BOTH0 || form == WF_BOTH1 || form == WF_BOTH2 ? 0xffu : emask) | (form << 8) | (sel << 16);
    out[n++] = w;
  }
  return n;
}

}  // namespace qipk
