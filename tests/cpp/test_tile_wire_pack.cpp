// The interpreter's wire format (rustqip_amd/csrc/qip_tile_wire.h) as plain C++: pack descriptors with every field at its smallest
// and largest legal value, read them back through the accessors the kernel uses, compare field by field in both precisions, and
// check the pairing rule of run items on hand-made lists.  Built with -fsanitize=address,undefined by tests/test_tile_wire_pack_cpu.py.
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "qip_tile_wire.h"

using namespace qipk;

// the fields of TileGate<T> / TileDiagItem<T> (csrc/qip_kernels.h) that the packer reads
template <typename T> struct Amp { T x, y; };
template <typename T> struct Gate {
  uint32_t kind, b0, b1, cmask, nz, tpos_out;
  uint64_t omask;
  uint32_t op, cm_reg, cm_lane, pad_;
  Amp<T> m[4];
};
template <typename T> struct Item {
  Amp<T> f0, f1;
  uint64_t omask, oval;
  uint32_t lane_mask, lane_val, emask_sel, reg_pack;
};

// TileOp values (csrc/qip_kernels.h)
enum { DIAG_UNIFORM = 0, DIAG_LANE = 1, DIAG_LANE_CTL = 2, DIAG_REG0 = 3, DENSE0 = 6, DENSE_LANE0 = 9, DENSE2Q_01 = 12, SWAP_01 = 18, DENSE3Q_210 = 26, DIAG_RUN = 27 };
static const TileWireOps kOps = {DIAG_UNIFORM, DIAG_LANE, DIAG_LANE_CTL, DENSE0, DIAG_RUN};

static int failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      ++failures;                                                        \
      if (failures < 20) printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                                    \
  } while (0)

template <typename T> static bool same_bits(T a, T b) { return !memcmp(&a, &b, sizeof a); }
// the amplitude whose first word is word `at`, as the kernel's wire_amp reads it
template <typename T> static Amp<T> amp_at(const uint32_t* w, int at) {
  Amp<T> a;
  memcpy(&a.x, w + at, sizeof(T));
  memcpy(&a.y, w + at + sizeof(T) / 4, sizeof(T));
  return a;
}
template <typename T> static bool same_amp(Amp<T> a, Amp<T> b) { return same_bits(a.x, b.x) && same_bits(a.y, b.y); }

template <typename T> static std::vector<T> values() {
  return {(T)0, -(T)0, (T)1, (T)-1, (T)0.7071067811865476, std::numeric_limits<T>::max(), std::numeric_limits<T>::denorm_min(),
          -std::numeric_limits<T>::min(), std::numeric_limits<T>::infinity()};
}

template <typename T> static uint32_t expected_code(const Gate<T>& g) {
  if (g.op >= DENSE0 && g.op < DENSE0 + 3 && (g.b1 & 7u) == 5u && g.cm_reg == 0) return WOP_SIGNS0 + (g.op - DENSE0);
  if (g.op == DIAG_RUN) return WOP_RUN;
  if (g.op == DIAG_UNIFORM) return WOP_DIAG_UNIFORM;
  if (g.op == DIAG_LANE || g.op == DIAG_LANE_CTL) return WOP_DIAG_LANE;
  return kWireOther + g.op;
}

template <typename T> static void gates() {
  using WW = TileWireWords<T>;
  const std::vector<T> vals = values<T>();
  const uint32_t ops[] = {DIAG_UNIFORM, DIAG_LANE, DIAG_LANE_CTL, DIAG_REG0, DIAG_REG0 + 2, DENSE0, DENSE0 + 1, DENSE0 + 2, DENSE_LANE0,
                          DENSE2Q_01, SWAP_01, DENSE3Q_210, DIAG_RUN};
  const uint32_t b0s[] = {0u, kWireTileBits - 1u, 0xffffffffu};
  // b1: flags of a dense gate (real, X, sign rows and the two signs), a tile bit, a run's item count at its largest
  const uint32_t b1s[] = {0u, 1u, 2u, 5u, 13u, 21u, 29u, 4u, kWireTileBits - 1u, kWireMaxGates * kWireItemsPerGate};
  const uint32_t nzs[] = {0u, 15u, kWireMaxGates * kWireItemsPerGate - 1u};
  const uint32_t tps[] = {0u, kWireMaxPos - 1u};
  const uint32_t cms[] = {0u, 1u, (1u << kWireTileBits) - 1u};
  const uint64_t oms[] = {0ull, 1ull << 11, 1ull << 63, ~0ull};
  size_t vi = 0, n = 0;
  for (uint32_t op : ops)
    for (uint32_t b0 : b0s)
      for (uint32_t b1 : b1s)
        for (uint32_t nz : nzs)
          for (uint32_t tp : tps)
            for (uint32_t cr : cms)
              for (uint32_t cl : cms)
                for (uint64_t om : oms) {
                  Gate<T> g;
                  memset(&g, 0xa5, sizeof g);  // whatever the packer does not read must not matter
                  g.op = op, g.b0 = b0, g.b1 = b1, g.nz = nz, g.tpos_out = tp, g.cm_reg = cr, g.cm_lane = cl, g.omask = om;
                  for (int k = 0; k < 4; ++k) g.m[k].x = vals[vi++ % vals.size()], g.m[k].y = vals[vi++ % vals.size()];
                  TileWireGate<T> wg;
                  memset(&wg, 0x5a, sizeof wg);
                  CHECK((wire_pack_gate<T>(g, kOps, &wg)));
                  uint32_t w[sizeof wg / 4];
                  memcpy(w, &wg, sizeof wg);
                  CHECK(w[kWireWCode] == expected_code(g));
                  CHECK(w[kWireWB1] == b1 && w[kWireWNz] == nz);
                  CHECK(wire_cm_reg(w[kWireWCm]) == cr);
                  CHECK(wire_cm_lane(w[kWireWCm]) == (op == DIAG_LANE ? 0u : cl));  // TOP_DIAG_LANE reads no lane control
                  CHECK(wire_b0(w[kWireWBits]) == (b0 == 0xffffffffu ? kWireOutside : b0));
                  CHECK(wire_tpos_out(w[kWireWBits]) == tp);
                  uint64_t om_back;
                  memcpy(&om_back, w + kWireWOmask, 8);
                  CHECK(om_back == om);
                  CHECK(same_amp(amp_at<T>(w, WW::m0), g.m[0]) && same_amp(amp_at<T>(w, WW::m1), g.m[1]));
                  CHECK(same_amp(amp_at<T>(w, WW::m2), g.m[2]) && same_amp(amp_at<T>(w, WW::m3), g.m[3]));
                  CHECK(WW::m1 + WW::amp <= 16);  // everything but the second row: the first 64-byte block
                  ++n;
                }
  // what does not fit is refused, not truncated
  Gate<T> g;
  memset(&g, 0, sizeof g);
  TileWireGate<T> wg;
  g.b0 = kWireOutside;  // (a tile bit index that would read as "outside")
  CHECK(!(wire_pack_gate<T>(g, kOps, &wg)));
  g.b0 = 0, g.cm_reg = 0x10000u;
  CHECK(!(wire_pack_gate<T>(g, kOps, &wg)));
  g.cm_reg = 0, g.cm_lane = 0x10000u;
  CHECK(!(wire_pack_gate<T>(g, kOps, &wg)));
  printf("gates<%s>: %zu descriptors\n", sizeof(T) == 8 ? "double" : "float", n);
}

// the form of a mask, worked out from the elements: J and half of a mask that is exactly one half by one pass bit
static uint32_t form_by_elements(uint32_t emask) {
  if (emask == 0xffu) return WF_ALL;
  for (uint32_t j = 0; j < 3; ++j)
    for (uint32_t half = 0; half < 2; ++half) {
      uint32_t m = 0;
      for (uint32_t i = 0; i < 8; ++i)
        if (((i >> j) & 1u) == half) m |= 1u << i;
      if (m == emask) return WF_LO0 + 2u * j + half;
    }
  return WF_MASK;
}

template <typename T> static Item<T> item(uint32_t emask, uint32_t sel, T tag) {
  Item<T> it;
  memset(&it, 0, sizeof it);
  it.f0 = {tag, (T)(tag + 1)};
  it.f1 = {(T)(tag + 2), (T)(tag + 3)};
  it.emask_sel = emask | (sel << 24);
  it.reg_pack = 0xdeadbeefu;  // (the packer does not read it)
  return it;
}

template <typename T> static void items() {
  using WW = TileWireWords<T>;
  const uint32_t lanes[] = {0u, 1u, (1u << kWireTileBits) - 1u};
  const uint64_t outs[] = {0ull, 1ull << 63, ~0ull};
  const uint32_t sels[] = {0u, 1u, kWireTileBits};
  size_t n = 0;
  for (uint32_t emask = 0; emask < 256; ++emask)
    for (uint32_t sel : sels)
      for (uint32_t lm : lanes)
        for (uint64_t om : outs) {
          Item<T> it = item<T>(emask, sel, (T)emask);
          it.lane_mask = lm, it.lane_val = lm & 0x555u, it.omask = om, it.oval = om & 0xaaaaaaaaaaaaaaaaull;
          TileWireItem<T> wi[1];
          CHECK((wire_pack_items<T>(&it, 1, wi)) == 1);
          uint32_t w[16];
          memcpy(w, wi, 64);
          CHECK(wire_emask(w[WW::ctl]) == emask && wire_sel(w[WW::ctl]) == sel);
          CHECK(wire_form(w[WW::ctl]) == form_by_elements(emask));
          CHECK(wire_lane_mask(w[WW::lane]) == lm && wire_lane_val(w[WW::lane]) == (lm & 0x555u));
          uint64_t a, b;
          memcpy(&a, w + WW::omask, 8);
          memcpy(&b, w + WW::oval, 8);
          CHECK(a == it.omask && b == it.oval);
          CHECK(same_amp(amp_at<T>(w, WW::f0), it.f0) && same_amp(amp_at<T>(w, WW::f1), it.f1));
          CHECK(WW::ctl < 16);
          ++n;
        }
  Item<T> bad = item<T>(0xff, 0, (T)1);
  bad.lane_mask = 0x10000u;
  TileWireItem<T> tmp[4];
  CHECK((wire_pack_items<T>(&bad, 1, tmp)) == -1);

  // pairing: halves by pass bit J, low first (the order tile_merge_diag_runs emits) and high first
  const uint32_t lo[3] = {0x55u, 0x33u, 0x0fu};
  for (uint32_t j = 0; j < 3; ++j)
    for (int hi_first = 0; hi_first < 2; ++hi_first) {
      Item<T> two[2] = {item<T>(hi_first ? lo[j] ^ 0xffu : lo[j], 0, (T)10), item<T>(hi_first ? lo[j] : lo[j] ^ 0xffu, 0, (T)20)};
      for (Item<T>& t : two) t.lane_mask = 6, t.lane_val = 2, t.omask = 1ull << 40, t.oval = 1ull << 40;
      TileWireItem<T> out[2];
      CHECK((wire_pack_items<T>(two, 2, out)) == 1);
      uint32_t w[16];
      memcpy(w, out, 64);
      CHECK(wire_form(w[WW::ctl]) == WF_BOTH0 + j && wire_sel(w[WW::ctl]) == 0);
      const Item<T>& l = two[hi_first ? 1 : 0];
      const Item<T>& h = two[hi_first ? 0 : 1];
      CHECK(same_amp(amp_at<T>(w, WW::f0), l.f1) && same_amp(amp_at<T>(w, WW::f1), h.f1));  // an item without selector multiplies by f1
      CHECK(wire_lane_mask(w[WW::lane]) == 6 && wire_lane_val(w[WW::lane]) == 2);
      // ... and nothing pairs when one condition differs, the second item has a selector, or the halves belong to different bits
      for (int what = 0; what < 6; ++what) {
        Item<T> v[2] = {two[0], two[1]};
        if (what == 0) v[1].omask |= 1;
        if (what == 1) v[1].oval = 0;
        if (what == 2) v[1].lane_mask = 7;
        if (what == 3) v[1].lane_val = 4;
        if (what == 4) v[1].emask_sel |= 3u << 24;
        if (what == 5) v[1].emask_sel = lo[(j + 1) % 3];
        CHECK((wire_pack_items<T>(v, 2, out)) == 2);
        memcpy(w, out, 64);
        CHECK(wire_form(w[WW::ctl]) == form_by_elements(two[0].emask_sel & 0xffu));
        memcpy(w, out + 1, 64);
        CHECK(wire_emask(w[WW::ctl]) == (v[1].emask_sel & 0xffu));
      }
    }
  // low, high, low: the first two pair, the third stays alone; a full mask between two halves keeps them apart
  {
    Item<T> three[3] = {item<T>(0x33, 0, (T)1), item<T>(0xcc, 0, (T)2), item<T>(0x33, 0, (T)3)};
    TileWireItem<T> out[3];
    CHECK((wire_pack_items<T>(three, 3, out)) == 2);
    uint32_t w[16];
    memcpy(w, out, 64);
    CHECK(wire_form(w[WW::ctl]) == WF_BOTH1);
    memcpy(w, out + 1, 64);
    CHECK(wire_form(w[WW::ctl]) == WF_LO1 && same_amp(amp_at<T>(w, WW::f1), three[2].f1));
    Item<T> apart[3] = {item<T>(0x0f, 0, (T)1), item<T>(0xff, 0, (T)2), item<T>(0xf0, 0, (T)3)};
    CHECK((wire_pack_items<T>(apart, 3, out)) == 3);
  }
  CHECK((wire_pack_items<T>((const Item<T>*)nullptr, 0, tmp)) == 0);
  printf("items<%s>: %zu single items\n", sizeof(T) == 8 ? "double" : "float", n);
}

int main() {
  gates<double>();
  gates<float>();
  items<double>();
  items<float>();
  if (failures) {
    printf("FAILED: %d checks\n", failures);
    return 1;
  }
  printf("wire pack ok\n");
  return 0;
}
