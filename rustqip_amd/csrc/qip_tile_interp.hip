// qip_tile_interp.hip — the interpreter's tile-sweep kernel (k_tile_passes, qip_kernels.h) and nothing else: the unit is compiled
// with an option of its own (rustqip_amd/build.py, UNIT_FLAGS), which must not reach any other kernel.
//
// Every branch of k_tile_passes is wave-uniform (the gate descriptors are scalar loads; per-lane conditions are selects).  hipcc's
// default pipeline still runs the control-flow structurizer over the gate loop, and the "flow" blocks it inserts carry the lane's
// eight amplitudes through PHIs with undefined inputs that the register coalescer cannot join: the amplitudes then live in two
// register sets and are copied between them at the loop latch and at the entry of the diagonal-run loop (16 + up to 48 v_mov_b64
// per gate, a third of the vector issue slots of a Hadamard / Rz circuit).  With uniform regions left unstructured the loop keeps
// the scalar branches it was written with and one register set (profiles/gate_loop_copies.md).
#include "qip_tile.h"

template <typename T>
void launch_tile_passes(hipStream_t stream, dim3 grid, size_t lds, bool nt, amp_t<T>* st, const Ins& ins, const TilePassDesc& pd,
                        const TileWireGate<T>* gates, const amp_t<T>* mats, amp_t<T>* out, const TileStorePerm* fold,
                        const TileWireItem<T>* items) {
  if (fold) {
#define TPF(NTV) hipLaunchKernelGGL((k_tile_passes<T, NTV, true>), grid, dim3(kTileBlock), lds, stream, st, ins, pd, gates, mats, out, *fold, items)
    if (nt) TPF(true);
    else TPF(false);
#undef TPF
  } else {
#define TP(NTV) hipLaunchKernelGGL((k_tile_passes<T, NTV>), grid, dim3(kTileBlock), lds, stream, st, ins, pd, gates, mats, (amp_t<T>*)nullptr, TileStorePerm(), items)
    if (nt) TP(true);
    else TP(false);
#undef TP
  }
}
template void launch_tile_passes<double>(hipStream_t, dim3, size_t, bool, amp_t<double>*, const Ins&, const TilePassDesc&, const TileWireGate<double>*,
                                         const amp_t<double>*, amp_t<double>*, const TileStorePerm*, const TileWireItem<double>*);
template void launch_tile_passes<float>(hipStream_t, dim3, size_t, bool, amp_t<float>*, const Ins&, const TilePassDesc&, const TileWireGate<float>*,
                                        const amp_t<float>*, amp_t<float>*, const TileStorePerm*, const TileWireItem<float>*);
