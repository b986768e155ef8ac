# A/B builds of libqip_hip.so that differ in compile-time switches of the interpreter's unit (qip_tile_interp.hip: k_tile_passes):
#   bash tools/build_variants.sh TAG "-DNAME=VALUE ..." [TAG "..." ...]   -> rustqip_amd/lib/libqip_hip_vTAG.so per pair
# run one with QIP_HIP_LIB=<path> (rustqip_amd/_ffi.py).  The objects of the other translation units are shared with the main build.
# (The switches of the diagonal-run loop this was written for, QIP_DIAG_PREFETCH / QIP_DIAG_ASM, are gone with the wire format: the
# loop fetches one block per item and waits once; profiles/entry_fetch.md.)
cd "$(dirname "$0")/../rustqip_amd" || exit 1
F="--offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -fPIC"
U="-mllvm -structurizecfg-skip-uniform-regions"  # the unit's own option (build.py, UNIT_FLAGS)
while [ $# -ge 2 ]; do
  tag=$1; defs=$2; shift 2
  ( /opt/rocm/bin/hipcc $F $U $defs -c csrc/qip_tile_interp.hip -o build/qip_tile_interp_v$tag.o &&
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -fPIC -shared -Wl,--version-script=csrc/exports.map -o lib/libqip_hip_v$tag.so \
      build/qip_core.o build/qip_launch.o build/qip_tile_sched.o build/qip_circuit.o build/qip_tile_interp_v$tag.o build/qip_jit.o build/qip_slice.o build/qip_host.o build/qip_measure.o build/qip_pauli.o build/qip_dist.o -ldl ) &
done
wait
ls -la lib/
