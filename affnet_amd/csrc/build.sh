#!/bin/bash
# Builds libaffnet_hip.so for gfx950 in-tree (affnet_amd/libaffnet_hip.so): product kernels + the stamped debug instantiations only, one object
# per source of FILES in obj/.
# AFFNET_PROBES=1: builds affnet_amd/libaffnet_hip_probes.so instead - the product objects of obj/ (brought up to date, not compiled a second
# time) plus PROBE_FILES, the probe kernels of the tuning / measurement tools (include/affnet_hip_probes.h), in obj_probes/.
# An object whose source is no longer in its directory's list is deleted: tools/kernel_resources.py reads every object of obj/.
# -ffp-contract=off: the detector / sampler reproduce the reference's fp32 operation sequence
# exactly; fused multiply-adds appear only where written as fmaf().
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wno-unused-function $EXTRA_HIPCC_FLAGS"
FILES="config_fill context pyramid detect laf_ops weights_pack cnn32 derive_u cnn_trunk_affnet cnn_trunk_affnet_poly cnn_trunk_orinet cnn_trunk_hardnet cnn_trunk_hardnet_poly cnn_trunk_hardnet_f43 cnn_trunk_hardnet_c5 cnn_trunk_hardnet_c1 hardnet_conv5_f43 cnn_heads pipeline match knn knn_q8 ivf spatial epipolar epipolar_planar guided ratio_match handcrafted sift tfeat fullconv"
PROBE_FILES="debug split_probe cnn_probe"
pids=()
objs=""

# compile_into DIR FILE...: start a compile of every stale object of DIR, drop the objects of other sources, append DIR's objects to $objs
compile_into() {
  local dir="$1" f o dep stale
  shift
  mkdir -p "$dir"
  for o in "$dir"/*.o; do
    [ -f "$o" ] || continue
    f="$(basename "$o" .o)"
    case " $* " in *" $f "*) ;; *) rm -f "$o" ;; esac
  done
  for f in "$@"; do
    stale=0      # no object yet, or the source or ANY header (internal or public) is newer than it
    for dep in "$HERE/$f.hip" "$HERE"/*.h "$HERE"/../../include/*.h; do
      if [ ! -f "$dir/$f.o" ] || [ "$dep" -nt "$dir/$f.o" ]; then stale=1; break; fi
    done
    if [ $stale = 1 ]; then
      $HIPCC $FLAGS -c "$HERE/$f.hip" -o "$dir/$f.o" &
      pids+=($!)
    fi
    objs="$objs $dir/$f.o"
  done
}

OUT="$HERE/../libaffnet_hip.so"
compile_into "$HERE/obj" $FILES
if [ "$AFFNET_PROBES" = "1" ]; then
  compile_into "$HERE/obj_probes" $PROBE_FILES
  OUT="$HERE/../libaffnet_hip_probes.so"
fi
for p in "${pids[@]}"; do wait $p; done
$HIPCC --offload-arch=gfx950 -shared -fPIC -Wl,--no-undefined -o "$OUT" $objs
echo "built $OUT"
