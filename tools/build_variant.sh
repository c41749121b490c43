#!/bin/bash
# Another build of the engine for kernel A/B experiments: tools/build_variant.sh NAME "-DFLAG=..." -> sbr_rs_amd/libsbr_hip_NAME.so
# (select it with SBR_HIP_LIB=$PWD/sbr_rs_amd/libsbr_hip_NAME.so; git-ignored like every built artefact).
# The source list is sbr_rs_amd/build.py's SOURCES, so that it cannot drift from the library's own build.
set -e
name=$1; flags=$2
root=$(cd "$(dirname "$0")/.." && pwd)
out=$root/build/variant_$name; mkdir -p "$out"
sources=$(cd "$root" && python -c "from sbr_rs_amd.build import SOURCES; print(' '.join(SOURCES))")
pids=()
for src in $sources; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wno-unused-function -Wno-unused-result \
    -Wno-unused-value $flags -c "$root/sbr_rs_amd/csrc/$src" -o "$out/${src%.hip}.o" &
  pids+=($!)
done
for p in "${pids[@]}"; do wait "$p"; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -pthread -o "$root/sbr_rs_amd/libsbr_hip_$name.so" "$out"/*.o -ldl
echo "$root/sbr_rs_amd/libsbr_hip_$name.so"
