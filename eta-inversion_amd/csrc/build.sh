#!/bin/bash
# Build libetainv_hip.so for gfx950 in-tree (the .so is git-ignored but travels to the GPU box with gpurun).
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"
OUT="$HERE/../etainv/lib"
OBJ="$HERE/obj"; LIBNAME=libetainv_hip.so; SRCS="step_kernels ddpm regularize proximal metrics clip dino lpips igemm norm attention misc maps aux_nets f32path ppgemm ppconv"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result"
mkdir -p "$OUT" "$OBJ"
pids=()
for f in $SRCS; do
  if [ ! -f "$OBJ/$f.o" ] || [ "$HERE/$f.hip" -nt "$OBJ/$f.o" ] || [ "$HERE/common.h" -nt "$OBJ/$f.o" ] || [ "$HERE/kernels.h" -nt "$OBJ/$f.o" ] || [ "$HERE/self_attn_route.h" -nt "$OBJ/$f.o" ] || [ "$HERE/../../include/etainv.h" -nt "$OBJ/$f.o" ]; then
    EXTRA=""
    # attention: keep MFMA results in VGPRs (the softmax consumes them on the VALU: no v_accvgpr moves) and drop the
    # NaN-canonicalising v_max the compiler inserts in front of every fmaxf on MFMA outputs
    if [ "$f" = "attention" ]; then EXTRA="-mllvm -amdgpu-mfma-vgpr-form -fno-honor-nans"; fi
    hipcc $FLAGS $EXTRA -c "$HERE/$f.hip" -o "$OBJ/$f.o" &
    pids+=($!)
  fi
done
hipcc $FLAGS -x hip -c "$HERE/engine.cpp" -o "$OBJ/engine.o" &
pids+=($!)
hipcc $FLAGS -x hip -c "$HERE/ops_capi.cpp" -o "$OBJ/ops_capi.o" &
pids+=($!)
for p in "${pids[@]}"; do wait $p; done
objs=""; for f in $SRCS engine ops_capi; do objs="$objs $OBJ/$f.o"; done
hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT/$LIBNAME" $objs
echo "built $OUT/$LIBNAME"
# regularize.hip steers its register allocation (opaque copies of the thread index, scheduling fences every four slots: DESIGN 4.9b), which a
# compiler change can undo without any test failing.  Expected with these flags, noise_regularize_kernel<MAXQ, L0_LDS> at 1024 threads (128
# VGPRs available): <4, true> 48 VGPRs, <16, true> 120 VGPRs, <36, false> 128 VGPRs + 276 spilled dwords (580 B scratch); no spill in the first
# two.  RESOURCES=1 prints what this compiler gives (the lines to compare are "VGPRs:", "VGPRs Spill:", "ScratchSize").
# proximal.hip keeps up to 32 values per thread in registers through five passes.  Expected, prox_guidance_kernel<Q> at 1024 threads:
# <4> 46 VGPRs, <32> 110 VGPRs, <0> 42 VGPRs; no spill and no scratch in any of the three; 17,424 B of LDS each.
# metrics.hip: metrics_level_kernel<float / double> at 256 threads: 114 VGPRs, no scratch, 44,456 B of LDS (three blocks per CU).
# dino.hip at 256 threads: dino_selfsim_kernel<f16 / bf16> 58 VGPRs + 32 AGPRs (the two Gram tiles' accumulators), no scratch, 36,896 B of LDS
# (four 64 x 72 slabs: four blocks per CU); dino_selfsim_f32_kernel 86 VGPRs, no scratch, 33,824 B; dino_preprocess_kernel 19-21 VGPRs, no
# scratch, max_rows * R * 4 B of dynamic LDS (18,816 B for 512 -> 224 at patch 8); the row-norm, GELU and finalize kernels 8-12 VGPRs, no LDS.
# norm.hip at 256 threads: layerscale_add_layernorm_kernel<f16 / bf16> 60 VGPRs, <float> 59, layernorm_kernel 56; no scratch, no LDS, 8 waves per SIMD.
# lpips.hip at 256 threads: lpips_conv2d_kernel<T, cin == 4> 44-48 VGPRs + 32 AGPRs (the 2 x 4 accumulator tiles), no scratch, 15,360 B of LDS
# (16-bit: 192 rows of 40 elements) / 27,648 B (fp32: 192 rows of 36); maxpool3s2_kernel 38-48 VGPRs, lpips_distance_kernel 46-48 VGPRs and 32 B
# of LDS, lpips_preprocess_kernel 29-34 VGPRs; no scratch in any of them.
if [ "${RESOURCES:-0}" = "1" ]; then
  for f in regularize proximal metrics dino lpips norm; do
    hipcc $FLAGS --cuda-device-only -Rpass-analysis=kernel-resource-usage -c "$HERE/$f.hip" -o /dev/null 2>&1 | grep -E "Function Name|VGPRs|ScratchSize" || true
  done
fi
# diagnostic variant (STAMPS=1): igemm with in-kernel s_memtime stamps -> lib/libetainv_hip_stamps.so (load it with ETAINV_LIB=<path>;
# tools/experiments/*: reads SHARES of a K step, never a run time)
if [ "${STAMPS:-0}" = "1" ]; then
  hipcc $FLAGS -DETAINV_IGEMM_STAMPS -c "$HERE/igemm.hip" -o "$OBJ/igemm_stamps.o"
  hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT/libetainv_hip_stamps.so" ${objs/$OBJ\/igemm.o/$OBJ\/igemm_stamps.o}
  echo "built $OUT/libetainv_hip_stamps.so"
fi
# A/B variant of one kernel file (same-box comparisons; boxes of the pool differ by several percent):
#   VARIANT=name VARIANT_FILE=igemm VARIANT_FLAGS="-DETAINV_IGEMM_STAMPS" bash build.sh   ->  lib/libetainv_hip_name.so  (load with ETAINV_LIB)
if [ -n "${VARIANT:-}" ]; then
  vf="${VARIANT_FILE:-igemm}"
  EXTRA=""
  if [ "$vf" = "attention" ]; then EXTRA="-mllvm -amdgpu-mfma-vgpr-form -fno-honor-nans"; fi
  hipcc $FLAGS $EXTRA ${VARIANT_FLAGS:-} -c "$HERE/$vf.hip" -o "$OBJ/${vf}_$VARIANT.o"
  objs=""
  for f in $SRCS engine ops_capi; do
    if [ "$f" = "$vf" ]; then objs="$objs $OBJ/${vf}_$VARIANT.o"; else objs="$objs $OBJ/$f.o"; fi
  done
  hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT/libetainv_hip_$VARIANT.so" $objs
  echo "built $OUT/libetainv_hip_$VARIANT.so"
fi
