#!/bin/bash
# Per-kernel register use / spills / occupancy of pathtrace.hip (device-only compile, a few seconds).
# usage: tools/kernel_regs.sh [query.hip | occlusion.hip | hits.hip | nearest.hip | ambient.hip | radiance.hip | denoise.hip | display.hip] [extra hipcc flags]
# With a source name: every kernel of that file of csrc/ instead (rt_query_kernel / rt_occlusion_kernel / rt_ambient_kernel /
# rt_radiance_kernel instances as <mode, triangles, threads>, the latter also <..., kind>: 0 radiance,
# 1 gather, 2 probe, 3 lens; nearest.hip: rt_nearest_kernel instances as <mode, triangles, sweep, threads>; display.hip:
# rt_display_meter_kernel, rt_display_solve_kernel and rt_display_tone_kernel instances as <operator, encode>).
cd "$(dirname "$0")/.." || exit 1
src=pathtrace.hip
case "$1" in *.hip) src=$1; shift ;; esac
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math \
  -fhip-fp32-correctly-rounded-divide-sqrt -fno-gpu-flush-denormals-to-zero -fno-slp-vectorize \
  --cuda-device-only -c -o /dev/null -Iinclude -Irust_gpu_raytracing_amd/csrc "$@" \
  -Rpass-analysis=kernel-resource-usage rust_gpu_raytracing_amd/csrc/$src 2>&1 |
  grep -E "Function Name|VGPRs:|SGPRs Spill|VGPRs Spill|ScratchSize|Occupancy" |
  sed -E 's/.*remark: //' | paste - - - - - - |
  if [ "$src" = pathtrace.hip ]; then
    grep pathtrace_kernel |
    sed -E "s/ \[-Rpass-analysis=kernel-resource-usage\]//g; s/Function Name: _Z19rt_pathtrace_kernelIL(i[0-9])ELj([0-9]+)ELb([01])ELb([01])EEv10KernelArgs/mode \1 threads \2 tris \3 frame_par \4/; s/[[:space:]]+/ /g"
  else
    sed -E "s/ \[-Rpass-analysis=kernel-resource-usage\]//g; s/Function Name: _Z[0-9]+(rt_[a-z_]+)IL(i[0-9])ELb([01])ELj([0-9]+)EL8PathKind([0-3])EEv10KernelArgs[0-9A-Za-z]+/\1 mode \2 tris \3 threads \4 kind \5/; s/Function Name: _Z[0-9]+(rt_[a-z_]+)IL(i[0-9])ELb([01])ELj([0-9]+)EEv10KernelArgs[0-9A-Za-z]+/\1 mode \2 tris \3 threads \4/; s/Function Name: _Z[0-9]+(rt_[a-z_]+)IL(i[0-9])ELb([01])ELb([01])ELj([0-9]+)EEv10KernelArgs[0-9A-Za-z]+/\1 mode \2 tris \3 sweep \4 threads \5/"
  fi
