#!/bin/bash
# VGPRs / SGPRs / scratch / waves per SIMD / LDS / code bytes of every kernel instantiation of one file (compile-only, no GPU needed):
#   tools/kernel_regs.sh ["[-Dflags] file.hip"] [kernel-name regex]     defaults: traverse.hip, k_traverse
#   tools/kernel_regs.sh scene_kernels.hip k_scene         tools/kernel_regs.sh "-DNRT_PROF=1 traverse.hip"
# One table of tools/resource_usage_diff.py (a build against itself); for two builds side by side use that tool directly.
here="$(cd "$(dirname "$0")" && pwd)"
cd "$here/../nanort_amd/csrc" || exit 1
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt \
  -fno-gpu-flush-denormals-to-zero --cuda-device-only -Rpass-analysis=kernel-resource-usage -S ${1:-traverse.hip} -o "$tmp/k.s" 2> "$tmp/k.log" ||
  { cat "$tmp/k.log"; exit 1; }
python3 "$here/resource_usage_diff.py" --kernels "${2:-k_traverse}" "$tmp/k.log,$tmp/k.s" "$tmp/k.log,$tmp/k.s"
