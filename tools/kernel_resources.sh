#!/bin/bash
# SGPR / VGPR / AGPR / scratch / occupancy / LDS of every kernel (compiler remarks, cross-compiled for gfx950: no GPU needed).
# usage: kernel_resources.sh <repo root>                    - every kernel of the default units, one line each
#        kernel_resources.sh <repo root> <parent root>      - the same kernels of two trees side by side (parent | this tree), a '*' in front of the
#                                                             rows that differ:  tools/kernel_resources.sh . ../parent > profiles/seq_k_kernel_resources.txt
# CFEAR_KR_UNITS: the translation units (default: pipeline replay register_step register_step_large kstrongest cfar drift)
set -o pipefail
UNITS=${CFEAR_KR_UNITS:-"pipeline replay register_step register_step_large kstrongest cfar drift"}
OUT=$(mktemp -d)
trap 'rm -rf "$OUT"' EXIT
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}

# $1 tree, $2 unit -> "kernel SGPRs VGPRs AGPRs Scratch Occ LDS" per kernel
resources() {
  $HIPCC --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -c --cuda-device-only -Rpass-analysis=kernel-resource-usage \
    "$1/cfear_radarodometry_code_public_amd/csrc/$2.hip" -I"$1/include" -o "$OUT/kr.o" 2>&1 |
    grep -E "Function Name|TotalSGPRs:|VGPRs:|AGPRs:|ScratchSize|Occupancy|LDS Size" | grep -v "VGPRs/" |
    sed -e 's/.*remark: *//' -e 's/\[-Rpass.*//' -e 's/Function Name: *//' -e 's/ScratchSize \[bytes\/lane\]/Scratch/' -e 's/Occupancy \[waves\/SIMD\]/Occ/' \
        -e 's/LDS Size \[bytes\/block\]/LDS/' -e 's/: */:/' -e 's/ *$//' | paste -d' ' - - - - - - -
}

echo "# SGPRs / VGPRs / AGPRs / scratch (bytes per lane) / occupancy (waves per SIMD) / LDS (bytes per workgroup) of every kernel, cross-compiled for gfx950"
echo "# (hipcc -O3 -ffp-contract=off, -Rpass-analysis=kernel-resource-usage)"
if [ -z "$2" ]; then
  for f in $UNITS; do echo "== $f.hip"; resources "$1" $f; done
  exit 0
fi
echo "# per kernel: the parent tree | this tree; '*' marks a kernel whose figures differ"
for f in $UNITS; do
  echo "== $f.hip"
  resources "$2" $f > "$OUT/parent.txt"
  resources "$1" $f > "$OUT/branch.txt"
  awk 'NR == FNR { k = $1; $1 = ""; p[k] = $0; next }
       { k = $1; $1 = ""; printf "%s %s\n    %s\n    %s\n", (p[k] == $0 ? " " : "*"), k, (k in p ? p[k] : " (not in the parent)"), $0 }' "$OUT/parent.txt" "$OUT/branch.txt"
done
