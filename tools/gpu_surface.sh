#!/bin/bash
# The cost-surface measurements of DESIGN.md: tools/gpu_surface.py with the product build and with the naive A/B build, then one
# rocprofv3 kernel-trace run of each for the kernels' own times. Build the variant first, on the build machine:
#   tools/build_variant.sh surfnaive "-DCFEAR_SURFACE_NAIVE=1"
# Results go to $CFEAR_OUT (default tools/_out/). Every GPU step has a time limit of its own; the first failure ends the script.
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${CFEAR_OUT:-$R/tools/_out}
NAIVE=$R/tools/_stop/libcfear_hip_surfnaive.so
mkdir -p "$OUT"
cd "$R" || exit 1
[ -f "$NAIVE" ] || { echo "missing $NAIVE"; exit 2; }
timeout -k 10 300 python tools/gpu_surface.py > "$OUT/surface_product.jsonl" 2> "$OUT/surface_product.err" || exit $?
CFEAR_SURF_REPS=2 CFEAR_HIP_LIB=$NAIVE timeout -k 10 300 python tools/gpu_surface.py > "$OUT/surface_naive.jsonl" 2> "$OUT/surface_naive.err" || exit $?
for v in product naive; do
  rm -rf /tmp/surf_kt_$v
  if [ $v = naive ]; then export CFEAR_HIP_LIB=$NAIVE; else unset CFEAR_HIP_LIB; fi
  CFEAR_SURF_REPS=2 timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/surf_kt_$v -o kt -- python "$R/tools/gpu_surface.py" > "$OUT/surface_rocprof_$v.log" 2>&1 || exit $?
  f=$(find /tmp/surf_kt_$v -name "*kernel_stats.csv" | head -1)
  [ -n "$f" ] && cp "$f" "$OUT/surface_kernel_stats_$v.csv"
  f=$(find /tmp/surf_kt_$v -name "*kernel_trace.csv" | head -1)
  [ -n "$f" ] && grep -i "surface" "$f" > "$OUT/surface_kernel_trace_$v.csv"
done
unset CFEAR_HIP_LIB
cat "$OUT/surface_product.jsonl" "$OUT/surface_naive.jsonl"
for v in product naive; do grep -i "surface" "$OUT/surface_kernel_stats_$v.csv" | cut -c1-220; done
