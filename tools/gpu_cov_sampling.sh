#!/bin/bash
# The cost-sampling measurements of DESIGN.md (estimate_cov_by_sampling on the batched step): tools/gpu_cov_sampling.py with the product build and with
# the naive A/B build (every sample a get_cost_block through the registration's general path), then one rocprofv3 kernel-trace run of each for the
# sampling kernel's own time. Build the variant first, on the build machine:
#   tools/build_variant.sh naive "-DCFEAR_COV_SAMPLING_NAIVE=1"
# Results go to $CFEAR_OUT (default tools/_out/). Every GPU step has a time limit of its own; the first failure ends the script.
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${CFEAR_OUT:-$R/tools/_out}
NAIVE=$R/tools/_stop/libcfear_hip_naive.so
mkdir -p "$OUT"
cd "$R" || exit 1
[ -f "$NAIVE" ] || { echo "missing $NAIVE (tools/build_variant.sh naive \"-DCFEAR_COV_SAMPLING_NAIVE=1\")"; exit 2; }
timeout -k 10 900 python tools/gpu_cov_sampling.py > "$OUT/cov_sampling_product.jsonl" 2> "$OUT/cov_sampling_product.err" || exit $?
CFEAR_COV_STREET=0 CFEAR_HIP_LIB=$NAIVE timeout -k 10 900 python tools/gpu_cov_sampling.py > "$OUT/cov_sampling_naive.jsonl" 2> "$OUT/cov_sampling_naive.err" || exit $?
for v in product naive; do
  rm -rf /tmp/cov_kt_$v
  if [ $v = naive ]; then export CFEAR_HIP_LIB=$NAIVE; else unset CFEAR_HIP_LIB; fi
  CFEAR_COV_STREET=0 timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/cov_kt_$v -o kt -- python "$R/tools/gpu_cov_sampling.py" > "$OUT/cov_sampling_rocprof_$v.log" 2>&1 || exit $?
  f=$(find /tmp/cov_kt_$v -name "*kernel_stats.csv" | head -1)
  [ -n "$f" ] && cp "$f" "$OUT/cov_sampling_kernel_stats_$v.csv"
done
unset CFEAR_HIP_LIB
head -c 3000 "$OUT/cov_sampling_product.jsonl"; head -c 1500 "$OUT/cov_sampling_naive.jsonl"
for v in product naive; do grep -i "cov_sample\|register_step\|features_step\|kstrongest" "$OUT/cov_sampling_kernel_stats_$v.csv" | cut -c1-200; done
