#!/bin/bash
# HBM traffic of the k-strongest kernel: FETCH_SIZE and WRITE_SIZE in separate --pmc passes
# (MI355X_MICROARCH.md "HBM": TCC slots do not fit both; FETCH_SIZE reads 1/2 of a wide coalesced stream on gfx950)
R=$(cd "$(dirname "$0")/.." && pwd); O=${CFEAR_OUT:-$R/tools/_out}; mkdir -p $O; cd /tmp && export TMPDIR=/tmp
for c in FETCH_SIZE WRITE_SIZE; do
  K1_REPS=2 K1_CONFIGS="8,2,0" rocprofv3 --kernel-trace --pmc $c -d $O/pmc_k1_$c -o k1 -- python $R/tools/gpu_time_k1.py > $O/pmc_k1_$c.log 2>&1
done
cd $R && rocprofv3 --kernel-trace --stats -d $O/prof_bench -o bench -- python $R/bench.py --full --steps 20 --warmup 10 --no-cpu-baseline > $O/prof_bench.log 2>&1
tail -1 $O/prof_bench.log | cut -c1-300
