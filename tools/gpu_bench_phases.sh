set -x
R=$(cd "$(dirname "$0")/.." && pwd); O=${CFEAR_OUT:-$R/tools/_out}
cd $R
mkdir -p $O
(timeout 600 python bench.py --full --no-cpu-baseline --single-sequence-sweeps 0 --stream-steps 0 --steps 40 2>&1 | tail -1) > $O/gpu_bench.log 2>&1
(ODO_B=1536 ODO_U=16 timeout 600 python tools/gpu_phase_times.py 2>&1 | tail -12) > $O/gpu_phases.log 2>&1
