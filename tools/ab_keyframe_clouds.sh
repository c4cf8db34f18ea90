#!/bin/bash
# Interleaved A/B of the keyframe recorder on one box: the parent commit's NODES | CELLS recording (a built copy of its tree, $1) against this
# tree's NODES | CELLS, + CLOUD and + CLOUD | PEAKS (tools/gpu_keyframe_clouds.py), three alternations (ALTERNATIONS) at one sequence and at 1536.
# Every run under its own time limit, the first failure ends the script. $2 = output file (default tools/_out/, ignored by git).
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); P=$(cd "$1" && pwd) || exit 2; OUT=${2:-$R/tools/_out/kf_clouds_ab.txt}
mkdir -p "$(dirname "$OUT")"; : > "$OUT"
# ORDER: who runs first in an alternation ("parent this", or "this parent" to tell a difference of the trees from a drift of the box);
# SIZES: the sequence counts (default "1 1536")
for B in ${SIZES:-1 1536}; do
  if [ "$B" = 1 ]; then cfg="${SWEEPS_1:-2000} 1"; else cfg="${SWEEPS_1536:-300} $B"; fi
  for i in $(seq 1 "${ALTERNATIONS:-3}"); do
    for who in ${ORDER:-parent this}; do
      if [ $who = parent ]; then
        (cd "$P" && CFEAR_TREE="$P" CFEAR_TAG=parent timeout -k 10 300 python "$R/tools/gpu_keyframe_clouds.py" $cfg baseline) >> "$OUT" 2>&1 || { echo "parent $cfg $i failed"; tail -5 "$OUT"; exit 1; }
      else
        (cd "$R" && CFEAR_TAG=this timeout -k 10 300 python "$R/tools/gpu_keyframe_clouds.py" $cfg ${THIS_MODE:-}) >> "$OUT" 2>&1 || { echo "this $cfg $i failed"; tail -5 "$OUT"; exit 1; }
      fi
    done
  done
done
cat "$OUT"
