#!/bin/bash
# Interleaved A/B of the driver's bench command on one box: a built copy of the parent commit's tree ($1) against this tree, three alternations
# (ALTERNATIONS), every run under its own time limit, the first failure ends the script. $2 = output file (default tools/_out/, ignored by git).
# One line per run: ms per step, scans/s, the three step kernels' launch times (HIP events inside the timed region) and the five repeats.
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); P=$(cd "$1" && pwd) || exit 2; OUT=${2:-$R/tools/_out/bench_ab.txt}
mkdir -p "$(dirname "$OUT")"; W=$(mktemp -d); : > "$OUT"
for i in $(seq 1 "${ALTERNATIONS:-3}"); do
  for who in parent this; do
    if [ $who = parent ]; then cd "$P"; else cd "$R"; fi
    timeout -k 10 400 python bench.py --gpus 1 --steps 20 --warmup 5 --repeats 5 2> "$W/err.log" | tail -1 > "$W/line.json" || { echo "$who $i failed"; tail -5 "$W/err.log"; exit 1; }
    python - "$who" "$i" "$W/line.json" >> "$OUT" <<'PY' || exit 1
import json, sys
d = json.load(open(sys.argv[3])); k = d["kernels"]
print("%-6s %s  ms_per_step %.4f  scans/s %.0f  kstrongest_launch_us %.1f  features_launch_us %.1f  registration_launch_us %.1f  repeats (scans/s) %s" % (
    sys.argv[1], sys.argv[2], d["ms_per_step"], d["value"], k["kstrongest_launch_us"], k["features_launch_us"], k["registration_launch_us"],
    " ".join("%.0f" % v for v in d["repeats"]["values"])))
PY
  done
done
cat "$OUT"; rm -rf "$W"
