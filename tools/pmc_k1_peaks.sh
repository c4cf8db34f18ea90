#!/bin/bash
# VALU / SALU / LDS instructions and wave cycles per azimuth row of the two instantiations of the k-strongest kernel - with the suppression phase
# (cfear_tune FILTER_PEAKS = 1) and without (0) - on S-uniform, S-world and S-ties; then the kernel times of both, interleaved. The counters come
# from a run of their own (rocprofv3 --pmc alone, no tracing in the same run); the timing run is not profiled. $1 = output file.
set -o pipefail
# (the default output folder, tools/_out/, is ignored by git)
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${1:-$R/tools/_out/k1_peaks.txt}; N=${K1_N:-1536}
W=$(mktemp -d); mkdir -p "$(dirname "$OUT")"
( cd "$W" && K1_N=$N K1_REPS=1 K1_CONFIGS="7,0" K1_PEAKS="1,0" timeout -k 10 300 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVE_CYCLES -f csv -d "$W/pmc" -o k1 -- python "$R/tools/gpu_time_k1_peaks.py" > "$W/pmc.log" 2>&1 ) || { tail -20 "$W/pmc.log"; exit 1; }
K1_N=$N K1_REPS=3 K1_CONFIGS="7,0" K1_PEAKS="1,0" timeout -k 10 300 python "$R/tools/gpu_time_k1_peaks.py" > "$W/time.log" 2>&1 || { tail -20 "$W/time.log"; exit 1; }
python - "$N" "$W" > "$OUT" <<'PY'
import csv, glob, collections, sys
N, W = int(sys.argv[1]), sys.argv[2]
d = collections.defaultdict(list)
for f in glob.glob(W + '/pmc/**/*counter_collection.csv', recursive=True):
    for r in csv.DictReader(open(f)):
        if 'kstrongest_kernel' in r['Kernel_Name']:
            d[(r['Kernel_Name'].replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0], r['Counter_Name'])].append((int(r['Dispatch_Id']), float(r['Counter_Value'])))
print("k-strongest kernel per azimuth row, with (<4, 7, true>) and without (<4, 7, false>) the suppression phase; %d-scan launches (%d rows), averages over 12 launches" % (N, N * 400))
print("per input; counters from a rocprofv3 --pmc run of their own; columns: uniform world ties")
for (kn, cn), l in sorted(d.items()):
    l.sort(); per = 12
    groups = [l[i:i + per] for i in range(0, len(l), per)]
    print("%-40s %-16s %s" % (kn, cn, " ".join("%9.1f" % (sum(v for _, v in g) / len(g) / (N * 400)) for g in groups[:3])))
print()
print(open(W + '/time.log').read())
PY
cat "$OUT"
rm -rf "$W"
