# The reference's CA-CFAR detector grid (params/kstrong_vs_cfar/oxford-cfear-3-ca-cfar: 7 windows x 7 false-alarm rates, guard 10, z_min 20) over S source
# sweeps of 400 x 3360: ONE call of cfear_filter_cfar_grid_device against the same 49 x S detections made the only way there was before it -
# cfear_filter_cfar_batch_device once per set over the same sweeps. Device events on the context's stream, warmed up, the two sides alternating in one
# process; the clouds of the two sides are compared byte for byte first. Writes the times, the ratio and the spread to argv[1]
# (default profiles/cfar_grid_time.txt). CFAR_S: source sweeps (1024), CFAR_REPS: timed alternations (7).
import os, sys, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cfear_radarodometry_code_public_amd import capi, synth
A, R, RR = 400, 3360, np.float32(0.0595238)
S = int(os.environ.get("CFAR_S", "1024")); REPS = int(os.environ.get("CFAR_REPS", "7")); U = 16
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "cfar_grid_time.txt")
WINDOWS, RATES, GUARD, ZMIN = (40, 70, 100, 150, 200, 300, 500), (0.1, 0.05, 0.01, 0.005, 0.001, 0.0005, 0.0001), 10, 20.0
SETS = [(w, GUARD, p, ZMIN) for w in WINDOWS for p in RATES]
K = len(SETS)
CAP = 4096  # points kept per cloud (the counts are the true ones either way; both sides truncate alike)
w = synth.World(1234)
uniq = torch.from_numpy(np.stack([synth.world_scan(w, u, A, R, RR, seed=1) for u in range(U)])).cuda()
d = uniq[torch.arange(S, device="cuda") % U].contiguous()
st = torch.cuda.Stream()  # the context's stream and the events': a stream of its own (the default stream's handle is 0, which asks the context for its own)
ctx = capi.Context(capi.default_params(range_res=RR, z_min=ZMIN), A, R, stream=st.cuda_stream)
# cloud k * S + s: source s under set k - the layout of the baseline's K calls, so that the buffers of the two sides compare as they are
dets = capi.detector_array([SETS[k] for k in range(K) for s in range(S)])
source = np.tile(np.arange(S, dtype=np.int32), K)
torch.cuda.synchronize()
xyi = [torch.zeros((K, S, CAP, 3), dtype=torch.float32, device="cuda") for _ in range(2)]
cnt = [torch.zeros((K, S), dtype=torch.int32, device="cuda") for _ in range(2)]


def grid():
    ctx.filter_cfar_grid(d.data_ptr(), S, dets, source, xyi[0].data_ptr(), CAP, cnt[0].data_ptr())


def baseline():
    for k, (win, guard, pfa, _) in enumerate(SETS):
        ctx.filter_cfar_batch(d.data_ptr(), S, xyi[1][k].data_ptr(), CAP, cnt[1][k].data_ptr(), window_size=win, nb_guard_cells=guard, false_alarm_rate=pfa)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st); fn(); e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


for _ in range(2):  # warm-up: tables, scratch, code objects
    grid(); baseline()
torch.cuda.synchronize()
same = bool(torch.equal(cnt[0], cnt[1])) and bool(torch.equal(xyi[0], xyi[1]))
if not same:
    sys.exit("the clouds of the two sides differ: nothing timed")
tg, tb = [], []
for _ in range(REPS):
    tg.append(timed(grid)); tb.append(timed(baseline))
tg, tb = np.array(tg), np.array(tb)
lines = [
    "CA-CFAR grid: %d sets (windows %s x rates %s, guard %d, z_min %g) over %d source sweeps of %d x %d, %d timed alternations" %
    (K, "/".join(map(str, WINDOWS)), "/".join(map(str, RATES)), GUARD, ZMIN, S, A, R, REPS),
    "clouds of the two sides byte-identical: yes (%d clouds, %.0f detections per cloud, %.1f %% truncated at %d points)" %
    (K * S, cnt[0].float().mean().item(), 100.0 * (cnt[0] > CAP).float().mean().item(), CAP),
    "grid     (one cfear_filter_cfar_grid_device call):        median %.2f ms, min %.2f, max %.2f, spread (max - min) / median %.1f %%" %
    (np.median(tg) * 1e3, tg.min() * 1e3, tg.max() * 1e3, 100.0 * (tg.max() - tg.min()) / np.median(tg)),
    "baseline (%d cfear_filter_cfar_batch_device calls):        median %.2f ms, min %.2f, max %.2f, spread (max - min) / median %.1f %%" %
    (K, np.median(tb) * 1e3, tb.min() * 1e3, tb.max() * 1e3, 100.0 * (tb.max() - tb.min()) / np.median(tb)),
    "grid / baseline: %.3f (medians); per sweep and set: grid %.2f us, baseline %.2f us" %
    (np.median(tg) / np.median(tb), np.median(tg) / (K * S) * 1e6, np.median(tb) / (K * S) * 1e6),
]
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
ctx.close()
