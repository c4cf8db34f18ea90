# K1 (k-strongest) with and without the suppression phase - cfear_tune FILTER_PEAKS 1 / 0, i.e. kstrongest_kernel<.., true> / <.., false> - on
# S-uniform, S-world and S-ties, interleaved; K1_CONFIGS = "occ,rows;..." launch shapes (rows 0 = the library's default), K1_PEAKS = knob values,
# K1_N scans per launch, K1_REPS rounds. Launch order inside a round: shape, knob, input (uniform, world, ties), 2 warm-up + 10 timed launches each.
import os, sys, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cfear_radarodometry_code_public_amd import capi, synth
A, R, k = 400, 3360, 12
n = int(os.environ.get("K1_N", "1536"))
ctx = capi.Context(capi.default_params(range_res=np.float32(0.0595238)), A, R)
data = {}
ub = torch.from_numpy(np.stack([synth.uniform_scan(A, R, seed=0xC0FFEE + u) for u in range(min(n, 64))])).cuda()
data["uniform"] = ub.repeat((n + ub.shape[0] - 1) // ub.shape[0], 1, 1)[:n].contiguous()
w = synth.World(1234)
base = torch.from_numpy(np.stack([synth.world_scan(w, t, seed=1) for t in range(8)])).cuda()
data["world"] = base.repeat(n // 8, 1, 1).contiguous()
tb = torch.from_numpy(np.stack([synth.ties_scan(A, R, seed=7 + u) for u in range(8)])).cuda()
data["ties"] = tb.repeat(n // 8, 1, 1).contiguous()
names = [x for x in os.environ.get("K1_INPUTS", "uniform,world,ties").split(",") if x]
out = torch.zeros((n, A, k), dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
configs = [tuple(int(x) for x in c.split(",")) for c in os.environ.get("K1_CONFIGS", "7,0").split(";")]
knobs = [int(x) for x in os.environ.get("K1_PEAKS", "1,0").split(",")]
res, launched = {}, {}
for rep in range(int(os.environ.get("K1_REPS", "3"))):
    for (occ, rows) in configs:
        ctx.tune(capi.TUNE_FILTER_OCCUPANCY, occ); ctx.tune(capi.TUNE_FILTER_ROWS_PER_WAVE, rows)
        launched[(occ, rows)] = ctx.kstrongest_launch_shape(n)[0]
        for pk in knobs:
            ctx.tune(capi.TUNE_FILTER_PEAKS, pk)
            for name in names:
                res.setdefault((occ, rows, pk, name), []).append(ctx.time_kstrongest(data[name], n, out, 2, 10))
print("k-strongest kernel, %d-scan launches, us per launch (each value: the mean of 10 launches); peaks 1 = kstrongest_kernel<4,occ,true>, 0 = <4,occ,false>" % n)
for (occ, rows, pk, name), ts in res.items():
    print("occ=%d rows/wave=%d (launched: %d) peaks=%d %-8s %s  min %.1f  %.2f TB/s" % (
        occ, rows, launched[(occ, rows)], pk, name,
        " ".join("%7.1f" % (t * 1e6) for t in ts), min(ts) * 1e6, n * (A * R + A * k * 4) / min(ts) / 1e12))
