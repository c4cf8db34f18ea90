"""What recording the keyframes' clouds costs (cfear_odometry_set_keyframe_clouds): sweeps replayed through cfear_odometry_replay_device
(frames resident, nothing copied per sweep) with the recorder at NODES | CELLS - the baseline, which a tree without the point log runs
too -, + CLOUD and + CLOUD | PEAKS (the latter also puts the object's filter on its PEAKS = true instantiation). One line per
configuration, the median of three timed passes and the three values:
    python tools/gpu_keyframe_clouds.py <sweeps> <B> [baseline]
CFEAR_TREE: the tree whose package and bench.py are imported (default: this one) - tools/ab_keyframe_clouds.sh points it at a built copy
of the parent commit for the baseline line, interleaved with this tree's lines on the same box."""
import os, sys, time
import numpy as np
import torch
TREE = os.path.abspath(os.environ.get("CFEAR_TREE", os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, TREE)
import bench
from cfear_radarodometry_code_public_amd import capi

n, B = int(sys.argv[1]), int(sys.argv[2])
baseline_only = len(sys.argv) > 3 and sys.argv[3] == "baseline"
tag = os.environ.get("CFEAR_TAG", "this")
imgs = bench.make_streams(1, 72, 0)[0]
T = imgs.shape[0]
period = 2 * (T - 1)
order = [m if m < T else period - m for m in (i % period for i in range(n))]  # forwards, backwards, forwards ...: a consistent drive of any length
piece = max(1, min(n, (1 << 30) // (B * bench.A * bench.R)))
d_imgs = torch.from_numpy(imgs).cuda()
d_piece = torch.empty((piece, B, bench.A, bench.R), dtype=torch.uint8, device="cuda")
BASE = capi.KF_NODES | capi.KF_CELLS
configs = [("nodes + cells", BASE)]
if not baseline_only:
    configs += [("nodes + cells + cloud", BASE | capi.KF_CLOUD), ("nodes + cells + cloud + peaks", BASE | capi.KF_CLOUD | capi.KF_PEAKS)]
for name, what in configs:
    ctx = capi.Context(bench.params(capi), bench.A, bench.R)
    odo = ctx.odometry(B)
    if what == BASE:
        odo.record_keyframes(what, n, n * 112)
    else:
        odo.record_keyframes(what, n, n * 112, n * bench.A * 12)  # (about every second sweep fuses, its two clouds are < 2 A k points: a drop would show in the line)
    times = []
    for m in (min(n, 64), n, n, n):  # a short pass warms up (allocations, code objects), three are timed; the log starts again with every reset
        odo.reset()
        dt = 0.0
        for t0 in range(0, m, piece):
            cnt = min(piece, m - t0)
            d_piece[:cnt] = d_imgs[torch.tensor(order[t0:t0 + cnt], device="cuda")][:, None]
            torch.cuda.synchronize()
            t = time.perf_counter()
            odo.replay_device(d_piece, cnt)
            ctx.synchronize()
            dt += time.perf_counter() - t
        times.append(1e6 * dt / m)
    times = sorted(times[1:])
    recorded, dropped = odo.keyframe_counts()
    line = "%-6s B %4d  sweeps %4d  %-30s %8.1f us per sweep (three passes: %.1f %.1f %.1f)  keyframes %d..%d, dropped %d" % (
        tag, B, n, name, times[1], times[0], times[1], times[2], recorded.min(), recorded.max(), dropped.sum())
    if what != BASE:
        nc, npk = odo.keyframe_cloud_sizes(0)
        line += "  points of sequence 0: cloud %d, peaks %d (%.1f MB)" % (nc.sum(), npk.sum(), 12e-6 * (int(nc.sum()) + int(npk.sum())))
    print(line, flush=True)
    odo.release()
    ctx.close()
