"""What the keyframe recorder costs: 2000 sweeps replayed (cfear_odometry_replay_device: frames resident, nothing copied per sweep) at
B = 1, 64 and 1536 sequences with recording off, NODES and NODES | CELLS. Up to 256 sequences recording also takes the replay off the
persistent kernel (replay.hip), so recording off is timed a second time at REPLAY_PERSISTENT_MAX = 0 - the two-launch route the recorder
rides on - and the recorder's own share is the difference to that. One line per configuration:
    python tools/gpu_keyframes.py [sweeps] [B ...]
Every configuration runs three timed passes of all sweeps; the line gives the median and the three values."""
import os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from cfear_radarodometry_code_public_amd import capi

n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
sizes = [int(v) for v in sys.argv[2:]] or [1, 64, 1536]
imgs = bench.make_streams(1, 72, 0)[0]
T = imgs.shape[0]
period = 2 * (T - 1)
order = [m if m < T else period - m for m in (i % period for i in range(n))]  # forwards, backwards, forwards ...: a consistent drive of any length
for B in sizes:
    # the frames of a piece on the device: every sequence replays the same drive (what it costs does not depend on whose sweeps they are)
    piece = max(1, min(n, (1 << 30) // (B * bench.A * bench.R)))
    d_imgs = torch.from_numpy(imgs).cuda()
    d_piece = torch.empty((piece, B, bench.A, bench.R), dtype=torch.uint8, device="cuda")
    res = {}
    for name, what, pmax in (("off", 0, 256), ("off, two launches per sweep", 0, 0), ("nodes", capi.KF_NODES, 256), ("nodes + cells", capi.KF_NODES | capi.KF_CELLS, 256)):
        if B > 256 and pmax == 0:
            continue  # (already the route of recording off)
        ctx = capi.Context(bench.params(capi), bench.A, bench.R)
        ctx.tune(capi.TUNE_REPLAY_PERSISTENT_MAX, pmax)
        odo = ctx.odometry(B)
        if what:
            odo.record_keyframes(what, n, n * 112 if what & capi.KF_CELLS else 0)  # (a drop would show in the line)
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
        line = "B %4d  %-28s %8.1f us per sweep (median of three passes: %.1f %.1f %.1f)" % (B, name, times[1], times[0], times[1], times[2])
        if what:
            recorded, dropped = odo.keyframe_counts()
            line += "  keyframes %d..%d, dropped %d" % (recorded.min(), recorded.max(), dropped.sum())
        res[name] = times[1]
        print(line, flush=True)
        odo.release()
        ctx.close()
    base = res.get("off, two launches per sweep", res["off"])
    print("B %4d  leaving the persistent kernel %+.1f us per sweep; the recorder itself: nodes %+.1f, nodes + cells %+.1f us per sweep" %
          (B, base - res["off"], res["nodes"] - base, res["nodes + cells"] - base), flush=True)
