"""What registering loop candidates in one batch costs against the per-call loop (cfear_odometry_keyframe_edges against
cfear_odometry_keyframe_scans + cfear_register + release per candidate - the only route before it): the 2000-sweep drive of
tools/gpu_keyframes.py replayed once with NODES | CELLS, replay.loop_candidates on its ~990 keyframes cut at 1 and at 10 candidates per
node (about 1 k and 10 k jobs), each alone (n_side 0) and with two neighbours on each side (n_side 2).
    python tools/gpu_keyframe_edges.py [sweeps] [gap] [dist]
Per configuration five passes of each route in the same process, interleaved (batch, loop, batch, loop ...): median and range of both,
their ratio, and from event pairs around the calls the scan build's part of the batched call (cfear_odometry_keyframe_scans over the
same distinct keyframes, the one launch the batched call starts with) - the rest is the registration kernel and the copies. The
library reports what the call took from the pool on stderr (CFEAR_KF_EDGES_STATS). The per-call loop pays Python's ctypes calls too
(three per candidate); that is the route a user of the package had."""
import os, sys, time
os.environ["CFEAR_KF_EDGES_STATS"] = "1"
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from cfear_radarodometry_code_public_amd import capi, replay

n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
gap = int(sys.argv[2]) if len(sys.argv) > 2 else 6
dist = float(sys.argv[3]) if len(sys.argv) > 3 else 3.0
PASSES = 5
imgs = bench.make_streams(1, 72, 0)[0]
T = imgs.shape[0]
period = 2 * (T - 1)
order = [m if m < T else period - m for m in (i % period for i in range(n))]  # forwards, backwards, forwards ...
ctx = capi.Context(bench.params(capi), bench.A, bench.R)
odo = ctx.odometry(1)
odo.record_keyframes(capi.KF_NODES | capi.KF_CELLS, n, n * 400)
piece = max(1, min(n, (1 << 30) // (bench.A * bench.R)))
d_imgs = torch.from_numpy(imgs).cuda()
for t0 in range(0, n, piece):
    cnt = min(piece, n - t0)
    d_piece = d_imgs[torch.tensor(order[t0:t0 + cnt], device="cuda")][:, None].contiguous()
    torch.cuda.synchronize()
    odo.replay_device(d_piece, cnt)
    ctx.synchronize()
nodes = odo.keyframes(0)
recorded, dropped = odo.keyframe_counts()
print("sweeps %d, keyframes %d (dropped %d), cells per keyframe %d..%d" % (n, len(nodes), dropped.sum(), nodes["n_cells"].min(), nodes["n_cells"].max()), flush=True)


def per_call_loop(jobs):
    ok = 0
    for j in jobs:
        frm = [int(v) for v in j["from"][:int(j["n_from"])]]
        scans = odo.keyframe_scans(0, frm + [int(j["to"])])
        _, P, cov, S = ctx.register(scans, np.vstack([nodes["pose"][frm], nodes["pose"][int(j["to"])]]))
        for s in scans:
            s.release()
        ok += int(S.success)
    return ok


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    t = time.perf_counter()
    out = fn()
    dt = time.perf_counter() - t
    b.record()
    b.synchronize()
    return out, 1e3 * dt, a.elapsed_time(b)


def scans_only(keys):
    scans = odo.keyframe_scans(0, keys)
    for s in scans:
        s.release()


for per_node in (1, 10):
    pairs = replay.loop_candidates(nodes, gap, dist, max_per_node=per_node)
    for n_side in (0, 2):
        jobs = replay.edge_jobs(0, pairs, n_side, len(nodes))
        keys = sorted(set(int(v) for j in jobs for v in list(j["from"][:int(j["n_from"])]) + [int(j["to"])]))
        odo.keyframe_edges(jobs[:32]); per_call_loop(jobs[:32]); scans_only(keys[:32])  # warm: code objects, the pool
        tb, tl, eb, es = [], [], [], []
        for _ in range(PASSES):
            edges, w, e = timed(lambda: odo.keyframe_edges(jobs))
            tb.append(w); eb.append(e)
            ok, w, _ = timed(lambda: per_call_loop(jobs))
            tl.append(w)
            _, _, e = timed(lambda: scans_only(keys))
            es.append(e)
        assert ok == int(edges["success"].sum())
        mb, ml, me, ms = np.median(tb), np.median(tl), np.median(eb), np.median(es)
        print("jobs %5d  n_side %d  n_from %d..%d  distinct keyframes %d  usable %d  success %d  blocks %d..%d" % (
            len(jobs), n_side, jobs["n_from"].min(), jobs["n_from"].max(), len(keys), edges["usable"].sum(), edges["success"].sum(),
            edges["num_residual_blocks"].min(), edges["num_residual_blocks"].max()), flush=True)
        print("    one call       median %9.2f ms  (range %.2f .. %.2f)  %.1f us per job" % (mb, min(tb), max(tb), 1e3 * mb / len(jobs)), flush=True)
        print("    per-call loop  median %9.2f ms  (range %.2f .. %.2f)  %.1f us per job" % (ml, min(tl), max(tl), 1e3 * ml / len(jobs)), flush=True)
        print("    ratio loop / call %.1f (ranges %s)" % (ml / mb, "separate" if min(tl) > max(tb) else "OVERLAP"), flush=True)
        print("    events: the call %.2f ms (range %.2f .. %.2f), the scan build of its %d keyframes alone %.2f ms (range %.2f .. %.2f): %.0f %% of the call, "
              "the registration kernel and the copies the other %.0f %%" % (me, min(eb), max(eb), len(keys), ms, min(es), max(es), 100 * ms / me, 100 - 100 * ms / me), flush=True)
odo.release()
ctx.close()
