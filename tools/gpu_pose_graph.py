"""What optimising the keyframe graph on the device costs (cfear_pose_graph_optimize, pose_graph.hip): the 2000-sweep drive of
tools/gpu_keyframes.py replayed once with NODES | CELLS, replay.loop_candidates on its keyframes cut at 1 and at 10 candidates per node,
registered in one cfear_odometry_keyframe_edges call, and the resulting graph optimised as 1, 64 and 512 identical rows of one call -
beside posegraph.optimize_direct (scipy's sparse direct solve, Gauss-Newton) on the host for one row. Then the preconditioner's bad case:
a chain of 1000 nodes closed by a single loop edge.
    python tools/gpu_pose_graph.py [sweeps] [gap] [dist]
Five passes of every configuration in the same process, interleaved; median and range of the wall time of Context.pose_graph_optimize
(the host's table building, the copies, the one launch and the synchronisation) and of the host solver. No threshold anywhere.
The drive's two graphs run under a cap on the Levenberg-Marquardt iterations (see below; CFEAR_PG_TOOL_FULL=1 lifts it)."""
import os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from cfear_radarodometry_code_public_amd import capi, replay, posegraph as pg

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
print("sweeps %d, keyframes %d" % (n, len(nodes)), flush=True)


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return out, 1e3 * (time.perf_counter() - t)


def line(name, t):
    return "%s median %10.2f ms  (range %.2f .. %.2f)" % (name, np.median(t), min(t), max(t))


# The drive's graphs are timed under a cap on the Levenberg-Marquardt iterations (CFEAR_PG_TOOL_FULL=1: the default 50): the registrations of
# this synthetic drive come with covariances so small that neither solver converges on its graph (the device ends at its iteration limit,
# Gauss-Newton at its own), and an uncapped call of the denser graph takes most of a minute. The time of a call is its CG iterations times
# the time of one, which is what the capped calls measure.
FULL = os.environ.get("CFEAR_PG_TOOL_FULL") == "1"
problems = []
for per_node, cap in ((1, 3), (10, 1)):
    pairs = replay.loop_candidates(nodes, gap, dist, max_per_node=per_node)
    edges = odo.keyframe_edges(replay.edge_jobs(0, pairs, 0, len(nodes)))
    x0, E = pg.problem(nodes, edges)
    cap = 50 if FULL else cap
    (opt, S), t_log = timed(lambda: odo.keyframe_optimize(edges, max_iterations=cap))
    print("loop candidates per node <= %d: %d edges registered, %d with success; graph %d nodes %d edges; the log's route (one row, max_iterations %d) %.2f ms" % (
        per_node, len(edges), int(edges["success"].sum()), len(x0), len(E), cap, t_log), flush=True)
    problems.append(("drive, <= %d loops per node, max_iterations %d" % (per_node, cap), x0, E, cap))
x0, E, _ = pg.out_and_back(1000, seed=1000)
loops = np.flatnonzero(E["flags"] & 1)
far = loops[np.argmax(E["a"][loops] - E["b"][loops])]
problems.append(("chain of 1000 nodes, one loop edge (%d -> %d)" % (E["a"][far], E["b"][far]), x0, np.concatenate([E[(E["flags"] & 1) == 0], E[far:far + 1]]), 50))

for name, x0, E, cap in problems:
    ctx.pose_graph_optimize(x0, E, max_iterations=1, max_linear_iterations=10)  # warm: the code object, the pool
    rows = (1, 64, 512)
    td = {r: [] for r in rows}
    th = []
    for _ in range(PASSES):
        for r in rows:
            (got, S), w = timed(lambda: ctx.pose_graph_optimize([x0] * r, [E] * r, max_iterations=cap))
            td[r].append(w)
            assert all(g.tobytes() == got[0].tobytes() for g in got) and S.tobytes() == np.repeat(S[:1], r).tobytes()  # every row the same bits
        (xd, info), w = timed(lambda: pg.optimize_direct(x0, E, max_iterations=min(cap, 20)))
        th.append(w)
    dxy = float(np.max(np.hypot(got[0][:, 0] - xd[:, 0], got[0][:, 1] - xd[:, 1])))
    dth = float(np.max(np.abs(pg.wrap_pi(got[0][:, 2] - xd[:, 2]))))
    s = S[0]
    print("%s: %d nodes, %d edges" % (name, len(x0), len(E)), flush=True)
    print("    device: LM %d (%d accepted), CG %d in all, %s, cost %.9g -> %.9g" % (s["iterations"], s["accepted"], s["linear_iterations"],
                                                                                   capi.PG_TERMINATION[int(s["termination"])], s["initial_cost"], s["final_cost"]))
    for r in rows:
        print("    " + line("%3d rows in one call " % r, td[r]) + "  %.2f ms per row" % (np.median(td[r]) / r) + (
            ", %.2f us per CG iteration (the whole call over the row's CG iterations)" % (1e3 * np.median(td[r]) / max(int(s["linear_iterations"]), 1)) if r == 1 else ""))
    print("    " + line("optimize_direct, host", th) + "  (%d Gauss-Newton steps, cost %.9g); device - direct: %.3e m %.3e rad" % (info["iterations"], info["cost"], dxy, dth), flush=True)
odo.release()
ctx.close()
