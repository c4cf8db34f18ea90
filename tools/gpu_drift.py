"""Time of scoring a replayed grid on the device (cfear_drift_device, csrc/drift.hip) at the shape of an Oxford-length recording under a
1536-row grid - 8800 sweeps x 1536 rows of synthetic poses (0.9-1.1 m per sweep) in device memory in the record layout
cfear_odometry_replay_device leaves (stride 80) - and at B = 64 and B = 1; against kitti.drift per row in Python (a sample of 16 rows,
extrapolated). Every timed call is followed by a context synchronise; the median of the timed calls after the warm-up is reported.
usage: python tools/gpu_drift.py [--sweeps 8800] [--rows 1536] [--calls 60] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cfear_radarodometry_code_public_amd import capi, kitti  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=8800)
    ap.add_argument("--rows", type=int, default=1536)
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--sample", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    n, B = a.sweeps, a.rows
    rng = np.random.default_rng(7)
    th = np.cumsum(rng.normal(0, 0.01, n))
    v = 0.9 + 0.2 * rng.random(n)
    g = np.stack([np.cumsum(v * np.cos(th)), np.cumsum(v * np.sin(th)), th], 1)
    gt = kitti.poses_from_xyt(g)
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(3)
    rec = torch.full((n, B, 10), 1.5, dtype=torch.float64, device=dev)  # 80-byte records: the pose, then 56 bytes of other fields
    sig = torch.tensor([0.01, 0.01, 1e-3], dtype=torch.float64, device=dev)
    walk = torch.zeros((B, 3), dtype=torch.float64, device=dev)
    tg = torch.from_numpy(g).to(dev)
    for t0 in range(0, n, 400):  # (in pieces: the noise of all sweeps at once would double the footprint)
        m = min(400, n - t0)
        steps = torch.randn((m, B, 3), dtype=torch.float64, device=dev, generator=gen) * sig
        steps[0] += walk
        pos = torch.cumsum(steps, 0)
        walk = pos[-1].clone()
        rec[t0:t0 + m, :, :3] = tg[t0:t0 + m, None, :] + pos
    torch.cuda.synchronize()
    ctx = capi.Context(capi.default_params(), 400, 3360)
    t0 = time.perf_counter()
    plan = ctx.drift_plan(gt)
    t_plan = time.perf_counter() - t0
    seg = capi.drift_segments(gt)
    res = {"sweeps": n, "rows": B, "path_m": float(np.sum(v)), "segments": int(len(seg)), "plan_create_s": t_plan, "record_bytes": n * B * 80, "device": []}
    d_out = torch.zeros(B * 184, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    for b in (B, 64, 1):
        if b > B:
            continue
        times = []
        for i in range(10 + a.calls):
            t0 = time.perf_counter()
            plan.score(rec, n_sweeps=n, n_sequences=b, sweep_stride=B * 80, seq_stride=80, out=d_out)  # rows 0 .. b - 1 of the same buffer
            ctx.synchronize()
            times.append(time.perf_counter() - t0)
        t = float(np.median(times[10:]))
        # bytes the algorithm needs: per row one pose per segment end and one per start; what the stride-80 pattern fetches: whole 128-B lines
        starts = len(np.unique(seg[:, 0]))
        need = b * (len(seg) + starts) * 24
        res["device"].append({"rows": b, "median_s": t, "min_s": float(np.min(times[10:])), "max_s": float(np.max(times[10:])), "calls": a.calls,
                              "pose_bytes_needed": need, "needed_GBps": need / t / 1e9, "record_bytes_touched": b * (len(seg) + starts) * 80,
                              "touched_GBps": b * (len(seg) + starts) * 80 / t / 1e9})
    full = plan.score(rec, n_sweeps=n, n_sequences=B)
    # kitti.drift per row in Python on a sample, and agreement of the device result with it at this size
    k = min(a.sample, B)
    pick = np.linspace(0, B - 1, k).astype(int)
    poses = rec[:, pick.tolist(), :3].cpu().numpy()
    t0 = time.perf_counter()
    host = [kitti.drift(gt, kitti.poses_from_xyt(poses[:, i])) for i in range(k)]
    t_py = (time.perf_counter() - t0) / k
    res["python_per_row_s"] = t_py
    res["python_all_rows_s_extrapolated"] = t_py * B
    res["agreement_on_sample"] = {
        "segments_equal": bool(all(int(full[q]["segments"]) == h["segments"] for q, h in zip(pick, host))),
        "translation_rel": float(max(abs(full[q]["translation_percent"] - h["translation_percent"]) / h["translation_percent"] for q, h in zip(pick, host))),
        "rotation_rel": float(max(abs(full[q]["rotation_deg_per_100m"] - h["rotation_deg_per_100m"]) / h["rotation_deg_per_100m"] for q, h in zip(pick, host)))}
    plan.release()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
