# Cost surfaces (GetSurface): the measurements of DESIGN.md. Per call: an 81 x 81 surface (res 0.05, width 2) around the registered pose of
# BASELINE configs[1] (k = 12, P2L, four keyframes) and of the CFEAR-3 street preset (k = 40, P2P, street world). Batched: cfear_odometry_surface
# at CFEAR_SURF_B sequences (default 1536) of configs[1] with width 1, res 0.05 (41 x 41), after bench.py's pre-roll. Wall-clock per call
# (synchronised), blocks per problem and ns per (visited pixel x block). One JSON line per leg. CFEAR_HIP_LIB=tools/_stop/libcfear_hip_surfnaive.so
# runs the A/B build (tools/build_variant.sh surfnaive "-DCFEAR_SURFACE_NAIVE=1"). Kernel times: run under rocprofv3 --kernel-trace --stats.
import json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench


def per_call(capi, name, pk, imgs, reps):
    p = capi.default_params(range_res=bench.RANGE_RES, **pk)
    ctx = capi.Context(p, bench.A, bench.R, device=0)
    scans = [ctx.scan_create(ctx.filter_polar(img, peaks=False)[0]) for img in imgs]
    poses = np.zeros((len(scans), 3))
    ok, poses, _, S = ctx.register(scans, poses)
    itr = S.outer_iterations
    _, res = ctx.get_cost(scans, poses, itr=itr)
    blocks = len(res) // (1 if pk.get("cost", 1) == 1 else 2)
    surf = ctx.get_surface(scans, poses, 0.05, 2, itr=itr)  # (warm-up)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        surf = ctx.get_surface(scans, poses, 0.05, 2, itr=itr)
        t.append(time.perf_counter() - t0)
    vis = int(np.isfinite(surf).sum())
    med = float(np.median(t))
    print(json.dumps({"leg": name, "pixels": surf.shape[0], "visited": vis, "blocks": blocks, "itr": itr, "ms_per_call": 1e3 * med,
                      "ms_all": [round(1e3 * x, 3) for x in t], "ns_per_pixel_block_wall": 1e9 * med / (vis * blocks),
                      "lib": os.path.basename(os.environ.get("CFEAR_HIP_LIB", "product build"))}), flush=True)
    ctx.close()


def batched(capi, dev, stream, B, reps, W=4):
    p = capi.default_params(range_res=bench.RANGE_RES, **bench.PARAMS)
    ctx = capi.Context(p, bench.A, bench.R, device=0, stream=stream)
    odo = ctx.odometry(B)
    st = bench.make_streams(16, bench.PRE_ROLL + W + 4, 0)
    wl = bench.Resident(torch, dev, st, list(range(B)), 1, 0, B, st.shape[0], st.shape[1] - bench.PRE_ROLL, seed=77)
    odo.set_surface_recording(True)
    odo.reset()
    wl.pre_roll(ctx, odo)
    for s in range(W):
        odo.step_device(wl.d_polar[wl.frame_of(s)].data_ptr())
    ctx.synchronize()
    out, n_used, itr_used, _ = odo.surface(0.05, 1, details=True)  # (warm-up)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = odo.surface(0.05, 1)
        t.append(time.perf_counter() - t0)
    blocks = [odo.summary(q)[0].num_residual_blocks for q in range(0, B, max(1, B // 128))]
    vis = int(torch.isfinite(out).sum().item())
    med = float(np.median(t))
    print(json.dumps({"leg": "batched_configs1", "sequences": B, "pixels": int(out.shape[1]), "visited_all": vis,
                      "blocks_mean_approx": float(np.mean(blocks)), "ms_per_call": 1e3 * med, "ms_all": [round(1e3 * x, 3) for x in t],
                      "ns_per_pixel_block_wall": 1e9 * med / (vis * float(np.mean(blocks))),
                      "lib": os.path.basename(os.environ.get("CFEAR_HIP_LIB", "product build"))}), flush=True)
    odo.release(); ctx.close(); wl.free()


def main():
    torch.cuda.set_stream(torch.cuda.Stream())
    from cfear_radarodometry_code_public_amd import capi
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    reps = int(os.environ.get("CFEAR_SURF_REPS", "5"))
    st = bench.make_streams(1, 5, 0)
    per_call(capi, "per_call_configs1", dict(bench.PARAMS), st[0, :5], reps)
    st2 = bench.dense_streams(1, 5, kind="street")
    per_call(capi, "per_call_cfear3_k40_p2p_street", dict(bench.PARAMS, k_strongest=40, cost=0), st2[0, :5], reps)
    batched(capi, dev, stream, int(os.environ.get("CFEAR_SURF_B", "1536")), reps)


if __name__ == "__main__":
    main()
