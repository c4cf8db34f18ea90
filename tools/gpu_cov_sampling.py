# estimate_cov_by_sampling on the batched step (cfear_odometry_set_cov_sampling): steps per second with the option off, on at 3 and on at 5
# samples per axis, ALTERNATING in one process (the modes see the same clocks and the same resident sweeps), at CFEAR_COV_B sequences (default 4608)
# of BASELINE configs[1] after bench.py's 8-sweep pre-roll; then the CFEAR-3 street preset (k = 40, P2P, street world) at 1536 sequences, off and at 3.
# "registration stage" = the stage events around the registration kernel and, when on, the sampling kernel behind it (cov_sample_kernel). One JSON
# line per leg. CFEAR_HIP_LIB=tools/_stop/libcfear_hip_naive.so runs the A/B build of tools/build_variant.sh (every sample a get_cost_block).
import json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench


def leg(capi, dev, stream, name, pk, st, B, modes, W=4, K=12, reps=3):
    p = capi.default_params(range_res=bench.RANGE_RES, **pk)
    ctx = capi.Context(p, bench.A, bench.R, device=0, stream=stream)
    odo = ctx.odometry(B)
    U = st.shape[0]
    frames = st.shape[1] - bench.PRE_ROLL
    wl = bench.Resident(torch, dev, st, list(range(B)), 1, 0, B, U, frames, seed=77)
    odo.reset()
    wl.pre_roll(ctx, odo)
    step = 0
    for _ in range(W):
        odo.step_device(wl.d_polar[wl.frame_of(step)].data_ptr()); step += 1
    res = {m: [] for m in modes}
    for r in range(reps):
        for m in modes:
            if m:
                odo.set_cov_sampling(True, 0.4, 0.0043625, m, 4.0)
            else:
                odo.set_cov_sampling(False)
            for _ in range(2):  # the first steps of a mode are not timed
                odo.step_device(wl.d_polar[wl.frame_of(step)].data_ptr()); step += 1
            ctx.synchronize(); torch.cuda.synchronize()
            odo.profile(True)
            t0 = time.perf_counter()
            for _ in range(K):
                odo.step_device(wl.d_polar[wl.frame_of(step)].data_ptr()); step += 1
            ctx.synchronize(); torch.cuda.synchronize()
            el = time.perf_counter() - t0
            t_f, n_f = odo.profile_read()
            t_feat, t_reg, n = odo.profile_read_stages()
            odo.profile(False)
            res[m].append(dict(steps_per_s=K / el, scans_per_s=B * K / el, filter_us=1e6 * t_f / max(n_f, 1), features_us=1e6 * t_feat / max(n, 1),
                               registration_stage_us=1e6 * t_reg / max(n, 1)))
    sampled = sum(int(odo.cov_samples(q)[1]) for q in range(0, B, max(1, B // 64))) if modes[-1] else None
    out = {"leg": name, "sequences": B, "steps_per_mode_and_repeat": K, "repeats": reps, "lib": os.path.basename(os.environ.get("CFEAR_HIP_LIB", "product build")),
           "sampled_fraction_of_64": sampled}
    for m in modes:
        key = "off" if not m else "samples_per_axis_%d" % m
        v = res[m]
        out[key] = {k: float(np.median([x[k] for x in v])) for k in v[0]}
        out[key]["steps_per_s_all"] = [round(x["steps_per_s"], 2) for x in v]
    off = out["off"]["registration_stage_us"]
    for m in modes:
        if m:
            out["samples_per_axis_%d" % m]["sampling_us_over_off"] = out["samples_per_axis_%d" % m]["registration_stage_us"] - off
    print(json.dumps(out), flush=True)
    odo.release(); ctx.close(); wl.free()


def main():
    torch.cuda.set_stream(torch.cuda.Stream())
    from cfear_radarodometry_code_public_amd import capi
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    W, K = 4, 12
    B = int(os.environ.get("CFEAR_COV_B", "4608"))
    st = bench.make_streams(16, bench.PRE_ROLL + W + K, 0)
    leg(capi, dev, stream, "configs1", dict(bench.PARAMS), st, B, [0, 3, 5], W, K)
    if os.environ.get("CFEAR_COV_STREET", "1") == "1":
        pk = dict(bench.PARAMS, k_strongest=40, cost=0, submap_scan_size=4, res=3.0, weight_intensity=1, weight_opt=4)
        st2 = bench.dense_streams(16, bench.PRE_ROLL + W + K, kind="street")
        leg(capi, dev, stream, "cfear3_k40_p2p_street", pk, st2, 1536, [0, 3], W, K)


if __name__ == "__main__":
    main()
