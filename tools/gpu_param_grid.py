# Parameter grids in one batch (cfear_odometry_set_sequence_params / _set_sequence_sources): what the feature is worth. BASELINE configs[1]
# (bench.PARAMS), CFEAR_GRID_B sequences (default 1536) over CFEAR_GRID_SOURCES generated recordings (default 64), after bench.py's 8-sweep pre-roll
# and W warm-up steps; per leg three repeats of K timed steps, medians, the filter time from cfear_odometry_profile_read and the features /
# registration split from cfear_odometry_profile_read_stages. One JSON line per leg:
#   (a) no table                      - the behaviour without the feature, the reference point
#   (b) identity table + identity map - the overhead of the lookups
#   (c) a B-row grid (losses x limits x weights x res x z_min x weight_intensity), every sequence with its own copy of its sweep
#   (d) the same grid on the shared sources: the filter runs on 64 sweeps per step instead of B, and 64 sweeps per step are resident
#   (e) the kstrong_vs_cfar axis (params/kstrong_vs_cfar/oxford-cfear-3-kstrong: k = 1 5 10 20 30 40 50) on the CFEAR-3 preset: the seven k of
#       every recording as seven sequences of ONE object under K = 50 on the shared sources (7 x sources sequences; the filter runs once per
#       recording, with k = 50, and 50 slots per bearing are resident for every row)
#   (f) the same seven values as seven uniform objects, one per k, a sequence per recording (the filter runs once per recording and k)
#   (g) the reference's params/submap_keyframes/submap_keyframe_cfear-3 (cost_type P2P P2L P2D x submap_scan_size 1 .. 10, utils/worker:49-52) on the
#       CFEAR-3 preset: the 30 points of every recording as 30 sequences of ONE object under submap_scan_size 10 on the shared sources
#       (cfear_odometry_set_sequence_shapes; 30 x sources sequences: every row pays the 11 scan slots and the scratch of ten keyframes, and the
#       registration stage is up to six launches per sweep, one per (cost, up to 7 keyframes or more))
#   (h) the same 30 points as 30 uniform objects, one per (cost, submap_scan_size), a sequence per recording; the last line sums them
# CFEAR_GRID_LEGS: a comma-separated subset of a,b,c,d,e,f,g,h (default: all)
# usage: python tools/gpu_param_grid.py >> profiles/param_grid_steps.jsonl
import json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench


def grid_rows(capi, replay, base, B):
    rows = replay.param_grid(base, loss=[1, 2, 3, 5], loss_limit=[0.1, 0.5, 1.0, 2.0], weight_opt=[0, 2, 4, 5], res=[2.5, 3.0, 3.5, 5.0],
                             z_min=[50.0, 60.0, 70.0], weight_intensity=[0, 1])  # 1536 points in the worker's loop order
    return [rows[q % len(rows)] for q in range(B)]


def leg(capi, name, ctx_params, stream, B, S, d_frames, d_pre, idx, rows, shared, W, K, reps, shapes=None):
    """d_frames: [frames, S, A, R] resident sweeps of the S sources; shared: the object reads them through a source map, otherwise every
    sequence gets its own copy ([frames, B, A, R], gathered here, resident for the leg)"""
    ctx = capi.Context(ctx_params, bench.A, bench.R, device=0, stream=stream)
    odo = ctx.odometry(B)
    if shapes is not None:
        odo.set_sequence_shapes(shapes)
    if rows is not None:
        odo.set_sequence_params(rows)
    frames = d_frames.shape[0]
    if shared:
        odo.set_sequence_sources(idx.cpu().numpy().astype(np.int32), S)
        d_in, d_tmp = d_frames, None
    else:
        if rows is not None and name.startswith("b"):
            odo.set_sequence_sources(np.arange(B, dtype=np.int32), B)
        d_in = torch.empty((frames, B, bench.A, bench.R), dtype=torch.uint8, device=d_frames.device)
        for t in range(frames):
            torch.index_select(d_frames[t], 0, idx, out=d_in[t])
        d_tmp = torch.empty((B, bench.A, bench.R), dtype=torch.uint8, device=d_frames.device)
    torch.cuda.synchronize()
    period = 2 * (frames - 1)
    frame_of = lambda s: (s % period) if (s % period) < frames else period - (s % period)  # forwards, then backwards (bench.Resident.frame_of)
    for t in range(bench.PRE_ROLL):
        if shared:
            src = d_pre[:, t].contiguous()
        else:
            torch.index_select(d_pre[:, t], 0, idx, out=d_tmp); src = d_tmp
        torch.cuda.current_stream().synchronize()
        odo.step_device(src.data_ptr())
        ctx.synchronize()
    step = 0
    for _ in range(W):
        odo.step_device(d_in[frame_of(step)].data_ptr()); step += 1
    res = []
    for r in range(reps):
        ctx.synchronize(); torch.cuda.synchronize()
        odo.profile(True)
        t0 = time.perf_counter()
        for _ in range(K):
            odo.step_device(d_in[frame_of(step)].data_ptr()); step += 1
        ctx.synchronize(); torch.cuda.synchronize()
        el = time.perf_counter() - t0
        t_f, n_f = odo.profile_read()
        t_feat, t_reg, n = odo.profile_read_stages()
        odo.profile(False)
        res.append(dict(step_us=1e6 * el / K, scans_per_s=B * K / el, filter_us=1e6 * t_f / max(n_f, 1), features_us=1e6 * t_feat / max(n, 1),
                        registration_us=1e6 * t_reg / max(n, 1)))
    outer = [odo.summary(q)[0].outer_iterations for q in range(0, B, max(1, B // 128))]
    out = {"leg": name, "sequences": B, "input_sweeps_per_step": S if shared else B, "resident_input_MB_per_step": (S if shared else B) * bench.A * bench.R / 1e6,
           "steps_per_repeat": K, "repeats": reps, "outer_iterations_last_step_min_mean_max": [int(min(outer)), float(np.mean(outer)), int(max(outer))]}
    for k in res[0]:
        out[k] = float(np.median([x[k] for x in res]))
        out[k + "_all"] = [round(x[k], 1) for x in res]
    print(json.dumps(out), flush=True)
    odo.release(); ctx.close()
    del d_in, d_tmp
    torch.cuda.empty_cache()
    return out


def main():
    torch.cuda.set_stream(torch.cuda.Stream())
    from cfear_radarodometry_code_public_amd import capi, replay
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    W, K, reps = 4, 12, 3
    B = int(os.environ.get("CFEAR_GRID_B", "1536"))
    S = int(os.environ.get("CFEAR_GRID_SOURCES", "64"))
    st = bench.make_streams(S, bench.PRE_ROLL + W + K, 0)  # [S, PRE_ROLL + frames, A, R]
    d_all = torch.from_numpy(np.ascontiguousarray(st)).to(dev)
    d_pre = d_all[:, :bench.PRE_ROLL].clone()
    d_frames = d_all[:, bench.PRE_ROLL:].transpose(0, 1).contiguous()  # [frames, S, A, R]
    del d_all
    idx = torch.from_numpy(np.arange(B) % S).to(dev)  # sequence q replays recording q % S
    base = capi.default_params(range_res=bench.RANGE_RES, **bench.PARAMS)
    rows = grid_rows(capi, replay, base, B)
    ident = [base] * B
    legs = os.environ.get("CFEAR_GRID_LEGS", "a,b,c,d,e,f,g,h").split(",")
    if "a" in legs:
        leg(capi, "a_no_table", base, stream, B, S, d_frames, d_pre, idx, None, False, W, K, reps)
    if "b" in legs:
        leg(capi, "b_identity_table", base, stream, B, S, d_frames, d_pre, idx, ident, False, W, K, reps)
    if "a" in legs:
        leg(capi, "a_no_table_again", base, stream, B, S, d_frames, d_pre, idx, None, False, W, K, reps)  # (a)'s own spread between objects
    if "c" in legs:
        leg(capi, "c_grid_replicated_frames", base, stream, B, S, d_frames, d_pre, idx, rows, False, W, K, reps)
    if "d" in legs:
        leg(capi, "d_grid_shared_sources", base, stream, B, S, d_frames, d_pre, idx, rows, True, W, K, reps)
    # the kstrong_vs_cfar axis on the CFEAR-3 preset (bench.preset_legs cfear3_k40_p2p with k as the axis)
    ks = [1, 5, 10, 20, 30, 40, 50]
    cfear3 = capi.default_params(range_res=bench.RANGE_RES, **dict(bench.PARAMS, cost=0, submap_scan_size=4, res=3.0, weight_intensity=1, weight_opt=4))
    if "e" in legs:
        krows = replay.param_grid(cfear3, k_strongest=ks)
        Bk = len(ks) * S
        kidx = torch.from_numpy(np.arange(Bk) // len(ks)).to(dev)  # sequences 7 r .. 7 r + 6: the seven k of recording r
        leg(capi, "e_k_grid_shared_sources_K50", replay.grid_context_params(krows), stream, Bk, S, d_frames, d_pre, kidx, [krows[q % len(ks)] for q in range(Bk)], True,
            W, K, reps)
    if "f" in legs:
        sidx = torch.from_numpy(np.arange(S)).to(dev)
        for k in ks:
            pk = capi.Params.from_buffer_copy(cfear3)
            pk.k_strongest = k
            leg(capi, "f_uniform_object_k%d" % k, pk, stream, S, S, d_frames, d_pre, sidx, None, False, W, K, reps)
    # the submap_keyframes sweep on the CFEAR-3 preset: cost x submap_scan_size, 30 points
    srows = replay.param_grid(cfear3, cost=[0, 1, 2], submap_scan_size=range(1, 11))
    if "g" in legs:
        Bs = len(srows) * S
        gidx = torch.from_numpy(np.arange(Bs) // len(srows)).to(dev)  # sequences 30 r .. 30 r + 29: the thirty points of recording r
        cpar = replay.grid_context_params(srows)
        grows = [srows[q % len(srows)] for q in range(Bs)]
        leg(capi, "g_cost_submap_grid_shared_sources_S10", cpar, stream, Bs, S, d_frames, d_pre, gidx, grows, True, W, K, reps, shapes=replay.grid_shapes(grows, cpar))
    if "h" in legs:
        sidx = torch.from_numpy(np.arange(S)).to(dev)
        outs = [leg(capi, "h_uniform_object_cost%d_s%d" % (r.cost, r.submap_scan_size), r, stream, S, S, d_frames, d_pre, sidx, None, False, W, K, reps) for r in srows]
        total = {"leg": "h_sum_of_30_uniform_objects", "sequences": len(srows) * S, "input_sweeps_per_step": len(srows) * S,
                 "resident_input_MB_per_step": sum(o["resident_input_MB_per_step"] for o in outs)}
        for k in ("step_us", "filter_us", "features_us", "registration_us"):
            total[k] = float(sum(o[k] for o in outs))
        print(json.dumps(total), flush=True)


if __name__ == "__main__":
    main()
