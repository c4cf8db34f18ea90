# What the fuser's options cost on the batched step (cfear_odometry_set_fuser_options): BASELINE configs[1] (bench.PARAMS), CFEAR_GRID_B
# sequences (default 1536) over CFEAR_GRID_SOURCES generated recordings (default 64, shared through a source map), after bench.py's 8-sweep
# pre-roll and W warm-up steps; per leg three repeats of K timed steps, medians, the stage times from cfear_odometry_profile_read /
# _profile_read_stages and the outer-iteration counts of the last step. One JSON line per leg: the defaults, soft_constraint = 1,
# use_guess = 0, both, and the defaults again (the spread between two objects).
# usage: python tools/gpu_fuser_options.py > profiles/fuser_options_steps.jsonl
import json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench


def leg(capi, name, base, stream, B, S, d_frames, d_pre, idx, options, W, K, reps):
    ctx = capi.Context(base, bench.A, bench.R, device=0, stream=stream)
    odo = ctx.odometry(B)
    odo.set_sequence_sources(idx.cpu().numpy().astype(np.int32), S)
    if options is not None:
        odo.set_fuser_options(options)
    frames = d_frames.shape[0]
    period = 2 * (frames - 1)
    frame_of = lambda s: (s % period) if (s % period) < frames else period - (s % period)  # forwards, then backwards (bench.Resident.frame_of)
    for t in range(bench.PRE_ROLL):
        src = d_pre[:, t].contiguous()
        torch.cuda.current_stream().synchronize()
        odo.step_device(src.data_ptr())
        ctx.synchronize()
    step = 0
    for _ in range(W):
        odo.step_device(d_frames[frame_of(step)].data_ptr()); step += 1
    res = []
    for r in range(reps):
        ctx.synchronize(); torch.cuda.synchronize()
        odo.profile(True)
        t0 = time.perf_counter()
        for _ in range(K):
            odo.step_device(d_frames[frame_of(step)].data_ptr()); step += 1
        ctx.synchronize(); torch.cuda.synchronize()
        el = time.perf_counter() - t0
        t_f, n_f = odo.profile_read()
        t_feat, t_reg, n = odo.profile_read_stages()
        odo.profile(False)
        res.append(dict(step_us=1e6 * el / K, scans_per_s=B * K / el, filter_us=1e6 * t_f / max(n_f, 1), features_us=1e6 * t_feat / max(n, 1),
                        registration_us=1e6 * t_reg / max(n, 1)))
    summ = [odo.summary(q)[0] for q in range(0, B, max(1, B // 128))]
    outer = [s.outer_iterations for s in summ]
    inner = [sum(s.inner_iterations[:min(max(s.outer_iterations, 0), 8)]) for s in summ]
    out = {"leg": name, "sequences": B, "input_sweeps_per_step": S, "steps_per_repeat": K, "repeats": reps,
           "outer_iterations_last_step_min_mean_max": [int(min(outer)), float(np.mean(outer)), int(max(outer))],
           "inner_iterations_last_step_mean": float(np.mean(inner))}
    for k in res[0]:
        out[k] = float(np.median([x[k] for x in res]))
        out[k + "_all"] = [round(x[k], 1) for x in res]
    print(json.dumps(out), flush=True)
    odo.release(); ctx.close()


def main():
    torch.cuda.set_stream(torch.cuda.Stream())
    from cfear_radarodometry_code_public_amd import capi
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
    for name, opt in (("defaults", None), ("soft_constraint", capi.FuserOptions(1, 1)), ("no_guess", capi.FuserOptions(0, 0)),
                      ("soft_no_guess", capi.FuserOptions(1, 0)), ("defaults_again", None)):
        leg(capi, name, base, stream, B, S, d_frames, d_pre, idx, opt, W, K, reps)


if __name__ == "__main__":
    main()
