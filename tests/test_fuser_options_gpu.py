"""The fuser's soft_constraint and use_guess (odometrykeyframefuser.h:94; odometrykeyframefuser.cpp:165-168, :186) on the batched
odometry routes, per object and per sequence (cfear_odometry_set_fuser_options).

Device against the reference fuser composed from the oracle's per-call pieces (tests/fuser_ref.py) at the project's bar: outer / inner
iteration counts, residual, keyframe and cell counts equal and the pose within 1e-4 m / 1e-5 rad at EVERY sweep of EVERY sequence;
device against device bit for bit. tests/test_fuser_options_cpu.py shows on the reference alone that either switch moves these drives'
trajectories by more than ten times that bar. Twelve sweeps form four keyframes on the free runs; under the soft prior (identity
covariance, weight sqrt(cells)) the reference's P2L trajectory is held near its guesses and forms three - the full keyframe ring under
soft is covered by the large-submap case (every sweep a keyframe) and by the rows of the parameter-table case."""
import subprocess

import numpy as np
import pytest

import fuser_ref as fr
import test_param_grid_gpu as pg
from cfear_radarodometry_code_public_amd import capi

pytestmark = pytest.mark.gpu

A, R, RR = fr.A, fr.R, fr.RR
T = fr.T_SWEEPS
FIELDS = ("pose", "final_cost", "outer_iterations", "num_residuals", "n_keyframes", "n_cells", "inner_iterations")


def opts_of(pairs):
    return [capi.FuserOptions(s, g) for s, g in pairs]


def make(kw, B, options=None, tune=(), odo_kw=None, rows=None, source=None):
    ctx = capi.Context(capi.default_params(**kw), A, R)
    for k, v in tune:
        ctx.tune(k, v)
    odo = ctx.odometry(B, **(odo_kw or {}))
    if rows is not None:
        odo.set_sequence_params([capi.default_params(**r) for r in rows])
    if source is not None:
        odo.set_sequence_sources(*source)
    if options is not None:
        odo.set_fuser_options(options)
    return ctx, odo


def step_records(odo, frames):
    """the step route sweep by sweep -> what a replay records, [T, B] of SWEEP_RECORD_DTYPE"""
    n = frames.shape[0]
    rec = np.zeros((n, odo.B), dtype=capi.SWEEP_RECORD_DTYPE)
    for t in range(n):
        odo.step_host(frames[t])
        poses = odo.poses()
        for q in range(odo.B):
            S, nc, nk = odo.summary(q)
            r = rec[t, q]
            r["pose"], r["final_cost"], r["outer_iterations"], r["num_residuals"] = poses[q], S.final_cost, S.outer_iterations, S.num_residuals
            r["n_keyframes"], r["n_cells"], r["inner_iterations"] = nk, nc, list(S.inner_iterations[:8])
    return rec


def as_runs(rec):
    """records -> [sequence][sweep] (counts, pose) as fuser_ref.run gives them"""
    out = []
    for q in range(rec.shape[1]):
        rows = []
        for r in rec[:, q]:
            no = min(max(int(r["outer_iterations"]), 0), 8)
            rows.append(((int(r["outer_iterations"]), [int(v) for v in r["inner_iterations"][:no]], int(r["num_residuals"]), int(r["n_keyframes"]), int(r["n_cells"])),
                         np.array(r["pose"])))
        out.append(rows)
    return out


def same(a, b, what):
    for f in FIELDS:
        assert np.array_equal(a[f], b[f]), (what, f)


def drive_of(q):
    return (q + q // len(fr.SEQS)) % len(fr.SEQS)  # (a second group of four sequences sees the drives shifted by one)


def frames_for(B):
    all4 = fr.frames_of()
    return np.ascontiguousarray(all4[:, [drive_of(q) for q in range(B)]])


# ---- 1. every option pair, every cost ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cost", ["P2L", "P2D", "P2P"])
@pytest.mark.parametrize("soft,guess", [(1, 1), (0, 0), (1, 0)])
def test_every_option_pair_matches_the_reference_fuser(oracle, cost, soft, guess):
    B, kw = 4, fr.COSTS[cost]
    ctx, odo = make(kw, B, capi.FuserOptions(soft, guess))
    for q in range(B):
        o = odo.fuser_options(q)
        assert (o.soft_constraint, o.use_guess) == (soft, guess)
    rec = step_records(odo, frames_for(B))
    odo.release(); ctx.close()
    exp = [fr.reference(oracle, cost, kw, fr.SEQS[drive_of(q)], soft, guess) for q in range(B)]
    pg.assert_at_the_bar(as_runs(rec), exp, "%s soft %d guess %d" % (cost, soft, guess))
    assert exp[0][-1][0][2] > 50  # residuals: the registrations have something to work on


# ---- 2. mixed rows ----------------------------------------------------------------------------------------------------------------------
def test_mixed_rows_match_the_reference_and_uniform_objects_bit_for_bit(oracle):
    B, kw = 8, fr.COSTS["P2L"]
    pairs = [fr.OPTIONS[q % 4] for q in range(B)]
    frames = frames_for(B)
    ctx, odo = make(kw, B, opts_of(pairs))
    mixed = step_records(odo, frames)
    odo.release(); ctx.close()
    exp = [fr.reference(oracle, "P2L", kw, fr.SEQS[drive_of(q)], *pairs[q]) for q in range(B)]
    pg.assert_at_the_bar(as_runs(mixed), exp, "mixed rows")
    for pair in fr.OPTIONS:
        ctx, odo = make(kw, B, capi.FuserOptions(*pair))
        uni = step_records(odo, frames)
        odo.release(); ctx.close()
        for q in range(B):
            if pairs[q] == pair:
                same(mixed[:, q], uni[:, q], ("uniform", pair, q))
    ctx, odo = make(kw, B)  # the call never made
    plain = step_records(odo, frames)
    odo.release(); ctx.close()
    for q in range(B):
        if pairs[q] == (0, 1):
            same(mixed[:, q], plain[:, q], ("never called", q))
    # and the rows do differ from one another on the device, as they do in the reference
    assert np.abs(mixed["pose"][:, 1, :2] - plain["pose"][:, 1, :2]).max() > 1e-3


# ---- 3. the routes agree bit for bit ----------------------------------------------------------------------------------------------------
def test_routes_agree_bit_for_bit(oracle):
    import torch
    B, kw = 4, fr.COSTS["P2L"]
    pairs = fr.OPTIONS
    frames = frames_for(B)
    ctx, odo = make(kw, B, opts_of(pairs))
    step = step_records(odo, frames)
    odo.release(); ctx.close()
    pg.assert_at_the_bar(as_runs(step), [fr.reference(oracle, "P2L", kw, fr.SEQS[drive_of(q)], *pairs[q]) for q in range(B)], "step")
    for persistent_max in (256, 0):  # the persistent chunk kernel; two launches per sweep
        ctx, odo = make(kw, B, opts_of(pairs), tune=[(capi.TUNE_REPLAY_PERSISTENT_MAX, persistent_max)])
        same(odo.replay_host(frames), step, ("replay_host", persistent_max))
        # reset keeps the options: the same records again
        odo.reset()
        same(odo.replay_host(frames), step, ("replay_host after reset", persistent_max))
        odo.release(); ctx.close()
    ctx, odo = make(kw, B, opts_of(pairs))
    d_frames = torch.from_numpy(frames).cuda()
    d_rec = torch.zeros((T, B, capi.SWEEP_RECORD_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    odo.replay_device(d_frames, T, d_rec)
    ctx.synchronize(); torch.cuda.synchronize()
    same(d_rec.cpu().numpy().view(capi.SWEEP_RECORD_DTYPE).reshape(T, B), step, "replay_device")
    odo.release(); ctx.close()
    ctx, odo = make(kw, B, opts_of(pairs), odo_kw=dict(overlap=2))  # ODOMETRY_OVERLAP streams
    same(step_records(odo, frames), step, "overlap 2")
    odo.release(); ctx.close()


CFAR = dict(window_size=40, nb_guard_cells=10, false_alarm_rate=0.01)


@pytest.mark.parametrize("overlap", [0, 2])
def test_cfar_object_and_cloud_step_agree_under_soft(oracle, overlap):
    import torch
    B, Tc = 2, 10
    kw = dict(fr.BASE, z_min=20.0, cost=fr.P2P, weight_intensity=0)
    hp = dict(kw, filter_type=capi.FILTER_CACFAR, cfar_window_size=40, cfar_nb_guard_cells=10, cfar_false_alarm_rate=0.01)
    frames = frames_for(B)[:Tc]
    pairs = [(1, 1), (1, 0)]
    ctx, odo = make(hp, B, opts_of(pairs), odo_kw=dict(overlap=overlap))
    built_in = step_records(odo, frames)
    odo.release()
    odo2 = ctx.odometry(B, overlap=overlap)
    odo2.set_fuser_options(opts_of(pairs))
    cap = 32768
    d_xyi = torch.empty((B, cap, 3), dtype=torch.float32, device="cuda")
    d_n = torch.empty((B,), dtype=torch.int32, device="cuda")
    for t in range(Tc):
        d_img = torch.from_numpy(frames[t]).cuda()
        torch.cuda.synchronize()
        ctx.filter_cfar_batch(d_img.data_ptr(), B, d_xyi.data_ptr(), cap, d_n.data_ptr(), **CFAR)
        odo2.step_cloud_device(d_xyi.data_ptr(), cap, d_n.data_ptr())
        assert np.array_equal(odo2.poses(), built_in["pose"][t]), t
        for q in range(B):
            S = odo2.summary(q)[0]
            assert (S.final_cost, S.num_residuals, S.outer_iterations) == (built_in["final_cost"][t, q], built_in["num_residuals"][t, q], built_in["outer_iterations"][t, q])
    odo2.release(); ctx.close()
    if overlap == 0:
        exp = [fr.run(oracle, kw, frames[:, q], *pairs[q], cfar=CFAR) for q in range(B)]
        pg.assert_at_the_bar(as_runs(built_in), exp, "CA-CFAR soft")


# ---- 4. the large-submap kernel -----------------------------------------------------------------------------------------------------------
def test_large_submap_kernels_under_soft(oracle):
    B = 4
    kw = dict(fr.COSTS["P2L"], submap_scan_size=8, use_keyframe=0)  # every sweep is a keyframe: nine scans from the ninth sweep on
    pairs = [(1, 1), (1, 0), (1, 1), (0, 0)]
    frames = frames_for(B)
    recs = {}
    for large in (1, 2):  # the 256-thread shape compiled for 64 scans; register_step_large.hip
        ctx, odo = make(kw, B, opts_of(pairs), odo_kw=dict(large_kernel=large))
        recs[large] = step_records(odo, frames)
        odo.release(); ctx.close()
    exp = [fr.run(oracle, kw, frames[:, q], *pairs[q]) for q in range(B)]
    for large in (1, 2):
        pg.assert_at_the_bar(as_runs(recs[large]), exp, "large kernel %d" % large)
    assert exp[0][-1][0][3] == 8
    for f in ("outer_iterations", "num_residuals", "n_keyframes", "n_cells", "inner_iterations"):
        assert np.array_equal(recs[1][f], recs[2][f]), f
    d = np.abs(recs[1]["pose"] - recs[2]["pose"])
    assert d[..., :2].max() < 1e-4 and d[..., 2].max() < 1e-5, d.max()


# ---- 5. with a parameter table and a source map -------------------------------------------------------------------------------------------
def test_options_with_parameter_table_and_source_map(oracle):
    B = 8
    rows = pg.rows_for(fr.BASE)[:B]  # res, loss, z_min, weights, compensation differ between the rows
    pairs = [fr.OPTIONS[(q + 1) % 4] for q in range(B)]
    one = fr.drive(*fr.SEQS[0])
    frames = np.ascontiguousarray(one[:, None])
    ctx, odo = make(fr.BASE, B, opts_of(pairs), rows=rows, source=(np.zeros(B, dtype=np.int32), 1))
    rec = odo.replay_host(frames)
    odo.release(); ctx.close()
    exp = [fr.run(oracle, rows[q], one, *pairs[q]) for q in range(B)]
    pg.assert_at_the_bar(as_runs(rec), exp, "table + map + options")
    for q in range(B):  # each row alone: an object of one sequence under that row's parameters and options
        ctx, odo = make(fr.BASE, 1, opts_of([pairs[q]]), rows=[rows[q]])
        alone = odo.replay_host(frames)
        odo.release(); ctx.close()
        same(rec[:, q], alone[:, 0], ("alone", q))


# ---- 6. covariances -----------------------------------------------------------------------------------------------------------------------
def test_covariances_and_cost_sampling_under_soft(oracle):
    B, kw = 4, fr.COSTS["P2L"]
    pairs = [(1, 1), (1, 0), (1, 1), (0, 1)]
    frames = frames_for(B)
    objs = [make(kw, B, opts_of(pairs)) for _ in range(2)]
    objs[1][1].set_cov_sampling(True, 0.4, 0.0043625, 3, 4.0)
    fus = []
    for q in range(B):
        p = oracle.default_params(**kw)
        fus.append([fr.Fuser(oracle, p, *pairs[q]), fr.Fuser(oracle, p, *pairs[q])])
        fus[q][1].set_cov_sampling(True, 0.4, 0.0043625, 3, 4.0)
    sampled = 0
    for t in range(T):
        for _, odo in objs:
            odo.step_host(frames[t])
        cov_reg, cov_smp = objs[0][1].covariances(), objs[1][1].covariances()
        assert np.array_equal(objs[0][1].poses(), objs[1][1].poses())
        for q in range(B):
            for f in fus[q]:
                f.process_polar(frames[t, q])
            if t == 0:
                continue
            # the registration covariance of the sweep: GetCovariance with the prior block and the soft final_cost / num_residuals
            e = fus[q][0].cov_current
            print("sweep %d seq %d: covariance rel diff %.2e" % (t, q, np.abs(cov_reg[q] - e).max() / np.abs(e).max()))
            assert np.allclose(cov_reg[q], e, rtol=1e-6, atol=1e-12), (t, q)  # (tests/test_getcost_gpu.py: cfear_register_soft's covariance)
            # the sampled costs are GetCost without the prior; the scaler is the soft summary's
            costs, ok = objs[1][1].cov_samples(q)
            assert np.allclose(costs, fus[q][1].costs, rtol=1e-10, atol=1e-10), (t, q)
            assert ok == fus[q][1].cov_sampled
            assert np.allclose(cov_smp[q], fus[q][1].cov_current, rtol=1e-5, atol=1e-12), (t, q)  # (tests/test_odometry_cov_sampling_gpu.py)
            sampled += int(ok)
            if pairs[q][0]:
                S = objs[0][1].summary(q)[0]
                assert S.num_residuals == S.num_residual_blocks + 3  # P2L: one residual per block, and the prior's three
    assert sampled >= 1
    for ctx, odo in objs:
        odo.release(); ctx.close()


# ---- 7. surfaces --------------------------------------------------------------------------------------------------------------------------
def _eq_nan(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def test_surfaces_of_soft_sequences_carry_the_prior():
    B = 4
    kw = dict(fr.COSTS["P2L"], weight_opt=4, use_keyframe=0, compensate=0, submap_scan_size=3)  # (the scans are the filtered clouds of the last sweeps)
    pairs = [(1, 1), (0, 1), (1, 0), (0, 0)]
    frames = frames_for(B)[:6]
    ctx, odo = make(kw, B, opts_of(pairs))
    ctx0, odo0 = make(kw, B)
    odo.set_surface_recording(True); odo0.set_surface_recording(True)
    for t in range(frames.shape[0]):
        odo.step_host(frames[t]); odo0.step_host(frames[t])
        if t not in (1, 5):
            continue
        s, n_used, itr_used, poses_used = odo.surface(0.05, 1, details=True)
        s = s.cpu().numpy()
        s0 = odo0.surface(0.05, 1).cpu().numpy()
        for q in range(B):
            n = int(n_used[q])
            assert n == min(t + 1, 4)
            dsc = [ctx.scan_create(ctx.filter_polar(frames[t - n + 1 + i, q], peaks=False)[0]) for i in range(n)]
            with_prior = ctx.get_surface(dsc, poses_used[q, :n], 0.05, 1, itr=int(itr_used[q]), prior_cov6=np.eye(6))
            without = ctx.get_surface(dsc, poses_used[q, :n], 0.05, 1, itr=int(itr_used[q]))
            m = ~np.isnan(without)
            print("sweep %d seq %d soft %d: |surface - with prior| %.3g, |surface - without| %.3g" %
                  (t, q, pairs[q][0], np.abs(s[q][m] - with_prior[m]).max(), np.abs(s[q][m] - without[m]).max()))
            if pairs[q][0]:
                assert _eq_nan(s[q], with_prior), (t, q)
                assert not _eq_nan(s[q], without) and np.abs(s[q][m] - without[m]).max() > 1e-3
            else:
                assert _eq_nan(s[q], without), (t, q)
        assert _eq_nan(s[1], s0[1])  # the (0, 1) sequence: the object the call was never made on
    odo.release(); ctx.close(); odo0.release(); ctx0.close()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_setting_untouched():
    B = 4
    ctx, odo = make(fr.BASE, B)
    assert [(odo.fuser_options(q).soft_constraint, odo.fuser_options(q).use_guess) for q in range(B)] == [(0, 1)] * B
    pairs = [(1, 1), (0, 0), (1, 0), (0, 1)]
    odo.set_fuser_options(opts_of(pairs))

    def current():
        return [(odo.fuser_options(q).soft_constraint, odo.fuser_options(q).use_guess) for q in range(B)]

    assert current() == pairs
    with pytest.raises(capi.CfearError, match=r"rc=-1.*row 2.*use_guess = 2"):
        odo.set_fuser_options(opts_of([(0, 1), (1, 1), (1, 2), (0, 1)]))
    with pytest.raises(capi.CfearError, match=r"rc=-1.*row 0.*soft_constraint = 2"):
        odo.set_fuser_options(capi.FuserOptions(2, 1))
    with pytest.raises(capi.CfearError, match=r"rc=-1.*row 1.*soft_constraint = -1"):
        odo.set_fuser_options(opts_of([(0, 1), (-1, 1), (1, 1), (0, 1)]))
    for n in (2, 3, 5):
        with pytest.raises(capi.CfearError, match=r"rc=-1.*n_rows = %d" % n):
            odo.set_fuser_options(opts_of([(1, 1)] * n))
    assert current() == pairs
    with pytest.raises(capi.CfearError):
        odo.fuser_options(B)
    frames = frames_for(B)
    odo.step_host(frames[0])
    with pytest.raises(capi.CfearError, match=r"rc=-1.*has processed 1 sweeps"):
        odo.set_fuser_options(capi.FuserOptions(0, 1))
    with pytest.raises(capi.CfearError, match=r"rc=-1.*has processed"):
        odo.set_fuser_options(None)
    assert current() == pairs
    odo.reset()  # keeps the setting, and allows a new one
    assert current() == pairs
    odo.set_fuser_options(capi.FuserOptions(1, 0))
    assert current() == [(1, 0)] * B
    odo.set_fuser_options(None)
    assert current() == [(0, 1)] * B
    odo.release(); ctx.close()


# ---- 9. the host tool -----------------------------------------------------------------------------------------------------------------------
def test_offline_odometry_replay_with_soft_constraint(oracle, tmp_path):
    import test_host_cpp
    exe = test_host_cpp.build_harness()
    imgs = fr.drive(*fr.SEQS[0])[:8]
    f = tmp_path / "sweeps.u8"
    imgs.tofile(f)
    est = {}
    for mode in ("0", "1"):
        d = tmp_path / ("m" + mode)
        d.mkdir()
        args = [exe, "--frames", str(f), "--range-res", "0.0595238", "--res", "3.0", "--submap_scan_size", "4", "--z-min", "60",
                "--weight_option", "0", "--est_directory", str(d), "--replay", mode, "--soft_constraint", "1"]
        r = subprocess.run(args, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        est[mode] = np.loadtxt(d / "est_00.txt")
    assert est["0"].shape == est["1"].shape == (8, 12)
    exp = fr.reference(oracle, "P2L", fr.COSTS["P2L"], fr.SEQS[0], 1, 1)
    free = fr.reference(oracle, "P2L", fr.COSTS["P2L"], fr.SEQS[0], 0, 1)
    for mode in ("0", "1"):
        for t in range(8):
            got = np.array([est[mode][t, 3], est[mode][t, 7], np.arctan2(est[mode][t, 4], est[mode][t, 0])])
            e = exp[t][1]
            assert np.all(np.abs(got[:2] - e[:2]) < 1e-4 + 5e-7) and abs(got[2] - e[2]) < 1e-5 + 2e-6, (mode, t, got, e)  # (+: 6-decimal KITTI text)
    assert np.abs(exp[7][1][:2] - free[7][1][:2]).max() > 1e-3  # and that is not the trajectory without the prior
    # the non-Oxford refusal stays
    r = subprocess.run([exe, "--frames", str(f), "--est_directory", str(tmp_path), "--replay", "1", "--dataset", "mulran"], capture_output=True, text=True)
    assert r.returncode != 0 and "Oxford" in r.stderr
