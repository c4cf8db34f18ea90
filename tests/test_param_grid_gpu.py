"""Parameter grids in one batch (cfear_odometry_set_sequence_params / _set_sequence_sources): every sequence of a batched odometry
object under its own parameter set, several sequences reading one sweep - the reference's evaluation grids (utils/worker:26-99, one
offline_odometry process per point) as the sequences of one object.

Device against the oracle at the project's bar: outer / inner iteration counts, residual, keyframe and cell counts equal and the pose
within 1e-4 m / 1e-5 rad at EVERY sweep of EVERY row; device against device bit for bit. No sweep and no row is exempt."""
import numpy as np
import pytest

from cfear_radarodometry_code_public_amd import capi, synth

pytestmark = pytest.mark.gpu

A, R, RR = 400, 3360, np.float32(0.0595238)
P2P, P2L, P2D = 0, 1, 2
NONE, HUBER, CAUCHY, SOFTLONE, TUKEY = 0, 1, 2, 3, 5
BASE = dict(range_res=RR, k_strongest=12, z_min=60.0, res=3.0, weight_intensity=1, weight_opt=0, compensate=1, radar_ccw=0, cost=P2L, loss=HUBER,
            loss_limit=0.1, covar_scale=1.0, regularization=1.0, submap_scan_size=4)
# rows drawn from the reference's grids (params/loss_function, weight_residual, resolution, grid_search, motion_compensation). Row 0 is the
# base; rows 1, 2, 3 differ from it in ONE field each (res / compensation / loss) for the 'not one code path' assertion
ROWS = [
    dict(),
    dict(res=5.0),
    dict(compensate=0),
    dict(loss=CAUCHY, loss_limit=0.01),
    dict(loss=NONE, weight_opt=1, res=2.5, z_min=50.0),
    dict(loss=SOFTLONE, loss_limit=4.0, weight_opt=3, res=3.5, z_min=70.0, weight_intensity=0),
    dict(loss=TUKEY, loss_limit=0.5, weight_opt=4, z_min=70.0, min_keyframe_dist=0.5),
    dict(loss=HUBER, loss_limit=1.0, weight_opt=5, res=2.5, compensate=0, weight_intensity=0),
    dict(loss=CAUCHY, loss_limit=0.2, weight_opt=2, res=3.5, z_min=50.0, min_keyframe_dist=3.0),
    dict(loss=TUKEY, loss_limit=2.0, weight_opt=4, res=5.0, z_min=50.0, max_itr_association=4, min_itr=2),
    dict(loss=NONE, weight_opt=2, res=2.5, z_min=70.0, max_solver_iterations=5),
    dict(loss=SOFTLONE, loss_limit=0.3, weight_opt=1, z_min=50.0, compensate=0, use_keyframe=0),
]
P2D_EXTRA = [dict(), dict(regularization=0.1), dict(covar_scale=2.0), dict(regularization=0.1, covar_scale=0.5)]


def rows_for(base, extra=None):
    out = []
    for i, r in enumerate(ROWS):
        kw = dict(base)
        kw.update(r)
        if extra:
            kw.update(extra[i % len(extra)])
        out.append(kw)
    return out


_DRIVES = {}


def drive(kind, T, world_seed=10, seed=20):
    key = (kind, T, world_seed, seed)
    if key not in _DRIVES:
        fr = np.empty((T, A, R), dtype=np.uint8)
        for t0, chunk in synth.drive_chunks(T, kind, world_seed, seed, A, R, RR, ccw=False):
            fr[t0:t0 + len(chunk)] = chunk
        _DRIVES[key] = fr
    return _DRIVES[key]


def _counts_o(fu):
    S = fu.last_summary()
    no = max(int(S.outer_iterations), 0)
    return (int(S.outer_iterations), [int(v) for v in S.inner_iterations[:min(no, 8)]], int(S.num_residuals), int(fu.num_keyframes), len(fu.last_cells()))


def oracle_run(oracle, rows, frames_of_row, cfar=None):
    """-> [row][sweep] (counts, pose) of the oracle's fuser under each row's own parameters"""
    out = []
    for q, kw in enumerate(rows):
        fu = oracle.Fuser(oracle.default_params(**kw))
        res = []
        for img in frames_of_row(q):
            if cfar:
                e = fu.process_cloud(oracle.cfar(img, float(np.float32(kw["range_res"])), float(kw["z_min"]), 2.5, **cfar))
            else:
                e = fu.process_polar(img)
            res.append((_counts_o(fu), np.array(e)))
        out.append(res)
    return out


def make_object(ctx_kw, rows, source=None, n_sources=None, tune=(), persistent_max=None, odo_kw=None):
    ctx = capi.Context(capi.default_params(**ctx_kw), A, R)
    for k, v in tune:
        ctx.tune(k, v)
    if persistent_max is not None:
        ctx.tune(capi.TUNE_REPLAY_PERSISTENT_MAX, persistent_max)
    odo = ctx.odometry(len(rows), **(odo_kw or {}))
    if rows:
        odo.set_sequence_params([capi.default_params(**kw) for kw in rows])
    if source is not None:
        odo.set_sequence_sources(source, n_sources)
    return ctx, odo


def device_run(odo, frames, route):
    """frames [T, n_sources, A, R] -> [sequence][sweep] (counts, pose)"""
    T, B = frames.shape[0], odo.B
    out = [[] for _ in range(B)]
    if route == "step":
        for t in range(T):
            odo.step_host(frames[t])
            got = odo.poses()
            for q in range(B):
                S, nc, nk = odo.summary(q)
                g = (int(S.outer_iterations), [int(v) for v in S.inner_iterations[:min(max(int(S.outer_iterations), 0), 8)]], int(S.num_residuals), nk, nc)
                out[q].append((g, np.array(got[q])))
    else:
        recs = odo.replay_host(frames)
        for t in range(T):
            for q in range(B):
                r = recs[t, q]
                g = (int(r["outer_iterations"]), [int(v) for v in r["inner_iterations"][:min(max(int(r["outer_iterations"]), 0), 8)]], int(r["num_residuals"]),
                     int(r["n_keyframes"]), int(r["n_cells"]))
                out[q].append((g, np.array(r["pose"])))
    return out


def assert_at_the_bar(dev, exp, what):
    for q in range(len(exp)):
        assert len(dev[q]) == len(exp[q])
        for t, ((g, pose), (e, ep)) in enumerate(zip(dev[q], exp[q])):
            print("%s row %d sweep %d: counts %r / %r, pose diff %.2e m %.2e rad" % (what, q, t, g, e, np.abs(pose[:2] - ep[:2]).max(), abs(pose[2] - ep[2])))
            if t > 0:
                assert g == e, (what, q, t, g, e)
            else:
                assert g[4] == e[4], (what, q, t, g, e)  # (the first sweep registers nothing: its cell count)
            assert np.all(np.abs(pose[:2] - ep[:2]) < 1e-4) and abs(pose[2] - ep[2]) < 1e-5, (what, q, t, pose, ep)


def assert_not_one_code_path(dev):
    traj = [np.array([p for _, p in d]) for d in dev]
    for q in (1, 2, 3):  # res / compensation / loss alone
        assert np.abs(traj[q][:, :2] - traj[0][:, :2]).max() > 1e-3, q


PERSISTENT = {"step": None, "replay": 0, "persistent": 256}
_ORACLE = {}


def oracle_rows(oracle, name, rows, frames):
    if name not in _ORACLE:
        _ORACLE[name] = oracle_run(oracle, rows, lambda q: frames)
    return _ORACLE[name]


# ---- 2. identity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["step", "replay", "persistent"])
def test_identity_table_and_map_change_nothing(route):
    T, B = 24, 3
    frames = np.ascontiguousarray(np.stack([drive("canyon", T, 10 + q, 20 + q) for q in range(B)], axis=1))
    outs = []
    for with_table in (False, True):
        ctx = capi.Context(capi.default_params(**BASE), A, R)
        if PERSISTENT[route] is not None:
            ctx.tune(capi.TUNE_REPLAY_PERSISTENT_MAX, PERSISTENT[route])
        odo = ctx.odometry(B)
        odo.set_cov_sampling(True, samples_per_axis=3)
        if with_table:
            odo.set_sequence_params([capi.default_params(**BASE)] * B)
            odo.set_sequence_sources(np.arange(B, dtype=np.int32), B)
        if route == "step":
            res = []
            for t in range(T):
                odo.step_host(frames[t])
                res.append((odo.poses().tobytes(), odo.covariances().tobytes(), b"".join(bytes(odo.summary(q)[0]) for q in range(B))))
        else:
            rec, cov = odo.replay_host(frames, covariances=True)
            res = (rec.tobytes(), cov.tobytes(), odo.poses().tobytes())
        outs.append(res)
        odo.release(); ctx.close()
    assert outs[0] == outs[1]


# ---- 3. mixed grid against the oracle --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cost,route,kind", [(P2L, "step", "blocks"), (P2P, "replay", "canyon"), (P2D, "persistent", "blocks"),
                                             (P2L, "persistent", "canyon"), (P2P, "step", "blocks"), (P2D, "replay", "canyon")])
def test_mixed_grid_matches_the_oracle_row_by_row(oracle, cost, route, kind):
    T = 60
    base = dict(BASE, cost=cost)
    rows = rows_for(base, P2D_EXTRA if cost == P2D else None)
    frames = drive(kind, T)
    exp = oracle_rows(oracle, "mixed %d %s" % (cost, kind), rows, frames)
    ctx, odo = make_object(base, rows, np.zeros(len(rows), dtype=np.int32), 1, persistent_max=PERSISTENT[route])
    for q, kw in enumerate(rows):
        got = odo.sequence_params(q)
        assert (got.res, got.loss, got.z_min, got.weight_opt) == (kw["res"], kw["loss"], kw["z_min"], kw["weight_opt"])
    dev = device_run(odo, frames[:, None], route)
    odo.release(); ctx.close()
    assert_at_the_bar(dev, exp, "mixed cost %d %s" % (cost, route))
    assert_not_one_code_path(dev)


def test_mixed_grid_ten_keyframes_large_submap_kernel(oracle):
    T = 70
    base = dict(BASE, cost=P2L, submap_scan_size=10, min_keyframe_dist=0.3)
    rows = rows_for(base)
    for r in rows:
        r["min_keyframe_dist"] = min(r["min_keyframe_dist"], 0.5)
    frames = drive("blocks", T)
    exp = oracle_rows(oracle, "ten keyframes", rows, frames)
    assert max(e[0][3] for e in exp[0]) == 10  # the ring really fills
    ctx, odo = make_object(base, rows, np.zeros(len(rows), dtype=np.int32), 1, odo_kw=dict(large_kernel=2))
    dev = device_run(odo, frames[:, None], "step")
    odo.release(); ctx.close()
    assert_at_the_bar(dev, exp, "ten keyframes")


@pytest.mark.parametrize("what", ["order_overlap", "tie_rule"])
def test_mixed_grid_sequence_workgroup_indirections_and_tie_rule(oracle, what):
    T = 60
    base = dict(BASE, cost=P2L)
    rows = rows_for(base)
    frames = drive("blocks", T)
    if what == "order_overlap":
        # The order[] indirection applies to whole-batch registration launches only (launch_register_kernel): with overlap 2 the sequences run
        # as two ranges (seq0 + blockIdx.x per range) and no order is used, whatever REGISTRATION_ORDER says. So the first object covers the
        # overlap ranges, the second (overlap 0) order[blockIdx.x]; no single object runs both.
        exp = oracle_rows(oracle, "mixed %d %s" % (P2L, "blocks"), rows, frames)
        ctx, odo = make_object(base, rows, np.zeros(len(rows), dtype=np.int32), 1, odo_kw=dict(reg_order=1, overlap=2))
        dev = device_run(odo, frames[:, None], "step")
        odo.release(); ctx.close()
        assert_at_the_bar(dev, exp, "ODOMETRY_OVERLAP 2 (ranges)")
        ctx, odo = make_object(base, rows, np.zeros(len(rows), dtype=np.int32), 1, odo_kw=dict(reg_order=1, overlap=0))
        dev = device_run(odo, frames[:, None], "step")
        odo.release(); ctx.close()
        assert_at_the_bar(dev, exp, "REGISTRATION_ORDER (order[])")
    else:
        oracle.set_perturbation(["nn_tie_high"])  # the oracle's twin of rule 1 (tests/test_tie_rule_gpu.py); process-wide
        try:
            exp = oracle_run(oracle, rows, lambda q: frames)
        finally:
            oracle.set_perturbation(0)
        ctx, odo = make_object(base, rows, np.zeros(len(rows), dtype=np.int32), 1, tune=[(capi.TUNE_NN_TIE_RULE, 1)])
        dev = device_run(odo, frames[:, None], "step")
        odo.release(); ctx.close()
        assert_at_the_bar(dev, exp, "NN_TIE_RULE 1")


def test_mixed_grid_ca_cfar_object(oracle):
    T = 60
    cf = dict(window_size=10, nb_guard_cells=20, false_alarm_rate=0.01)
    base = dict(BASE, cost=P2L, z_min=20.0)
    rows = [dict(r, z_min=20.0) for r in rows_for(base)]  # (the detector's static threshold is the object's)
    frames = drive("canyon", T)
    exp = oracle_run(oracle, rows, lambda q: frames, cfar=cf)
    hip = dict(filter_type=capi.FILTER_CACFAR, cfar_window_size=10, cfar_nb_guard_cells=20, cfar_false_alarm_rate=0.01)
    ctx, odo = make_object(dict(base, **hip), [dict(r, **hip) for r in rows])
    out = [[] for _ in rows]
    for t in range(T):
        odo.step_host(np.ascontiguousarray(np.broadcast_to(frames[t], (len(rows), A, R))))
        got = odo.poses()
        for q in range(len(rows)):
            S, nc, nk = odo.summary(q)
            g = (int(S.outer_iterations), [int(v) for v in S.inner_iterations[:min(max(int(S.outer_iterations), 0), 8)]], int(S.num_residuals), nk, nc)
            out[q].append((g, np.array(got[q])))
    with pytest.raises(capi.CfearError, match="rc=-1"):
        odo.set_sequence_sources(np.zeros(len(rows), dtype=np.int32), 1)  # (not fresh any more; a fresh CA-CFAR object: test_refusals)
    odo.release(); ctx.close()
    assert_at_the_bar(out, exp, "CA-CFAR")


# ---- 4. independence -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["step", "replay"])
def test_a_row_does_not_depend_on_its_neighbours_or_its_index(route):
    T = 40
    base = dict(BASE, cost=P2L)
    rows = rows_for(base)
    frames = drive("blocks", 60)[:T]
    ctx, odo = make_object(base, rows, np.zeros(len(rows), dtype=np.int32), 1, persistent_max=0)
    mixed = device_run(odo, frames[:, None], route)
    cov_mixed = odo.covariances()
    odo.release(); ctx.close()
    for q, kw in enumerate(rows):
        ctx = capi.Context(capi.default_params(**kw), A, R)
        ctx.tune(capi.TUNE_REPLAY_PERSISTENT_MAX, 0)
        odo = ctx.odometry(2)
        alone = device_run(odo, np.ascontiguousarray(np.stack([frames, frames], axis=1)), route)
        cov = odo.covariances()
        odo.release(); ctx.close()
        for t in range(T):
            assert mixed[q][t][0] == alone[0][t][0], (q, t)
            assert mixed[q][t][1].tobytes() == alone[0][t][1].tobytes(), (q, t, mixed[q][t][1], alone[0][t][1])
        assert cov_mixed[q].tobytes() == cov[0].tobytes(), q


# ---- 5. z_min after selection ------------------------------------------------------------------------------------------------------------
def _zmin_inputs():
    rng = np.random.default_rng(7)
    world = drive("canyon", 60)[:10]
    ties = np.where(rng.random((A, R)) < 0.02, 200, 10).astype(np.uint8)  # every return has the same intensity
    four = rng.choice(np.array([30, 55, 95, 160], dtype=np.uint8), size=(A, R), p=[0.9, 0.05, 0.03, 0.02])  # four levels: ties at every threshold
    blank = np.zeros((A, R), dtype=np.uint8)
    blank[17, 900:960] = np.linspace(30, 200, 60).astype(np.uint8)  # one bearing with a few returns on both sides of every threshold
    return {"drive": drive("blocks", 60),
            "ties": np.stack([ties, np.roll(ties, 3, axis=1), world[2], np.roll(ties, 7, axis=1), world[4], four, np.roll(four, 5, axis=1), world[7]]),
            "nearly_blank": np.stack([world[0], blank, world[2], world[3], blank, blank, world[6], world[7]])}


@pytest.mark.parametrize("name", ["drive", "ties", "nearly_blank"])
def test_per_sequence_z_min_on_one_shared_source(oracle, name):
    frames = _zmin_inputs()[name]
    base = dict(BASE, cost=P2L, z_min=90.0)  # (the context's own value is none of the smallest: the filter must take the rows' minimum)
    rows = [dict(base, z_min=z) for z in (40.0, 60.0, 90.0, 150.0)]
    exp = oracle_run(oracle, rows, lambda q: frames)
    cells = [[e[0][4] for e in r] for r in exp]
    assert cells[0] != cells[3]  # the thresholds really select different clouds
    for route in ("step", "replay", "persistent"):
        ctx, odo = make_object(base, rows, np.zeros(4, dtype=np.int32), 1, persistent_max=PERSISTENT[route])
        dev = device_run(odo, frames[:, None], route)
        odo.release(); ctx.close()
        for q in range(4):
            assert [d[0][4] for d in dev[q]] == cells[q], (route, q)  # cell counts exact, the first sweep included
        assert_at_the_bar(dev, exp, "z_min %s %s" % (name, route))


# ---- 6. shared sweeps ----------------------------------------------------------------------------------------------------------------------
SRC = np.array([0, 1, 1, 0, 1], dtype=np.int32)


def _shared_rows():
    base = dict(BASE, cost=P2L, use_keyframe=0, compensate=0, submap_scan_size=3)
    return base, [dict(base), dict(base, loss=CAUCHY, loss_limit=0.5), dict(base, loss=TUKEY, loss_limit=1.0, res=3.5), dict(base, loss=NONE, z_min=70.0),
                  dict(base, loss=SOFTLONE, loss_limit=0.3, weight_opt=4)]


@pytest.mark.parametrize("route", ["step", "replay", "persistent"])
def test_source_map_equals_replicated_frames(route):
    T = 24
    base, rows = _shared_rows()
    rec = np.ascontiguousarray(np.stack([drive("canyon", T, 10, 20), drive("canyon", T, 11, 21)], axis=1))  # [T, 2, A, R]
    outs = []
    for shared in (True, False):
        ctx, odo = make_object(base, rows, SRC if shared else None, 2 if shared else None, persistent_max=PERSISTENT[route])
        odo.set_cov_sampling(True, samples_per_axis=3)
        fr = rec if shared else np.ascontiguousarray(rec[:, SRC])
        if route == "step":
            res = []
            for t in range(T):
                odo.step_host(fr[t])
                res.append((odo.poses().tobytes(), odo.covariances().tobytes(), b"".join(bytes(odo.summary(q)[0]) for q in range(5)),
                            b"".join(odo.cov_samples(q)[0].tobytes() for q in range(5))))
        else:
            r, cov = odo.replay_host(fr, covariances=True)
            res = (r.tobytes(), cov.tobytes(), odo.poses().tobytes())
        outs.append(res)
        odo.release(); ctx.close()
    assert outs[0] == outs[1]


def test_shared_sweeps_cov_sampling_and_surfaces_against_the_oracle_per_row(oracle):
    import surface_ref
    RTOL, ATOL = 1e-5, 1e-12  # tests/test_odometry_cov_sampling_gpu.py
    T = 16
    base, rows = _shared_rows()
    rec = np.ascontiguousarray(np.stack([drive("canyon", 24, 10, 20)[:T], drive("canyon", 24, 11, 21)[:T]], axis=1))
    fus = [oracle.Fuser(oracle.default_params(**kw)) for kw in rows]
    for fu in fus:
        fu.set_cov_sampling(True, steps=3)
    ctx, odo = make_object(base, rows, SRC, 2)
    odo.set_cov_sampling(True, samples_per_axis=3)
    odo.set_surface_recording(True)
    n_sampled = [0] * 5

    def scans_of(q, t, n):  # compensation is off in these rows: the scans of a registration are exactly the filtered clouds, at the row's z_min and res
        p = oracle.default_params(**rows[q])
        return p, [oracle.Scan(oracle.cloud(oracle.filter_polar(rec[t - n + 1 + i, SRC[q]], int(rows[q]["z_min"]), 12), p.range_res, p.min_distance), p) for i in range(n)]

    for t in range(T):
        odo.step_host(rec[t])
        got, cov = odo.poses(), odo.covariances().reshape(5, 6, 6)
        _, n_used, itr_used, poses_used = odo.surface(2.0, 1, details=True)  # (what every registration used: scans, itr_, poses)
        for q in range(5):
            e = fus[q].process_polar(rec[t, SRC[q]])
            assert np.all(np.abs(got[q][:2] - e[:2]) < 1e-4) and abs(got[q][2] - e[2]) < 1e-5, (t, q)
            print("cov row %d sweep %d: max rel diff %.2e" % (q, t, np.max(np.abs(cov[q] - fus[q].last_cov()) / np.maximum(np.abs(fus[q].last_cov()), 1e-300))))
            assert np.allclose(cov[q], fus[q].last_cov(), rtol=RTOL, atol=ATOL), (t, q, cov[q], fus[q].last_cov())
            # the 27 sampled costs and the 'sampled' flag against the oracle's cov_by_sampling under the row's own loss / weights / res, on the
            # scans, poses and itr_ the registration used (as test_sampled_costs_match_the_per_call_oracle, rtol 1e-10)
            costs, sampled = odo.cov_samples(q)
            if t == 0:
                assert not sampled and int(n_used[q]) == 0
                continue
            n = int(n_used[q])
            assert n == min(t + 1, 4)
            p, osc = scans_of(q, t, n)
            S = odo.summary(q)[0]
            ok_o, cov_o, costs_o = oracle.cov_by_sampling(osc, poses_used[q, :n], p, S.final_cost, S.num_residuals, itr=int(itr_used[q]), steps=3)
            print("cov_samples row %d sweep %d: sampled %d / %d, max rel diff of the 27 costs %.2e" % (q, t, sampled, ok_o, np.max(np.abs(costs - costs_o) / np.maximum(np.abs(costs_o), 1e-300))))
            assert costs.shape == (27,) and np.allclose(costs, costs_o, rtol=1e-10, atol=1e-10), (t, q, costs, costs_o)
            assert sampled == ok_o, (t, q)
            if ok_o:
                assert np.allclose(cov[q], cov_o, rtol=RTOL, atol=ATOL), (t, q)
            n_sampled[q] += int(sampled)
        if t in (1, 7, T - 1):
            s, n_used, itr_used, poses_used = odo.surface(0.25, 1, details=True)
            s = s.cpu().numpy()
            for q in range(5):
                p = oracle.default_params(**rows[q])
                n = int(n_used[q])
                assert n == min(t + 1, 4)
                osc = [oracle.Scan(oracle.cloud(oracle.filter_polar(rec[t - n + 1 + i, SRC[q]], int(rows[q]["z_min"]), 12), p.range_res, p.min_distance), p) for i in range(n)]
                exp = surface_ref.surface(oracle, osc, poses_used[q, :n], p, int(itr_used[q]), 0.25, 1)
                m = ~np.isnan(exp)
                assert np.array_equal(np.isnan(s[q]), np.isnan(exp))
                print("surface row %d sweep %d: max rel diff %.2e" % (q, t, np.max(np.abs(s[q][m] - exp[m]) / np.maximum(np.abs(exp[m]), 1e-300))))
                assert np.all(np.abs(s[q][m] - exp[m]) <= 1e-9 * np.maximum(np.abs(exp[m]), 1e-300)), (t, q)  # tests/test_surface_gpu.py's bound for the restatement
    assert all(v >= 1 for v in n_sampled), n_sampled  # every row's covariance came from ITS sampling at least once (on this drive: at every registration)
    odo.release(); ctx.close()


def test_replay_grid_runs_the_rows_of_a_grid_over_one_recording():
    """replay.replay_grid (one recording, one source, a sequence per row, in pieces) gives each row the poses of the same rows set on an
    Odometry object directly, and the KITTI drift per row when ground truth is given"""
    from cfear_radarodometry_code_public_amd import kitti, replay
    T = 10
    frames = drive("blocks", 60)[:T]
    base = capi.default_params(**dict(BASE, cost=P2L))
    rows = replay.param_grid(base, res=[2.5, 3.5], loss=[HUBER, CAUCHY])
    assert [(r.res, r.loss) for r in rows] == [(2.5, HUBER), (2.5, CAUCHY), (3.5, HUBER), (3.5, CAUCHY)]
    gt = kitti.poses_from_xyt(np.cumsum(np.tile([[1.0, 0.0, 0.0]], (T, 1)), axis=0))
    out = replay.replay_grid(frames, rows, gt=gt, piece=4)  # (three pieces: 4 + 4 + 2 sweeps)
    assert out["poses"].shape == (T, 4, 3) and out["records"].shape == (T, 4)
    assert out["drift"] is not None and len(out["drift"]) == 4
    assert replay.replay_grid(frames[:3], rows)["drift"] is None
    ctx = capi.Context(base, A, R)
    odo = ctx.odometry(4)
    odo.set_sequence_params(rows)
    odo.set_sequence_sources(np.zeros(4, dtype=np.int32), 1)
    rec = odo.replay_host(frames[:, None])
    odo.release(); ctx.close()
    assert np.array_equal(out["poses"], rec["pose"])
    assert np.abs(out["poses"][:, 0, :2] - out["poses"][:, 2, :2]).max() > 1e-3  # res 2.5 against 3.5


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_object_unchanged_and_usable(oracle):
    T = 6
    frames = drive("blocks", 60)[:T]
    base = dict(BASE, cost=P2L)
    rows = rows_for(base)[:4]
    ctx, odo = make_object(base, rows, np.zeros(4, dtype=np.int32), 1)
    for field, v in (("k_strongest", 20), ("cost", P2P), ("submap_scan_size", 3), ("filter_type", capi.FILTER_CACFAR)):
        bad = [capi.default_params(**kw) for kw in rows]
        setattr(bad[2], field, v)
        with pytest.raises(capi.CfearError, match=r"rc=-1.*row 2.*%s" % field):
            odo.set_sequence_params(bad)
        assert odo.sequence_params(2).res == rows[2]["res"] and odo.sequence_params(1).res == rows[1]["res"]
    with pytest.raises(capi.CfearError, match="rc=-1"):
        odo.set_sequence_sources(np.array([0, 1, 2, 0], dtype=np.int32), 2)  # a source out of range
    assert odo.n_sources == 1
    with pytest.raises(capi.CfearError, match="rc=-3"):
        odo.step_cloud_device(1, 16, 1)  # the cloud route reads no source map (refused before anything is touched)
    exp = oracle_run(oracle, rows, lambda q: frames)
    dev = device_run(odo, frames[:, None], "step")  # the object kept its table and its map, and runs
    assert_at_the_bar(dev, exp, "after refusals")
    with pytest.raises(capi.CfearError, match="rc=-1.*sweeps"):
        odo.set_sequence_params([capi.default_params(**kw) for kw in rows])  # after the first sweep
    with pytest.raises(capi.CfearError, match="rc=-1.*sweeps"):
        odo.set_sequence_sources(None)
    # cfear_set_params afterwards: an object-wide field that no longer agrees with the table is refused at the next step, loudly
    ctx.set_params(capi.default_params(**dict(base, assoc_radius=3.0)))
    with pytest.raises(capi.CfearError, match="rc=-1.*assoc_radius"):
        odo.step_host(frames[0][None])
    ctx.set_params(capi.default_params(**base))
    odo.reset()  # keeps both
    dev = device_run(odo, frames[:, None], "step")
    assert_at_the_bar(dev, exp, "after reset")
    odo.release(); ctx.close()
    # a source map on a CA-CFAR object
    hip = dict(base, filter_type=capi.FILTER_CACFAR, z_min=20.0)
    ctx = capi.Context(capi.default_params(**hip), A, R)
    odo = ctx.odometry(3)
    with pytest.raises(capi.CfearError, match="rc=-3"):
        odo.set_sequence_sources(np.zeros(3, dtype=np.int32), 1)
    odo.step_host(np.ascontiguousarray(np.broadcast_to(frames[0], (3, A, R))))
    assert np.all(np.isfinite(odo.poses()))
    odo.release(); ctx.close()
