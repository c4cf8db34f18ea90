"""Per-sequence k_strongest (cfear_odometry_set_sequence_params): the context's k_strongest K is what the filter runs with and what the
object is sized for; a row may carry any k in 1..K and its sequence then gives what an object created under a context with that k gives,
bit for bit - the k strongest of a bearing are the last k of the returns the K-filter kept of it (tests/test_seq_k_cpu.py pins that on the
oracle), and the cloud pass reads that window.

The bar is tests/test_param_grid_gpu.py's: against the oracle, at EVERY sweep of EVERY row, outer / inner iteration counts, residual,
keyframe and cell counts equal and the pose within 1e-4 m / 1e-5 rad; device against device byte for byte. A = 400: k = 12 is the last
k whose cloud stays in registers and takes the compact feature path (A * k <= 5120), k = 13 the first past it."""
import numpy as np
import pytest

from cfear_radarodometry_code_public_amd import capi, replay

import seq_k_inputs
import test_param_grid_gpu as pg

pytestmark = pytest.mark.gpu

A, R = pg.A, pg.R
T = 24
ROUTES = ["step", "replay", "persistent"]
CTX_A = dict(pg.BASE, cost=pg.P2L, submap_scan_size=4, k_strongest=40, z_min=50.0)
# k alone (z_min 60, above the context's 50), then k together with z_min: further above the context's, and the context's own
ROWS_A = [dict(CTX_A, k_strongest=k, z_min=60.0) for k in (1, 5, 12, 13, 40)] + [dict(CTX_A, k_strongest=12, z_min=70.0), dict(CTX_A, k_strongest=5, z_min=50.0)]
CTX_B = dict(pg.BASE, cost=pg.P2L, submap_scan_size=4, k_strongest=12)
ROWS_B = [dict(CTX_B, k_strongest=k) for k in (12, 10, 1)]


def frames_main():
    return pg.drive("blocks", 60)[:T]


def run_rows(ctx_kw, rows, frames, route):
    ctx, odo = pg.make_object(ctx_kw, rows, np.zeros(len(rows), dtype=np.int32), 1, persistent_max=pg.PERSISTENT[route])
    for q, kw in enumerate(rows):
        assert odo.sequence_params(q).k_strongest == kw["k_strongest"]  # the row's own k
    dev = pg.device_run(odo, frames[:, None], route)
    odo.release(); ctx.close()
    return dev


# ---- 1. against the oracle, row by row (and 4.: not one code path) ---------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_rows_of_a_k40_object_match_the_oracle(oracle, route):
    frames = frames_main()
    exp = pg.oracle_rows(oracle, "seq k A", ROWS_A, frames)
    dev = run_rows(CTX_A, ROWS_A, frames, route)
    pg.assert_at_the_bar(dev, exp, "K = 40 %s" % route)
    traj = [np.array([p for _, p in d]) for d in dev]
    for a, b in ((1, 2), (2, 4), (1, 4)):  # k = 5, 12, 40 at one z_min: three different trajectories
        assert np.abs(traj[a][:, :2] - traj[b][:, :2]).max() > 1e-3, (a, b)


@pytest.mark.parametrize("route", ROUTES)
def test_rows_of_a_k12_object_match_the_oracle(oracle, route):
    frames = frames_main()
    exp = pg.oracle_rows(oracle, "seq k B", ROWS_B, frames)
    dev = run_rows(CTX_B, ROWS_B, frames, route)
    pg.assert_at_the_bar(dev, exp, "K = 12 %s" % route)


# ---- 2. alone equals in the batch, bit for bit -------------------------------------------------------------------------------------------
def outputs(odo, frames, route):
    """every output of every sequence over the sweeps, as bytes per sequence: [B] lists"""
    B = odo.B
    out = [[] for _ in range(B)]
    if route == "step":
        for t in range(frames.shape[0]):
            odo.step_host(frames[t])
            poses, cov = odo.poses(), odo.covariances()
            for q in range(B):
                costs, sampled = odo.cov_samples(q)
                assert costs.shape == (27,)
                out[q].append((poses[q].tobytes(), cov[q].tobytes(), bytes(odo.summary(q)[0]), odo.summary(q)[1:], costs.tobytes(), int(sampled)))
    else:
        rec, cov = odo.replay_host(frames, covariances=True)
        poses = odo.poses()
        for q in range(B):
            costs, sampled = odo.cov_samples(q)
            out[q] = [np.ascontiguousarray(rec[:, q]).tobytes(), np.ascontiguousarray(cov[:, q]).tobytes(), poses[q].tobytes(), bytes(odo.summary(q)[0]),
                      costs.tobytes(), int(sampled)]
    return out


_ALONE = {}


def alone(kw, frames, tag, route):
    """the row as the only sequence of an object whose context - and filter - runs with the row's own k_strongest"""
    key = (tuple(sorted(kw.items())), tag, route)
    if key not in _ALONE:
        ctx = capi.Context(capi.default_params(**kw), A, R)
        if pg.PERSISTENT[route] is not None:
            ctx.tune(capi.TUNE_REPLAY_PERSISTENT_MAX, pg.PERSISTENT[route])
        odo = ctx.odometry(1)
        odo.set_cov_sampling(True, samples_per_axis=3)
        _ALONE[key] = outputs(odo, frames[:, None], route)[0]
        odo.release(); ctx.close()
    return _ALONE[key]


@pytest.mark.parametrize("route", ROUTES)
def test_a_row_alone_equals_the_row_in_the_batch_bit_for_bit(route):
    frames = frames_main()
    ctx, odo = pg.make_object(CTX_A, ROWS_A, np.zeros(len(ROWS_A), dtype=np.int32), 1, persistent_max=pg.PERSISTENT[route])
    odo.set_cov_sampling(True, samples_per_axis=3)
    batch = outputs(odo, frames[:, None], route)
    odo.release(); ctx.close()
    for q, kw in enumerate(ROWS_A):
        assert batch[q] == alone(kw, frames, "blocks", route), (route, q, kw["k_strongest"], kw["z_min"])


@pytest.mark.parametrize("route", ["step", "persistent"])
def test_a_row_at_two_positions_of_a_larger_batch_with_its_own_sweeps(route):
    """no source map: every sequence reads its own sweep; each row twice, at positions q and 13 - q, on one of three drives (12 sweeps: the
    fourteen copies of a sweep are resident at once)"""
    n = 12
    drives = [pg.drive("blocks", 60)[:n], pg.drive("canyon", 24, 10, 20)[:n], pg.drive("canyon", 24, 11, 21)[:n]]
    rows = ROWS_A + ROWS_A[::-1]
    which = [q % 3 for q in range(len(rows))]
    frames = np.ascontiguousarray(np.stack([drives[d] for d in which], axis=1))
    ctx, odo = pg.make_object(CTX_A, rows, persistent_max=pg.PERSISTENT[route])
    odo.set_cov_sampling(True, samples_per_axis=3)
    batch = outputs(odo, frames, route)
    odo.release(); ctx.close()
    for q, kw in enumerate(rows):
        assert batch[q] == alone(kw, drives[which[q]], "drive %d x %d" % (which[q], n), route), (route, q, kw["k_strongest"], kw["z_min"])


# ---- 3. bearings with fewer than K returns ---------------------------------------------------------------------------------------------
def test_bearings_with_fewer_returns_than_K(oracle):
    """azimuth rows that hold exactly 0, 1, k - 1, k, k + 1 and K - 1 bytes at or above z_min, several of equal intensity (the range decides):
    where the zeros behind a bearing's returns and the window of its last k returns meet"""
    z = 60
    frames = seq_k_inputs.handmade_frames(frames_main(), z)
    ctx_kw = dict(CTX_A, z_min=float(z))
    rows = [dict(ctx_kw, k_strongest=k) for k in seq_k_inputs.KS]
    exp = pg.oracle_run(oracle, rows, lambda q: frames)
    for route in ROUTES:
        dev = run_rows(ctx_kw, rows, frames, route)
        pg.assert_at_the_bar(dev, exp, "fewer than K returns, %s" % route)


# ---- 5. identity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("K", [12, 40])
def test_rows_of_the_contexts_k_change_nothing(route, K):
    B = 3
    frames = np.ascontiguousarray(np.stack([pg.drive("canyon", T, 10 + q, 20 + q) for q in range(B)], axis=1))
    kw = dict(pg.BASE, k_strongest=K)
    outs = []
    for with_table in (False, True):
        ctx = capi.Context(capi.default_params(**kw), A, R)
        if pg.PERSISTENT[route] is not None:
            ctx.tune(capi.TUNE_REPLAY_PERSISTENT_MAX, pg.PERSISTENT[route])
        odo = ctx.odometry(B)
        odo.set_cov_sampling(True, samples_per_axis=3)
        if with_table:
            odo.set_sequence_params([capi.default_params(**kw)] * B)
        outs.append(outputs(odo, frames, route))
        odo.release(); ctx.close()
    assert outs[0] == outs[1]


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_object_unchanged_and_usable(oracle):
    n = 6
    frames = frames_main()[:n]
    rows = ROWS_A[:4]
    exp = [e[:n] for e in pg.oracle_rows(oracle, "seq k A", ROWS_A, frames_main())[:4]]
    ctx, odo = pg.make_object(CTX_A, rows, np.zeros(4, dtype=np.int32), 1)
    for k in (41, 0, -3, 65):
        bad = [capi.default_params(**kw) for kw in rows]
        bad[2].k_strongest = k
        with pytest.raises(capi.CfearError, match=r"rc=-1.*row 2.*k_strongest"):
            odo.set_sequence_params(bad)
        assert [odo.sequence_params(q).k_strongest for q in range(4)] == [1, 5, 12, 13]
    bad = [capi.default_params(**kw) for kw in rows]
    bad[1].cost = pg.P2P  # the other refusals name the per-sequence fields, k_strongest among them
    with pytest.raises(capi.CfearError, match=r"rc=-1.*row 1.*cost.*k_strongest \(<= the context's\)"):
        odo.set_sequence_params(bad)
    odo.set_sequence_sources(None)  # (under a map the cloud route is refused for the map)
    with pytest.raises(capi.CfearError, match="rc=-3.*k_strongest"):
        odo.step_cloud_device(1, 16, 1)  # a cloud has no slots to take a window of (refused before anything is touched)
    odo.set_sequence_sources(np.zeros(4, dtype=np.int32), 1)
    dev = pg.device_run(odo, frames[:, None], "step")
    pg.assert_at_the_bar(dev, exp, "after refusals")
    # cfear_set_params to a K below a row's k: refused at the next step, loudly; back at K the object runs on
    ctx.set_params(capi.default_params(**dict(CTX_A, k_strongest=12)))
    with pytest.raises(capi.CfearError, match="rc=-1.*k_strongest"):
        odo.step_host(frames[0][None])
    ctx.set_params(capi.default_params(**CTX_A))
    odo.reset()
    dev = pg.device_run(odo, frames[:, None], "step")
    pg.assert_at_the_bar(dev, exp, "after reset")
    odo.release(); ctx.close()
    # a CA-CFAR object: the detector has no k
    hip = dict(CTX_A, filter_type=capi.FILTER_CACFAR, z_min=20.0)
    ctx = capi.Context(capi.default_params(**hip), A, R)
    odo = ctx.odometry(3)
    with pytest.raises(capi.CfearError, match=r"rc=-1.*row 1.*k_strongest"):
        odo.set_sequence_params([capi.default_params(**dict(hip, k_strongest=k)) for k in (40, 12, 40)])
    odo.set_sequence_params([capi.default_params(**dict(hip, res=r)) for r in (3.0, 3.5, 2.5)])
    assert odo.sequence_params(1).res == 3.5
    # ... and cfear_set_params under its table: the rows' k is no longer the context's (the object's shape does not depend on k here, so
    # this is the table's own check)
    ctx.set_params(capi.default_params(**dict(hip, k_strongest=12)))
    with pytest.raises(capi.CfearError, match=r"rc=-1.*row 0.*k_strongest"):
        odo.step_host(np.ascontiguousarray(np.broadcast_to(frames[0], (3, A, R))))
    ctx.set_params(capi.default_params(**hip))
    odo.step_host(np.ascontiguousarray(np.broadcast_to(frames[0], (3, A, R))))
    assert np.all(np.isfinite(odo.poses()))
    odo.release(); ctx.close()


# ---- 7. replay.replay_grid with a k axis ------------------------------------------------------------------------------------------------
def test_replay_grid_with_a_k_axis(oracle):
    frames = frames_main()
    base = dict(CTX_A, z_min=60.0)
    rows = replay.param_grid(capi.default_params(**base), k_strongest=[5, 12, 40])
    assert [r.k_strongest for r in rows] == [5, 12, 40]
    out = replay.replay_grid(frames, rows)  # no context_params: the context runs with the largest k of the rows
    exp = pg.oracle_rows(oracle, "seq k A", ROWS_A, frames)
    rec = out["records"]
    dev = []
    for q in range(3):
        dev.append([])
        for t in range(T):
            r = rec[t, q]
            g = (int(r["outer_iterations"]), [int(v) for v in r["inner_iterations"][:min(max(int(r["outer_iterations"]), 0), 8)]], int(r["num_residuals"]),
                 int(r["n_keyframes"]), int(r["n_cells"]))
            dev[q].append((g, np.array(out["poses"][t, q])))
    pg.assert_at_the_bar(dev, [exp[1], exp[2], exp[4]], "replay_grid k axis")
