"""Per-sequence cost and submap_scan_size (cfear_odometry_set_sequence_shapes): loops 6 and 7 of the reference's evaluation grid
(utils/worker:49-52) as sequences of one object. The context's submap_scan_size S sizes the object; a sequence takes any cost and any
s in 1..S, keeps a ring of s keyframes and gives what an object created for that cost and s gives. The registration stage runs one launch
per group (cost, up to 7 keyframes or more), each on the production kernel of its cost.

The bar is tests/test_param_grid_gpu.py's: against the oracle, at EVERY sweep of EVERY row, outer / inner iteration counts, residual,
keyframe and cell counts equal and the pose within 1e-4 m / 1e-5 rad; device against device byte for byte (outputs() of
tests/test_seq_k_gpu.py, cost sampling on).

Drives: pg.drive("blocks"), which moves ~1 m per sweep, under min_keyframe_dist 0.3: every sweep after the first is a keyframe, a ring of
s fills at sweep s - 1 and evicts at every sweep from s on. Each test runs the shortest drive at which its longest ring has evicted at
least twice, and ring_turnover() asserts that from the records (n_keyframes and poses), so a drive that is too short fails."""
import numpy as np
import pytest

from cfear_radarodometry_code_public_amd import capi, replay

import test_param_grid_gpu as pg
import test_seq_k_gpu as sk

pytestmark = pytest.mark.gpu

A, R = pg.A, pg.R
P2P, P2L, P2D = pg.P2P, pg.P2L, pg.P2D
ROUTES = ["step", "replay", "persistent"]
KD = 0.3
BASE = dict(pg.BASE, min_keyframe_dist=KD)


def row(cost, s, **kw):
    return dict(BASE, cost=cost, submap_scan_size=s, **kw)


def shapes_of(rows):
    return [(kw["cost"], kw["submap_scan_size"]) for kw in rows]


def frames_for(longest):
    """the blocks drive cut to longest + 3 sweeps: the ring of `longest` is full after sweep longest - 1 and evicts at sweeps longest,
    longest + 1 and longest + 2"""
    return pg.drive("blocks", 24)[:longest + 3]


def make(ctx_kw, rows, shapes="rows", table=True, shared=True, persistent_max=None, odo_kw=None, cov=False):
    """an object of len(rows) sequences under ctx_kw with the rows' shapes (or the given ones; None: none), then the rows as its table"""
    ctx = capi.Context(capi.default_params(**ctx_kw), A, R)
    if persistent_max is not None:
        ctx.tune(capi.TUNE_REPLAY_PERSISTENT_MAX, persistent_max)
    odo = ctx.odometry(len(rows), **(odo_kw or {}))
    if shapes == "rows":
        shapes = shapes_of(rows)
    if shapes is not None:
        odo.set_sequence_shapes(shapes)
    if table:
        odo.set_sequence_params([capi.default_params(**kw) for kw in rows])
    if shared:
        odo.set_sequence_sources(np.zeros(len(rows), dtype=np.int32), 1)
    if cov:
        odo.set_cov_sampling(True, samples_per_axis=3)
    return ctx, odo


def ring_turnover(run, kw):
    """run: [sweep] (counts, pose) of one row. Follows the keyframe rule (KeyFrameBasedFuse, odometrykeyframefuser.cpp:62-73) on the recorded
    poses, asserts the recorded n_keyframes at every sweep - it reaches exactly the row's s and never exceeds it - and returns the number of
    evictions (keyframes added to a full ring)."""
    s = kw["submap_scan_size"]
    kd, kr = kw["min_keyframe_dist"], capi.default_params(**kw).min_keyframe_rot_deg
    nkf, evictions, key = 0, 0, None
    for t, (g, pose) in enumerate(run):
        if t == 0:
            nkf, key = 1, pose
        else:
            d = np.hypot(pose[0] - key[0], pose[1] - key[1])
            rot = abs((pose[2] - key[2] + np.pi) % (2 * np.pi) - np.pi)
            assert abs(d - kd) > 1e-3 and abs(np.degrees(rot) - kr) > 1e-3  # (no decision of the rule is near its threshold)
            if d > kd or np.degrees(rot) > kr:
                key = pose
                if nkf == s:
                    evictions += 1
                else:
                    nkf += 1
        assert g[3] == nkf and g[3] <= s, (t, g, nkf, s)
    assert nkf == s
    return evictions


def assert_rings_turn_over(runs, rows, longest):
    for q, kw in enumerate(rows):
        ev = ring_turnover(runs[q], kw)
        print("row %d (cost %d, s %d): %d evictions" % (q, kw["cost"], kw["submap_scan_size"], ev))
        assert ev >= 2, (q, ev)
    assert max(kw["submap_scan_size"] for kw in rows) == longest


# ---- 1. rows against the oracle; 2. alone equals in the batch ----------------------------------------------------------------------------
CTX7 = row(P2L, 7)
ROWS7 = [row(P2L, 1), row(P2L, 7), row(P2D, 3), row(P2P, 4), row(P2P, 1), row(P2D, 7), row(P2L, 3, res=3.5, loss=pg.CAUCHY, loss_limit=0.5)]


@pytest.mark.parametrize("route", ROUTES)
def test_rows_of_mixed_shapes_match_the_oracle(oracle, route):
    frames = frames_for(7)
    exp = pg.oracle_rows(oracle, "seq shape 7", ROWS7, frames)
    assert_rings_turn_over(exp, ROWS7, 7)
    ctx, odo = make(CTX7, ROWS7, persistent_max=pg.PERSISTENT[route])
    for q, kw in enumerate(ROWS7):
        got, sh = odo.sequence_params(q), odo.sequence_shape(q)
        assert (got.cost, got.submap_scan_size, got.res) == (kw["cost"], kw["submap_scan_size"], kw["res"])
        assert (sh.cost, sh.submap_scan_size) == (kw["cost"], kw["submap_scan_size"])
    dev = pg.device_run(odo, frames[:, None], route)
    odo.release(); ctx.close()
    pg.assert_at_the_bar(dev, exp, "shapes S = 7 %s" % route)
    assert_rings_turn_over(dev, ROWS7, 7)
    traj = [np.array([p for _, p in d]) for d in dev]
    for a, b in ((0, 1), (1, 5), (0, 4), (2, 5), (3, 4)):  # s alone (P2L 1 / 7, P2D 3 / 7, P2P 4 / 1), the cost alone (s = 7, s = 1): not one code path
        assert np.abs(traj[a][:, :2] - traj[b][:, :2]).max() > 1e-3, (a, b)


_ALONE = {}


def alone(kw, frames, tag, route, odo_kw=None):
    """the row as the only sequence of an object whose context has the row's own cost and submap_scan_size"""
    key = (tuple(sorted(kw.items())), tag, route, tuple(sorted((odo_kw or {}).items())))
    if key not in _ALONE:
        ctx = capi.Context(capi.default_params(**kw), A, R)
        if pg.PERSISTENT[route] is not None:
            ctx.tune(capi.TUNE_REPLAY_PERSISTENT_MAX, pg.PERSISTENT[route])
        odo = ctx.odometry(1, **(odo_kw or {}))
        odo.set_cov_sampling(True, samples_per_axis=3)
        _ALONE[key] = sk.outputs(odo, frames[:, None], route)[0]
        odo.release(); ctx.close()
    return _ALONE[key]


@pytest.mark.parametrize("route", ROUTES)
def test_a_row_alone_equals_the_row_in_the_batch_bit_for_bit(route):
    frames = frames_for(7)
    ctx, odo = make(CTX7, ROWS7, persistent_max=pg.PERSISTENT[route], cov=True)
    batch = sk.outputs(odo, frames[:, None], route)
    odo.release(); ctx.close()
    for q, kw in enumerate(ROWS7):
        assert batch[q] == alone(kw, frames, "blocks 10", route), (route, q, kw["cost"], kw["submap_scan_size"])


# ---- 3. across the small / large seam ---------------------------------------------------------------------------------------------------
CTX10 = row(P2L, 10)
ROWS10 = [row(P2L, 7), row(P2D, 7), row(P2L, 8), row(P2P, 8), row(P2D, 10), row(P2L, 10), row(P2P, 7)]


def test_across_the_small_large_seam(oracle):
    """s = 7 is the last submap the small kernels hold (8 scans with the current one), s = 8 the first that must run elsewhere. Four
    sequences of this batch are not small, one sequence of an alone object is: both are fewer than the compute units, so by
    launch_register_kernel's rule both run register_step_large_kernel, and the s = 7 rows run register_step_kernel on both sides - the same
    kernel shape in the batch and alone, hence bytes. With LARGE_SUBMAP_KERNEL = 1 the not-small rows run the 64-scan production shape
    (register_step64_kernel, 256 threads): against the oracle at the bar, and against alone objects forced the same way byte for byte; the
    256- and the 512-thread shapes differ in the summation order of an evaluation's partial sums (register_step_large.hip), so across
    shapes the comparison is the oracle's bar."""
    frames = frames_for(10)
    exp = pg.oracle_rows(oracle, "seq shape 10", ROWS10, frames)
    assert_rings_turn_over(exp, ROWS10, 10)
    for large_kernel in (0, 1):
        ctx, odo = make(CTX10, ROWS10, odo_kw=dict(large_kernel=large_kernel))
        dev = pg.device_run(odo, frames[:, None], "step")
        odo.release(); ctx.close()
        pg.assert_at_the_bar(dev, exp, "seam, LARGE_SUBMAP_KERNEL %d" % large_kernel)
        assert_rings_turn_over(dev, ROWS10, 10)
        ctx, odo = make(CTX10, ROWS10, odo_kw=dict(large_kernel=large_kernel), cov=True)
        batch = sk.outputs(odo, frames[:, None], "step")
        odo.release(); ctx.close()
        for q, kw in enumerate(ROWS10):
            assert batch[q] == alone(kw, frames, "blocks 13", "step", dict(large_kernel=large_kernel)), (large_kernel, q, kw["cost"], kw["submap_scan_size"])


# ---- 4. grouped longest-first order -----------------------------------------------------------------------------------------------------
def test_grouped_registration_order_changes_no_output():
    """13 sequences in groups of 1 (P2D, small), 5 (P2L, not small) and 7 (P2L, small), no P2P: with cfear_tune REGISTRATION_ORDER the workgroups of
    every launch take their group's sequences longest first from the second sweep on (order_groups_kernel); which workgroup a sequence takes
    changes nothing it computes."""
    rows = [row(P2D, 7)] + [row(P2L, 8, res=2.5 + 0.25 * i) for i in range(5)] + [row(P2L, 2, z_min=50.0 + 5 * i) for i in range(7)]
    rows = [rows[i] for i in (3, 7, 0, 8, 1, 9, 10, 2, 11, 4, 12, 5, 6)]
    frames = pg.drive("blocks", 24)[:6]
    outs = []
    for reg_order in (1, 0):
        ctx, odo = make(row(P2L, 8), rows, odo_kw=dict(reg_order=reg_order), cov=True)
        outs.append(sk.outputs(odo, frames[:, None], "step"))
        odo.release(); ctx.close()
    for q in range(13):
        assert outs[0][q] == outs[1][q], q
    assert len({o[-1][0] for o in outs[0]}) >= 8  # (the rows are no copies of each other: their last poses differ)


# ---- 5. identity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_shapes_equal_to_the_contexts_change_nothing(route):
    B = 3
    kw = row(P2L, 4)
    frames = np.ascontiguousarray(np.stack([pg.drive("blocks", 24)[:7], pg.drive("canyon", 24, 10, 20)[:7], pg.drive("canyon", 24, 11, 21)[:7]], axis=1))
    outs = []
    for shapes in (None, [(P2L, 4)] * B):
        ctx, odo = make(kw, [kw] * B, shapes=shapes, table=False, shared=False, persistent_max=pg.PERSISTENT[route], cov=True)
        outs.append(sk.outputs(odo, frames, route))
        odo.release(); ctx.close()
    assert outs[0] == outs[1]


# ---- 6. shared sources with cost sampling; a CA-CFAR object --------------------------------------------------------------------------------
def test_mixed_shapes_on_one_source_with_cost_sampling_against_the_oracle(oracle):
    RTOL, ATOL = 1e-5, 1e-12  # tests/test_odometry_cov_sampling_gpu.py
    rows = [row(P2L, 3), row(P2D, 5), row(P2P, 2), row(P2L, 1, loss=pg.CAUCHY, loss_limit=0.5), row(P2D, 2, res=3.5), row(P2P, 5)]
    frames = frames_for(5)
    fus = [oracle.Fuser(oracle.default_params(**kw)) for kw in rows]
    for fu in fus:
        fu.set_cov_sampling(True, steps=3)
    ctx, odo = make(row(P2L, 5), rows, cov=True)
    n_sampled = [0] * len(rows)
    runs = [[] for _ in rows]
    for t in range(len(frames)):
        odo.step_host(frames[t][None])
        got, cov = odo.poses(), odo.covariances().reshape(len(rows), 6, 6)
        for q in range(len(rows)):
            e = fus[q].process_polar(frames[t])
            S, nc, nk = odo.summary(q)
            runs[q].append(((0, [], 0, nk, nc), np.array(got[q])))
            assert nk == fus[q].num_keyframes, (t, q)
            assert np.all(np.abs(got[q][:2] - e[:2]) < 1e-4) and abs(got[q][2] - e[2]) < 1e-5, (t, q)
            ref = fus[q].last_cov()
            print("cov row %d sweep %d: max rel diff %.2e" % (q, t, np.max(np.abs(cov[q] - ref) / np.maximum(np.abs(ref), 1e-300))))
            assert np.allclose(cov[q], ref, rtol=RTOL, atol=ATOL), (t, q, cov[q], ref)
            n_sampled[q] += int(odo.cov_samples(q)[1])
    odo.release(); ctx.close()
    assert_rings_turn_over(runs, rows, 5)
    assert all(v >= 1 for v in n_sampled), n_sampled  # every row's covariance came from ITS sampling, under its own cost


def test_mixed_shapes_ca_cfar_object(oracle):
    cf = dict(window_size=10, nb_guard_cells=20, false_alarm_rate=0.01)
    hip = dict(filter_type=capi.FILTER_CACFAR, cfar_window_size=10, cfar_nb_guard_cells=20, cfar_false_alarm_rate=0.01)
    rows = [row(P2L, 4, z_min=20.0), row(P2D, 2, z_min=20.0), row(P2P, 4, z_min=20.0), row(P2L, 1, z_min=20.0, res=3.5)]
    frames = frames_for(4)
    exp = pg.oracle_run(oracle, rows, lambda q: frames, cfar=cf)
    assert_rings_turn_over(exp, rows, 4)
    ctx, odo = make(dict(row(P2L, 4, z_min=20.0), **hip), [dict(r, **hip) for r in rows], shared=False)
    out = [[] for _ in rows]
    for t in range(len(frames)):
        odo.step_host(np.ascontiguousarray(np.broadcast_to(frames[t], (len(rows), A, R))))
        got = odo.poses()
        for q in range(len(rows)):
            S, nc, nk = odo.summary(q)
            g = (int(S.outer_iterations), [int(v) for v in S.inner_iterations[:min(max(int(S.outer_iterations), 0), 8)]], int(S.num_residuals), nk, nc)
            out[q].append((g, np.array(got[q])))
    odo.release(); ctx.close()
    pg.assert_at_the_bar(out, exp, "CA-CFAR with shapes")


# ---- 7. replay_grid ---------------------------------------------------------------------------------------------------------------------
def test_replay_grid_with_a_cost_and_submap_scan_size_grid():
    from cfear_radarodometry_code_public_amd import kitti
    frames = frames_for(8)
    T = len(frames)
    base = capi.default_params(**row(P2L, 4))
    rows = replay.param_grid(base, submap_scan_size=[1, 3, 8], cost=[P2P, P2L, P2D])
    assert [(r.cost, r.submap_scan_size) for r in rows] == [(c, s) for c in (P2P, P2L, P2D) for s in (1, 3, 8)]
    gt = kitti.poses_from_xyt(np.cumsum(np.tile([[1.0, 0.0, 0.0]], (T, 1)), axis=0))
    out = replay.replay_grid(frames, rows, gt=gt, piece=4, drift_on="device")
    assert out["poses"].shape == (T, 9, 3) and out["records"].shape == (T, 9)
    assert out["drift"] is not None and len(out["drift"]) == 9 and all("translation_percent" in d for d in out["drift"])  # every row scored
    for q, r in enumerate(rows):
        assert int(out["records"]["n_keyframes"][:, q].max()) == r.submap_scan_size
        assert list(out["records"]["n_keyframes"][:, q]) == [min(t + 1, r.submap_scan_size) for t in range(T)]  # (every sweep a keyframe: the ring of 8 evicts at sweeps 8, 9, 10)
        ctx = capi.Context(r, A, R)  # the row alone: its own cost and submap_scan_size are the context's
        odo = ctx.odometry(1)
        rec = np.concatenate([odo.replay_host(frames[t0:t0 + 4, None]) for t0 in range(0, T, 4)], axis=0)
        odo.release(); ctx.close()
        assert np.array_equal(out["poses"][:, q], rec["pose"][:, 0]), q
    assert np.abs(out["poses"][:, 0, :2] - out["poses"][:, 2, :2]).max() > 1e-3  # P2P, s = 1 against 8


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_object_unchanged_and_usable(oracle):
    import surface_ref
    T = 5
    frames = pg.drive("blocks", 24)[:T]
    # (compensation off and every sweep a keyframe: the scans of a registration are the filtered clouds of the last sweeps, as in
    # tests/test_param_grid_gpu.py's surface test)
    nk = dict(use_keyframe=0, compensate=0)
    rows = [row(P2L, 4, **nk), row(P2L, 2, **nk), row(P2L, 1, res=3.5, **nk), row(P2L, 3, **nk)]
    ctx_kw = row(P2L, 4, **nk)
    good = shapes_of(rows)
    exp = pg.oracle_run(oracle, rows, lambda q: frames)
    ctx, odo = make(ctx_kw, rows)
    odo.set_surface_recording(True)

    def unchanged_and_usable(what):
        for q, kw in enumerate(rows):
            sh, par = odo.sequence_shape(q), odo.sequence_params(q)
            assert (sh.cost, sh.submap_scan_size) == good[q] == (par.cost, par.submap_scan_size) and par.res == kw["res"], (what, q)
        odo.reset()  # keeps shapes, table and map
        dev = pg.device_run(odo, frames[:, None], "step")
        pg.assert_at_the_bar(dev, exp, what)
        odo.reset()

    for field, v in (("submap_scan_size", 0), ("submap_scan_size", 5), ("submap_scan_size", -3), ("cost", 3), ("cost", -1)):
        bad = [list(s) for s in good]
        bad[2][0 if field == "cost" else 1] = v
        with pytest.raises(capi.CfearError, match=r"rc=-1.*row 2.*%s" % field):
            odo.set_sequence_shapes(bad)
        unchanged_and_usable("after %s = %d" % (field, v))
    with pytest.raises(capi.CfearError, match="rc=-1"):
        odo.set_sequence_shapes(good[:3])  # n_rows must be the object's n_sequences
    # the table's rows are compared with the shapes: a row that disagrees with ITS shape is refused, row and field named
    for field, v in (("submap_scan_size", 4), ("cost", P2D)):
        bad = [capi.default_params(**kw) for kw in rows]
        setattr(bad[1], field, v)
        with pytest.raises(capi.CfearError, match=r"rc=-1.*row 1.*%s" % field):
            odo.set_sequence_params(bad)
    # ... and shapes the existing table's rows would then disagree with: the other shapes, or none (the context's values again)
    other = list(good)
    other[3] = (P2L, 2)
    with pytest.raises(capi.CfearError, match=r"rc=-1.*row 3.*submap_scan_size"):
        odo.set_sequence_shapes(other)
    with pytest.raises(capi.CfearError, match=r"rc=-1.*row 1.*submap_scan_size"):
        odo.set_sequence_shapes(None)
    unchanged_and_usable("after table / shape disagreements")
    # surfaces under shapes that differ only in s: work, and match the oracle (tests/test_surface_gpu.py's bound for the restatement)
    for t in range(T):
        odo.step_host(frames[t][None])
    s, n_used, itr_used, poses_used = odo.surface(0.25, 1, details=True)
    s = s.cpu().numpy()
    for q, kw in enumerate(rows):
        p = oracle.default_params(**kw)
        n = int(n_used[q])
        assert n == min(T, kw["submap_scan_size"] + 1)  # the sequence's own ring and the current scan
        osc = [oracle.Scan(oracle.cloud(oracle.filter_polar(frames[T - n + i], int(kw["z_min"]), 12), p.range_res, p.min_distance), p) for i in range(n)]
        ref = surface_ref.surface(oracle, osc, poses_used[q, :n], p, int(itr_used[q]), 0.25, 1)
        m = ~np.isnan(ref)
        assert np.array_equal(np.isnan(s[q]), np.isnan(ref))
        print("surface row %d: max rel diff %.2e" % (q, np.max(np.abs(s[q][m] - ref[m]) / np.maximum(np.abs(ref[m]), 1e-300))))
        assert np.all(np.abs(s[q][m] - ref[m]) <= 1e-9 * np.maximum(np.abs(ref[m]), 1e-300)), q
    with pytest.raises(capi.CfearError, match="rc=-1.*sweeps"):
        odo.set_sequence_shapes(good)  # after the first sweep
    with pytest.raises(capi.CfearError, match="rc=-1.*sweeps"):
        odo.set_sequence_shapes(None)
    unchanged_and_usable("after a late call")
    # NULL, once the table is gone: the context's values again, and set_sequence_params refuses what it refused before shapes existed
    odo.set_sequence_params(None)
    odo.set_sequence_shapes(None)
    assert [(odo.sequence_shape(q).cost, odo.sequence_shape(q).submap_scan_size) for q in range(4)] == [(P2L, 4)] * 4
    with pytest.raises(capi.CfearError, match=r"rc=-1.*row 1.*submap_scan_size"):
        odo.set_sequence_params([capi.default_params(**kw) for kw in rows])
    odo.release(); ctx.close()
    # surfaces under shapes that differ in cost: refused, saying so; the object goes on stepping
    mixed = [row(P2L, 4), row(P2D, 4), row(P2L, 2), row(P2P, 1)]
    ctx, odo = make(ctx_kw, mixed)
    odo.set_surface_recording(True)
    odo.step_host(frames[0][None]); odo.step_host(frames[1][None])
    with pytest.raises(capi.CfearError, match="rc=-3.*cost"):
        odo.surface(0.25, 1)
    odo.reset()
    dev = pg.device_run(odo, frames[:, None], "step")
    pg.assert_at_the_bar(dev, pg.oracle_run(oracle, mixed, lambda q: frames), "after the refused surface")
    odo.release(); ctx.close()
    # an object created with overlap streams takes no shapes (its sub-batches are index ranges), and runs as before
    ctx = capi.Context(capi.default_params(**ctx_kw), A, R)
    odo = ctx.odometry(4, overlap=2)
    with pytest.raises(capi.CfearError, match="rc=-3.*overlap"):
        odo.set_sequence_shapes(good)
    assert [(odo.sequence_shape(q).cost, odo.sequence_shape(q).submap_scan_size) for q in range(4)] == [(P2L, 4)] * 4
    same = [dict(ctx_kw)] * 4
    dev = pg.device_run(odo, np.ascontiguousarray(np.broadcast_to(frames[:, None], (T, 4, A, R))), "step")
    pg.assert_at_the_bar(dev, pg.oracle_run(oracle, same[:1], lambda q: frames) * 4, "overlap object after the refusal")
    odo.release(); ctx.close()
