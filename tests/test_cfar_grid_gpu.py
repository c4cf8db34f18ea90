"""CA-CFAR detector grids in one pass (cfear_filter_cfar_grid_device, cfear_odometry_set_sequence_detectors): several detectors over shared
source images - a source row staged and its prefix sums built once, every distinct (source, detector) decided once - and the detector grid
of the reference's 4_filter_eval (params/kstrong_vs_cfar/oxford-cfear-3-ca-cfar) as the sequences of one CA-CFAR odometry object.

Filter level: every cloud bit for bit the oracle's AND the one-detector batch entry's on the same device. Odometry level: every sequence bit
for bit the only sequence of an object under a context with its detector, and at the project's bar (1e-4 m, 1e-5 rad, equal counts) against
the oracle's fuser fed the oracle's clouds."""
import numpy as np
import pytest

from cfear_radarodometry_code_public_amd import capi, synth

pytestmark = pytest.mark.gpu
RR = np.float32(0.0595238)
P2P, P2L = 0, 1

# (window_size, nb_guard_cells, false_alarm_rate, z_min). At 64 bins (60, 30) and (500, 10) reach past the row from every bin: both windows
# are clipped everywhere. (500, 10): the far corner of the reference's grid
SETS = [(1, 1, 0.5, 0.0), (3, 0, 0.2, 0.0), (10, 20, 0.01, 60.0), (40, 10, 0.01, 20.0), (60, 30, 0.001, 10.0), (500, 10, 0.0001, 20.0)]


def images(kind, n, A, R, seed):
    rng = np.random.default_rng(seed)
    out = np.empty((n, A, R), dtype=np.uint8)
    for s in range(n):
        if kind == "random":
            img = rng.integers(0, 256, size=(A, R), dtype=np.uint8)
            img[:, ::11] = np.minimum(img[:, ::11].astype(int) + 100, 255).astype(np.uint8)
        elif kind == "clutter":  # tests/test_cfar_gpu.py::test_rows_of_clutter
            img = rng.integers(0, 12, size=(A, R), dtype=np.uint8)
            img[::2, ::8] = 255
            img[1::4, 100:103] = 200
            img[3, :] = 90
            img[3, ::5] = 140
        else:
            img = np.full((A, R), 255 if kind == "saturated" else 0, dtype=np.uint8)
        out[s] = img
    return out


@pytest.mark.parametrize("kind", ["random", "clutter", "saturated", "zero"])
@pytest.mark.parametrize("A,R,n_src,mind", [(8, 64, 3, 0.0), (16, 3360, 2, 2.5), (5, 6000, 3, 2.5), (37, 1001, 2, 2.5)])
def test_grid_clouds_equal_the_oracle_and_the_one_detector_entry(oracle, A, R, n_src, mind, kind):
    """(37, 1001): rows of no whole dwords - the one-detector kernels once per distinct set, same indirection; the others the shared kernel
    (16 bins per thread at 64 and 3360 bins, 32 at 6000)"""
    import torch
    imgs = images(kind, n_src, A, R, A * 1000 + R)
    rng = np.random.default_rng(R + len(kind))
    # every (source, set) at least once, three exact duplicates, in scrambled order
    pairs = [(s, k) for s in range(n_src) for k in range(len(SETS))]
    pairs += [pairs[1], pairs[len(SETS)], pairs[-1]]
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    dets = [SETS[k] for _, k in pairs]
    source = np.array([s for s, _ in pairs], dtype=np.int32)
    n = len(pairs)
    exp = {}
    for s, k in set(pairs):
        w, g, pfa, z = SETS[k]
        exp[(s, k)] = oracle.cfar(imgs[s], RR, z, mind, w, g, pfa, prefix=True)
    cap = max(len(e) for e in exp.values()) + 5
    d = torch.from_numpy(imgs).cuda()
    # the same detections the only way there was: cfear_filter_cfar_batch_device per set, under a context with the set's z_min
    base = {}
    for k, (w, g, pfa, z) in enumerate(SETS):
        c = capi.Context(capi.default_params(range_res=RR, z_min=z, min_distance=mind), A, R)
        cnt = torch.zeros(n_src, dtype=torch.int32, device="cuda")
        flat = torch.zeros((n_src, cap, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        c.filter_cfar_batch(d, n_src, flat, cap, cnt, w, g, pfa)
        c.synchronize()
        for s in range(n_src):
            base[(s, k)] = flat[s, :int(cnt[s])].cpu().numpy()
        c.close()
    ctx = capi.Context(capi.default_params(range_res=RR, z_min=33.0, min_distance=mind), A, R)  # (the context's z_min is not a set's)
    for capacity in (cap, max(cap // 3, 1)):
        cnt = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        flat = torch.full((n * capacity * 3 + 3,), -7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ctx.filter_cfar_grid(d, n_src, dets, source, flat, capacity, cnt)
        ctx.synchronize()
        got_n, got = cnt.cpu().numpy(), flat.cpu().numpy()
        assert np.all(got[n * capacity * 3:] == -7.0)  # nothing past the last slot
        for c, (s, k) in enumerate(pairs):
            e = exp[(s, k)]
            assert got_n[c] == len(e), (c, s, k, got_n[c], len(e))  # the true count, whatever the capacity
            m = min(len(e), capacity)
            slot = got[c * capacity * 3:(c + 1) * capacity * 3].reshape(capacity, 3)
            assert np.array_equal(slot[:m], e[:m]), (c, s, k)  # points and order
            assert np.all(slot[m:] == -7.0)
            assert np.array_equal(base[(s, k)], e), (s, k)
            assert np.array_equal(slot[:m], base[(s, k)][:m])
    assert sum(len(e) for e in exp.values()) > 0 or kind == "zero"
    # source NULL: cloud c reads image c
    cnt = torch.full((n_src,), -1, dtype=torch.int32, device="cuda")
    flat = torch.full((n_src, cap, 3), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.filter_cfar_grid(d, n_src, [SETS[3]] * n_src, None, flat, cap, cnt)
    ctx.synchronize()
    for s in range(n_src):
        assert int(cnt[s]) == len(exp[(s, 3)]) and np.array_equal(flat[s, :int(cnt[s])].cpu().numpy(), exp[(s, 3)])
    ctx.close()


def test_grid_entry_refuses_bad_rows_by_name():
    import torch
    A, R = 8, 64
    ctx = capi.Context(capi.default_params(range_res=RR, z_min=20.0), A, R)
    d = torch.zeros((2, A, R), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(3, dtype=torch.int32, device="cuda")
    flat = torch.zeros((3, 16, 3), dtype=torch.float32, device="cuda")
    good = (40, 10, 0.01, 20.0)
    for bad, field in (((0, 10, 0.01, 20.0), "window_size"), ((40, -1, 0.01, 20.0), "nb_guard_cells"), ((40, 10, 0.0, 20.0), "false_alarm_rate"),
                       ((40, 10, float("inf"), 20.0), "false_alarm_rate"), ((40, 10, 0.01, float("nan")), "z_min")):
        with pytest.raises(capi.CfearError, match=r"rc=-1.*row 1.*%s" % field):
            ctx.filter_cfar_grid(d, 2, [good, bad, good], [0, 1, 1], flat, 16, cnt)
    with pytest.raises(capi.CfearError, match=r"rc=-1.*row 2.*source"):
        ctx.filter_cfar_grid(d, 2, [good, good, good], [0, 1, 2], flat, 16, cnt)
    ctx.filter_cfar_grid(d, 2, [good, good, good], [0, 1, 1], flat, 16, cnt)  # still usable
    ctx.synchronize()
    assert cnt.cpu().tolist() == [0, 0, 0]
    ctx.close()


# ---- odometry level ------------------------------------------------------------------------------------------------------------------
OA, OR, T = 400, 3360, 12
BASE = dict(range_res=RR, k_strongest=12, z_min=20.0, res=3.0, weight_intensity=1, weight_opt=0, compensate=1, radar_ccw=0, cost=P2L, loss=1,
            loss_limit=0.1, covar_scale=1.0, regularization=1.0, submap_scan_size=4, filter_type=capi.FILTER_CACFAR, cfar_nb_guard_cells=10)
# window {40, 150} x rate {0.01, 0.001}, then two rows that repeat a detector under another res / another cost
DETS = [(40, 10, 0.01, 20.0), (40, 10, 0.001, 20.0), (150, 10, 0.01, 20.0), (150, 10, 0.001, 20.0), (40, 10, 0.01, 20.0), (150, 10, 0.001, 20.0)]
EXTRA = [dict(), dict(), dict(), dict(), dict(res=5.0), dict(cost=P2P)]
PERSISTENT = {"step": None, "replay": 0, "persistent": 256}
_FRAMES, _ORACLE = {}, {}


def row_kw(q):
    w, g, pfa, z = DETS[q]
    return dict(BASE, cfar_window_size=w, cfar_nb_guard_cells=g, cfar_false_alarm_rate=pfa, z_min=z, **EXTRA[q])


def frames():
    if "f" not in _FRAMES:
        fr = np.empty((T, OA, OR), dtype=np.uint8)
        for t0, chunk in synth.drive_chunks(T, "canyon", 10, 20, OA, OR, RR, ccw=False):
            fr[t0:t0 + len(chunk)] = chunk
        _FRAMES["f"] = fr
    return _FRAMES["f"]


def run_route(odo, fr, route):
    """fr [T, n_sources, A, R] -> (poses after the last sweep, per-sweep records or per-sweep (poses, summaries)) as bytes-comparable arrays"""
    B = odo.B
    if route == "step":
        poses, sums = [], []
        for t in range(fr.shape[0]):
            odo.step_host(fr[t])
            poses.append(odo.poses())
            sums.append([(bytes(S), nc, nk) for S, nc, nk in (odo.summary(q) for q in range(B))])
        return np.array(poses), sums
    rec = odo.replay_host(fr)
    return np.array(rec["pose"]), [[rec[t, q].tobytes() for q in range(B)] for t in range(fr.shape[0])]


def make_ctx(kw, route):
    ctx = capi.Context(capi.default_params(**kw), OA, OR)
    if PERSISTENT[route] is not None:
        ctx.tune(capi.TUNE_REPLAY_PERSISTENT_MAX, PERSISTENT[route])
    return ctx


def grid_object(route):
    ctx = make_ctx(BASE, route)
    odo = ctx.odometry(len(DETS))
    odo.set_sequence_shapes([(row_kw(q)["cost"], 4) for q in range(len(DETS))])
    odo.set_sequence_detectors(DETS, np.zeros(len(DETS), dtype=np.int32), 1)
    odo.set_sequence_params([capi.default_params(**row_kw(q)) for q in range(len(DETS))])
    return ctx, odo


@pytest.mark.parametrize("route", ["step", "replay", "persistent"])
def test_every_sequence_equals_a_one_sequence_object_of_its_detector(oracle, route):
    fr = frames()
    ctx, odo = grid_object(route)
    for q, dq in enumerate(DETS):
        got = odo.sequence_detector(q)
        assert (got.window_size, got.nb_guard_cells, got.false_alarm_rate, got.z_min) == (dq[0], dq[1], np.float32(dq[2]), dq[3])
        p = odo.sequence_params(q)
        assert (p.cfar_window_size, p.cfar_false_alarm_rate, p.res, p.cost) == (dq[0], np.float32(dq[2]), row_kw(q)["res"], row_kw(q)["cost"])
    poses, per_sweep = run_route(odo, fr[:, None], route)
    odo.status()  # no cloud lost points, no scan cells
    odo.release(); ctx.close()
    for q in range(len(DETS)):
        c1 = make_ctx(row_kw(q), route)
        o1 = c1.odometry(1)
        p1, s1 = run_route(o1, fr[:, None], route)
        o1.release(); c1.close()
        assert poses[:, q].tobytes() == p1[:, 0].tobytes(), (route, q)
        assert [s[q] for s in per_sweep] == [s[0] for s in s1], (route, q)
    # the detector parameters are not ignored: two windows, two rates
    d01 = np.abs(poses[:, 0, :2] - poses[:, 1, :2]).max()
    d02 = np.abs(poses[:, 0, :2] - poses[:, 2, :2]).max()
    print("trajectories: rate 0.01 / 0.001 differ by %.3e m, window 40 / 150 by %.3e m" % (d01, d02))
    assert d01 > 1e-3 and d02 > 1e-3
    if route != "step":
        return
    # ... and at the bar against the oracle's fuser fed the oracle's clouds
    clouds = {}
    for q, (w, g, pfa, z) in enumerate(DETS):
        if DETS[q] not in clouds:
            clouds[DETS[q]] = [oracle.cfar(fr[t], float(RR), z, 2.5, w, g, pfa, prefix=True) for t in range(T)]
    for q in range(len(DETS)):
        fu = oracle.Fuser(oracle.default_params(**{k: v for k, v in row_kw(q).items() if not k.startswith("cfar_") and k != "filter_type"}))
        for t in range(T):
            e = np.array(fu.process_cloud(clouds[DETS[q]][t]))
            S = fu.last_summary()
            no = max(int(S.outer_iterations), 0)
            ec = (int(S.outer_iterations), [int(v) for v in S.inner_iterations[:min(no, 8)]], int(S.num_residuals), int(fu.num_keyframes), len(fu.last_cells()))
            Sd, nc, nk = per_sweep[t][q]
            Sd = capi.RegSummary.from_buffer_copy(Sd)
            nd = max(int(Sd.outer_iterations), 0)
            gc = (int(Sd.outer_iterations), [int(v) for v in Sd.inner_iterations[:min(nd, 8)]], int(Sd.num_residuals), nk, nc)
            pose = poses[t, q]
            print("row %d sweep %d: counts %r / %r, pose diff %.2e m %.2e rad" % (q, t, gc, ec, np.abs(pose[:2] - e[:2]).max(), abs(pose[2] - e[2])))
            if t > 0:
                assert gc == ec, (q, t, gc, ec)
            else:
                assert gc[4] == ec[4], (q, t, gc, ec)  # (the first sweep registers nothing: its cell count)
            assert np.all(np.abs(pose[:2] - e[:2]) < 1e-4) and abs(pose[2] - e[2]) < 1e-5, (q, t, pose, e)


def test_refusals_leave_the_object_unchanged_and_usable():
    fr = frames()[:3]
    # a k-strongest object has no detector
    ctx = capi.Context(capi.default_params(**dict(BASE, filter_type=capi.FILTER_KSTRONG, z_min=60.0)), OA, OR)
    odo = ctx.odometry(2)
    with pytest.raises(capi.CfearError, match="rc=-3"):
        odo.set_sequence_detectors(DETS[:2])
    odo.release(); ctx.close()
    ctx = capi.Context(capi.default_params(**row_kw(0)), OA, OR)
    odo = ctx.odometry(3)
    with pytest.raises(capi.CfearError, match="rc=-3"):  # as before: a source map of the k-strongest kind
        odo.set_sequence_sources(np.zeros(3, dtype=np.int32), 1)
    good = [DETS[0], DETS[2], DETS[3]]
    odo.set_sequence_detectors(good, [0, 0, 0], 1)

    def unchanged():
        assert odo.n_sources == 1
        for q in range(3):
            d = odo.sequence_detector(q)
            assert (d.window_size, d.nb_guard_cells, d.false_alarm_rate, d.z_min) == (good[q][0], good[q][1], np.float32(good[q][2]), good[q][3])

    for bad, field in (((0, 10, 0.01, 20.0), "window_size"), ((40, -1, 0.01, 20.0), "nb_guard_cells"), ((40, 10, 0.0, 20.0), "false_alarm_rate"),
                       ((40, 10, -0.5, 20.0), "false_alarm_rate"), ((40, 10, float("nan"), 20.0), "false_alarm_rate"), ((40, 10, float("inf"), 20.0), "false_alarm_rate"),
                       ((40, 10, 0.01, float("inf")), "z_min")):
        with pytest.raises(capi.CfearError, match=r"rc=-1.*row 2.*%s" % field):
            odo.set_sequence_detectors([DETS[1], DETS[1], bad], [0, 0, 0], 1)
        unchanged()
    with pytest.raises(capi.CfearError, match=r"rc=-1.*row 1.*source"):
        odo.set_sequence_detectors([DETS[1]] * 3, [0, 1, 0], 1)
    with pytest.raises(capi.CfearError, match=r"rc=-1.*row 0.*source"):
        odo.set_sequence_detectors([DETS[1]] * 3, [-1, 0, 0], 1)
    with pytest.raises(capi.CfearError, match=r"rc=-1.*n_sources"):
        odo.set_sequence_detectors([DETS[1]] * 3, [0, 0, 0], 4)
    with pytest.raises(capi.CfearError, match=r"rc=-1.*n_rows"):
        odo.set_sequence_detectors([DETS[1]] * 2, [0, 0], 1)
    unchanged()
    # the table follows the detectors: a row that disagrees with its sequence's detector is refused by name, one that agrees is taken
    def rows_of(dets):
        return [capi.default_params(**dict(BASE, cfar_window_size=d[0], cfar_nb_guard_cells=d[1], cfar_false_alarm_rate=d[2], z_min=d[3])) for d in dets]
    for field, v in (("cfar_window_size", 41), ("cfar_nb_guard_cells", 11), ("cfar_false_alarm_rate", 0.02), ("z_min", 21.0)):
        rows = rows_of(good)
        setattr(rows[1], field, v)
        with pytest.raises(capi.CfearError, match=r"rc=-1.*row 1.*%s" % field):
            odo.set_sequence_params(rows)
    odo.set_sequence_params(rows_of(good))
    with pytest.raises(capi.CfearError, match=r"rc=-1.*row 0.*cfar_false_alarm_rate"):  # detectors the table would then disagree with
        odo.set_sequence_detectors([DETS[1], DETS[2], DETS[3]], [0, 0, 0], 1)
    unchanged()
    # the cloud route takes one cloud per sequence
    import torch
    xyi = torch.zeros((3, 8, 3), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(3, dtype=torch.int32, device="cuda")
    with pytest.raises(capi.CfearError, match="rc=-3"):
        odo.step_cloud_device(xyi.data_ptr(), 8, cnt.data_ptr())
    # usable; and only before the first sweep since create / reset
    odo.step_host(fr[0][None])
    with pytest.raises(capi.CfearError, match="rc=-1.*reset"):
        odo.set_sequence_detectors(good, [0, 0, 0], 1)
    odo.step_host(fr[1][None])
    first = odo.poses().copy()
    odo.reset()  # keeps the detectors
    unchanged()
    odo.step_host(fr[0][None]); odo.step_host(fr[1][None])
    assert odo.poses().tobytes() == first.tobytes()
    # NULL: the context's detector, one sweep per sequence
    odo.reset()
    odo.set_sequence_params(None)
    odo.set_sequence_detectors(None)
    assert odo.n_sources == 3
    d = odo.sequence_detector(1)
    assert (d.window_size, d.nb_guard_cells, d.false_alarm_rate, d.z_min) == (DETS[0][0], DETS[0][1], np.float32(DETS[0][2]), DETS[0][3])
    odo.step_host(np.stack([fr[0]] * 3)); odo.step_host(np.stack([fr[1]] * 3))
    p = odo.poses()
    assert p[0].tobytes() == first[0].tobytes() and p[1].tobytes() == p[0].tobytes()
    # detectors without a source map: one sweep per sequence, and the cloud route stays open
    odo.reset()
    odo.set_sequence_detectors(good)
    assert odo.n_sources == 3
    odo.step_host(np.stack([fr[0]] * 3)); odo.step_host(np.stack([fr[1]] * 3))
    assert odo.poses()[0].tobytes() == first[0].tobytes()
    odo.status()
    odo.release(); ctx.close()


def test_replay_grid_runs_a_cfar_grid_in_one_object():
    """replay.replay_grid(frames, replay.cfar_grid(...)): the reference's experiment as one object - every row over the one source sweep"""
    from cfear_radarodometry_code_public_amd import replay
    fr = frames()
    rows = replay.cfar_grid(capi.default_params(**BASE), cfar_false_alarm_rate=[0.01, 0.001], cfar_window_size=[40, 150])
    assert [(r.cfar_window_size, r.cfar_false_alarm_rate) for r in rows] == [(d[0], np.float32(d[2])) for d in DETS[:4]]
    out = replay.replay_grid(fr, rows, piece=5)
    assert out["poses"].shape == (T, 4, 3)
    for q in (0, 3):
        c1 = make_ctx(row_kw(q), "persistent")
        o1 = c1.odometry(1)
        p1 = np.concatenate([o1.replay_host(fr[t0:t0 + 5, None])["pose"] for t0 in range(0, T, 5)], axis=0)
        o1.release(); c1.close()
        assert out["poses"][:, q].tobytes() == p1[:, 0].tobytes(), q
    assert np.abs(out["poses"][:, 0, :2] - out["poses"][:, 3, :2]).max() > 1e-3
