"""The keyframe graph of the batched routes (cfear_odometry_set_keyframe_recording, keyframes.hip): nodes, odometry constraints and the
scans' cells recorded on the device behind the registration stage - against the oracle's fuser (AddToGraph, odometrykeyframefuser.cpp:
428-445), against numpy for the constraint rule, and against the object's own registrations for the scans rebuilt from the log.

The drive is the replay tests': 35 sweeps of synth.world_sequence played forwards, then backwards (T = 70: more than one 64-sweep chunk);
at ~1 m per sweep and min_keyframe_dist 1.5 every second sweep fuses."""
import math

import numpy as np
import pytest

from cfear_radarodometry_code_public_amd import capi, synth
from test_keyframes_cpu import constraint_numpy

pytestmark = pytest.mark.gpu
RR = np.float32(0.0595238)
A, R, T = 400, 3360, 70
P2P, P2L, P2D = 0, 1, 2
KW = dict(range_res=RR, k_strongest=12, z_min=60.0, res=3.0, weight_intensity=1, weight_opt=4, submap_scan_size=4)
MAX_CELLS = T * 1024  # (a scan of this drive has ~200 cells)
WHAT = capi.KF_NODES | capi.KF_CELLS
REC_FIELDS = ("pose", "final_cost", "outer_iterations", "num_residuals", "n_keyframes", "n_cells", "inner_iterations")
_C = {}


def images():
    if "imgs" not in _C:
        imgs, _ = synth.world_sequence(T // 2, seed=31, world_seed=55)
        _C["imgs"] = np.concatenate([imgs, imgs[::-1]])
    return _C["imgs"]


def frames(B):
    """[T, B, A, R]: sequence q sees the world rotated by q azimuths"""
    if ("frames", B) not in _C:
        imgs = images()
        _C[("frames", B)] = np.ascontiguousarray(np.stack([np.roll(imgs, q, axis=1) if q else imgs for q in range(B)], axis=1))
    return _C[("frames", B)]


def mat(v):
    c, s = math.cos(v[2]), math.sin(v[2])
    return np.array([[c, -s, v[0]], [s, c, v[1]], [0.0, 0.0, 1.0]])


def xyt(M):
    return np.array([M[0, 2], M[1, 2], math.atan2(M[1, 0], M[0, 0])])


def oracle_run(oracle, q, kw=KW, cov_sampling=False):
    """the oracle's Fuser over sequence q's sweeps, once per process -> poses [T, 3], keyframe counts [T], cells of every sweep"""
    key = ("oracle", q, tuple(sorted(kw.items())), cov_sampling)
    if key not in _C:
        fu = oracle.Fuser(oracle.default_params(**kw))
        if cov_sampling:
            fu.set_cov_sampling(True)
        poses, nkf, cells = [], [], []
        for t in range(T):
            poses.append(np.array(fu.process_polar(np.roll(images()[t], q, axis=0) if q else images()[t])))
            nkf.append(fu.num_keyframes)
            cells.append(fu.last_cells())
        _C[key] = (np.array(poses), np.array(nkf), cells)
    return _C[key]


def rule_sweeps(poses, use_keyframe=1, dist=1.5, rot_deg=5.0):
    """KeyFrameBasedFuse (odometrykeyframefuser.cpp:62-73) restated on a trajectory: the sweeps that fuse (the first always does, :171-177)"""
    out, last = [0], mat([0.0, 0.0, 0.0])
    for t in range(1, len(poses)):
        D = np.linalg.inv(last) @ mat(poses[t])
        tn, rot = math.hypot(D[0, 2], D[1, 2]), abs(math.atan2(D[1, 0], D[0, 0]))
        if not use_keyframe or tn > dist or rot > rot_deg * math.pi / 180.0:
            out.append(t)
            last = mat(poses[t])
    return out


def check_nodes(nodes, rec, cov, sweeps, tag):
    """nodes of one sequence against its per-sweep records rec [T], covariances cov [T, 6, 6] and the sweeps expected to have fused"""
    assert list(nodes["sweep"]) == list(sweeps), (tag, list(nodes["sweep"]), list(sweeps))
    assert list(nodes["index"]) == list(range(len(nodes))) and list(nodes["prev"]) == [i - 1 for i in range(len(nodes))], tag
    worst = [0.0, 0.0, 0.0]
    for i, nd in enumerate(nodes):
        t = int(nd["sweep"])
        assert nd["pose"].tobytes() == rec["pose"][t].tobytes(), (tag, i)
        assert int(nd["n_cells"]) == int(rec["n_cells"][t]), (tag, i)
        P = lambda u: rec["pose"][u] if u >= 0 else np.zeros(3)
        mot = xyt(np.linalg.inv(mat(P(t - 2))) @ mat(P(t - 1)))
        worst[0] = max(worst[0], float(np.max(np.abs(nd["motion"] - mot))))
        if i == 0:
            assert not nd["motion"].any() and not nd["t_be"].any() and not nd["information"].any(), tag
            continue
        e_t, e_info = constraint_numpy(nd["pose"], nodes[i - 1]["pose"], cov[t])
        worst[1] = max(worst[1], float(np.max(np.abs(nd["t_be"] - e_t))))
        worst[2] = max(worst[2], float(np.max(np.abs(nd["information"] - e_info)) / np.max(np.abs(e_info))))
    print(tag, "nodes", len(nodes), "motion err", worst[0], "t_be err", worst[1], "information rel err", worst[2])
    assert worst[0] <= 1e-12 and worst[1] <= 1e-12 and worst[2] <= 1e-6, (tag, worst)


def log_of(odo):
    """(nodes, cells) of every sequence as bytes-comparable lists"""
    out = []
    for q in range(odo.B):
        nodes = odo.keyframes(q)
        out.append((nodes, [odo.keyframe_cells(q, i) for i in range(len(nodes))]))
    return out


def base_runs():
    """B = 3 rolled copies through the four routes of test 1, once per process"""
    if "base" in _C:
        return _C["base"]
    B = 3
    fr = frames(B)
    ctx = capi.Context(capi.default_params(**KW), A, R)
    out = {}
    # recording off, the default route (persistent workgroups at B = 3)
    odo = ctx.odometry(B)
    out["off"] = odo.replay_host(fr)
    assert not odo.status(per_sequence=True).any()
    odo.release()
    # recording on at the default REPLAY_PERSISTENT_MAX (the recorder takes the replay off the persistent kernel), with the covariances
    odo = ctx.odometry(B)
    odo.record_keyframes(WHAT, T, MAX_CELLS)
    out["on"], out["cov"] = odo.replay_host(fr, covariances=True)
    out["log_on"], out["counts_on"] = log_of(odo), odo.keyframe_counts()
    out["status_on"] = odo.status(per_sequence=True)
    odo.release()
    ctx.tune(capi.TUNE_REPLAY_PERSISTENT_MAX, 0)
    odo = ctx.odometry(B)
    odo.record_keyframes(WHAT, T, MAX_CELLS)
    out["on0"] = odo.replay_host(fr)
    out["log_on0"] = log_of(odo)
    odo.release()
    ctx.tune(capi.TUNE_REPLAY_PERSISTENT_MAX, 256)
    # one cfear_odometry_step_host per sweep with recording on: the record rebuilt from what the reading calls give
    odo = ctx.odometry(B)
    odo.record_keyframes(WHAT, T, MAX_CELLS)
    step = np.zeros((T, B), dtype=capi.SWEEP_RECORD_DTYPE)
    for t in range(T):
        odo.step_host(fr[t])
        P = odo.poses()
        for q in range(B):
            S, nc, nk = odo.summary(q)
            step[t, q]["pose"], step[t, q]["n_cells"], step[t, q]["n_keyframes"] = P[q], nc, nk
            if t > 0:
                step[t, q]["final_cost"], step[t, q]["outer_iterations"], step[t, q]["num_residuals"] = S.final_cost, S.outer_iterations, S.num_residuals
                step[t, q]["inner_iterations"] = list(S.inner_iterations[:8])
    out["step"], out["log_step"] = step, log_of(odo)
    odo.release()
    ctx.close()
    _C["base"] = out
    return out


def logs_equal(a, b):
    assert len(a) == len(b)
    for (na, ca), (nb, cb) in zip(a, b):
        assert na.tobytes() == nb.tobytes()
        assert len(ca) == len(cb) and all(x.tobytes() == y.tobytes() for x, y in zip(ca, cb))


def test_recording_changes_nothing_and_is_the_same_on_every_route():
    r = base_runs()
    for name in ("on", "on0", "step"):
        for f in REC_FIELDS:
            assert r[name][f].tobytes() == r["off"][f].tobytes(), (name, f)
    logs_equal(r["log_on"], r["log_on0"])
    logs_equal(r["log_on"], r["log_step"])
    recorded, dropped = r["counts_on"]
    assert list(recorded) == [len(n) for n, _ in r["log_on"]] and not dropped.any() and not r["status_on"].any()
    assert all(25 <= len(n) <= 45 for n, _ in r["log_on"])  # roughly every second sweep


@pytest.mark.parametrize("sampling", [False, True])
def test_nodes_are_the_fusers_keyframes(oracle, sampling):
    """node sweeps = where the keyframe rule fires on the ORACLE's trajectory; poses, cell counts and motions = the records'; constraints =
    numpy on the node poses and the sweep's cov_current - the registration's, and with cost sampling on the sampled one"""
    B = 3
    r = base_runs()
    if not sampling:
        rec, cov, logs = r["on"], r["cov"], r["log_on"]
    else:
        ctx = capi.Context(capi.default_params(**KW), A, R)
        odo = ctx.odometry(B)
        odo.set_cov_sampling(True)
        odo.record_keyframes(capi.KF_NODES, T, 0)
        rec, cov = odo.replay_host(frames(B), covariances=True)
        logs = [(odo.keyframes(q), None) for q in range(B)]
        with pytest.raises(capi.CfearError, match="rc=-1"):
            odo.keyframe_cells(0, 0)  # nodes only
        with pytest.raises(capi.CfearError, match="rc=-1"):
            odo.keyframe_scans(0, [0])
        odo.release(); ctx.close()
        # the sampled covariance is another matrix than the registration's on (nearly) every sweep: the check below tells them apart
        differ = np.mean([not np.allclose(cov[t, q], r["cov"][t, q], rtol=1e-3) for t in range(1, T) for q in range(B)])
        assert differ > 0.8, differ
        for f in ("pose", "n_cells", "n_keyframes"):
            assert rec[f].tobytes() == r["on"][f].tobytes(), f
    for q in range(B):
        poses, nkf, _ = oracle_run(oracle, q)
        sweeps = rule_sweeps(poses)
        fused = np.cumsum([1 if t in set(sweeps) else 0 for t in range(T)])
        assert list(nkf) == [min(int(v), KW["submap_scan_size"]) for v in fused], q  # the rule as restated is the oracle's
        check_nodes(logs[q][0], rec[:, q], cov[:, q], sweeps, "sampling=%s q=%d" % (sampling, q))


def test_cells_are_the_scans_cells(oracle):
    """every node of sequence 0: the recorded cells against the oracle fuser's scan of that sweep"""
    nodes, cells = base_runs()["log_on"][0]
    _, _, ocells = oracle_run(oracle, 0)
    worst = {f: 0.0 for f in ("mean", "normal", "cov", "scale")}
    for nd, c in zip(nodes, cells):
        o = ocells[int(nd["sweep"])]
        assert len(c) == len(o) == int(nd["n_cells"]), int(nd["index"])
        assert np.array_equal(c["nsamples"], o["nsamples"]), int(nd["index"])
        for f in worst:
            worst[f] = max(worst[f], float(np.max(np.abs(c[f] - o[f]) / (1.0 + np.abs(o[f])))))
    print("cells vs the oracle fuser's, worst |d| / (1 + |ref|):", worst)
    for f in worst:
        assert worst[f] <= 1e-9, worst  # allclose(rtol = atol = 1e-9): the project's cell bar


def register_again(ctx, odo, B, rec, tag, sequences):
    """for every node j >= 4: scans of keyframes j-4 .. j from the log, the four node poses and the guess pose[sweep - 1] o motion_j -> the
    registration of that sweep, against the sweep's record"""
    worst, n = [0.0, 0.0, 0.0], 0
    for q in sequences:
        nodes = odo.keyframes(q)
        assert len(nodes) > 8
        for j in range(4, len(nodes)):
            t = int(nodes[j]["sweep"])
            scans = odo.keyframe_scans(q, list(range(j - 4, j + 1)))
            guess = xyt(mat(rec["pose"][t - 1, q]) @ mat(nodes[j]["motion"]))
            _, P, _, S = ctx.register(scans, np.vstack([nodes["pose"][j - 4:j], guess]))
            for s in scans:
                s.release()
            e = rec[t, q]
            no = min(max(int(e["outer_iterations"]), 0), 8)
            assert (S.outer_iterations, S.num_residuals) == (int(e["outer_iterations"]), int(e["num_residuals"])), (tag, q, j)
            assert list(S.inner_iterations[:no]) == list(e["inner_iterations"][:no]), (tag, q, j)
            worst[0] = max(worst[0], abs(S.final_cost - e["final_cost"]) / abs(e["final_cost"]))
            worst[1] = max(worst[1], float(np.max(np.abs(P[-1, :2] - e["pose"][:2]))))
            worst[2] = max(worst[2], abs(P[-1, 2] - e["pose"][2]))
            n += 1
    print(tag, "registrations", n, "final_cost rel err", worst[0], "pose err", worst[1], worst[2])
    assert worst[0] <= 1e-9 and worst[1] <= 1e-4 and worst[2] <= 1e-5, (tag, worst)


def test_the_log_is_enough_to_register_again():
    B = 3
    ctx = capi.Context(capi.default_params(**KW), A, R)
    odo = ctx.odometry(B)
    odo.record_keyframes(WHAT, T, MAX_CELLS)
    rec = odo.replay_host(frames(B))
    register_again(ctx, odo, B, rec, "P2L", range(B))
    # the rebuilt scans' cells: the recorded fields bit for bit, the rest as the header says
    nodes = odo.keyframes(1)
    kc = odo.keyframe_cells(1, 3)
    s = odo.keyframe_scans(1, [3])[0]
    c = s.cells()
    assert s.size == len(kc) == int(nodes[3]["n_cells"])
    for f in ("mean", "normal", "cov", "scale", "nsamples"):
        assert c[f].tobytes() == kc[f].tobytes(), f
    assert np.all(c["valid"] == 1) and not c["sum_intensity"].any() and not c["avg_intensity"].any()
    assert np.array_equal(c["orth"], np.stack([-kc["normal"][:, 1], kc["normal"][:, 0]], axis=1))
    ev = np.linalg.eigvalsh(np.stack([np.stack([kc["cov"][:, 0], kc["cov"][:, 1]], 1), np.stack([kc["cov"][:, 1], kc["cov"][:, 2]], 1)], 1))
    assert np.allclose(c["lambda_min"], ev[:, 0], rtol=1e-9, atol=1e-12) and np.allclose(c["lambda_max"], ev[:, 1], rtol=1e-9, atol=1e-12)
    s.release()
    n = len(nodes)
    for bad in ([n], [-1], [0, n + 3]):
        with pytest.raises(capi.CfearError, match="rc=-1"):
            odo.keyframe_scans(1, bad)
    odo.release(); ctx.close()
    # P2D for one sequence: the cost that reads the target cells' covariances
    ctx = capi.Context(capi.default_params(**dict(KW, cost=P2D, loss=0)), A, R)
    odo = ctx.odometry(1)
    odo.record_keyframes(WHAT, T, MAX_CELLS)
    rec = odo.replay_host(frames(1))
    register_again(ctx, odo, 1, rec, "P2D", [0])
    odo.release(); ctx.close()


def test_shapes_and_rows(oracle):
    """submap_scan_size 1, 4 and 10 in one object, a row without the keyframe rule, a row with a 50 m rule: nodes against per-row oracles"""
    rows = [dict(KW, submap_scan_size=1), dict(KW, submap_scan_size=4), dict(KW, submap_scan_size=10), dict(KW, use_keyframe=0),
            dict(KW, min_keyframe_dist=50.0)]
    ctx = capi.Context(capi.default_params(**dict(KW, submap_scan_size=10)), A, R)
    odo = ctx.odometry(len(rows))
    odo.set_sequence_shapes([(P2L, kw["submap_scan_size"]) for kw in rows])
    odo.set_sequence_params([capi.default_params(**kw) for kw in rows])
    odo.set_sequence_sources(np.zeros(len(rows), dtype=np.int32), 1)
    odo.record_keyframes(capi.KF_NODES, T, 0)
    rec, cov = odo.replay_host(images()[:, None], covariances=True)
    for q, kw in enumerate(rows):
        poses, nkf, _ = oracle_run(oracle, 0, kw)
        sweeps = rule_sweeps(poses, kw.get("use_keyframe", 1), kw.get("min_keyframe_dist", 1.5))
        fused = np.cumsum([1 if t in set(sweeps) else 0 for t in range(T)])
        assert list(nkf) == [min(int(v), kw["submap_scan_size"]) for v in fused], q
        check_nodes(odo.keyframes(q), rec[:, q], cov[:, q], sweeps, "row %d" % q)
    assert len(odo.keyframes(3)) == T and 1 <= len(odo.keyframes(4)) < len(odo.keyframes(1)) // 2  # (the 5 degree rule still fires on the bends)
    odo.release(); ctx.close()


def test_cfar_object_with_two_detectors_over_one_source():
    """nodes only, oracle-free: the rule restated on the object's own records"""
    import test_cfar_grid_gpu as cg
    fr = cg.frames()
    dets = [cg.DETS[0], cg.DETS[2]]
    kws = [dict(cg.BASE, cfar_window_size=d[0], cfar_nb_guard_cells=d[1], cfar_false_alarm_rate=d[2], z_min=d[3]) for d in dets]
    ctx = capi.Context(capi.default_params(**cg.BASE), cg.OA, cg.OR)
    odo = ctx.odometry(2)
    odo.set_sequence_detectors(dets, np.zeros(2, dtype=np.int32), 1)
    odo.set_sequence_params([capi.default_params(**kw) for kw in kws])
    odo.record_keyframes(capi.KF_NODES, len(fr), 0)
    rec, cov = odo.replay_host(fr[:, None], covariances=True)
    for q in range(2):
        nodes = odo.keyframes(q)
        assert 3 <= len(nodes) <= len(fr)
        check_nodes(nodes, rec[:, q], cov[:, q], rule_sweeps(rec["pose"][:, q]), "cfar %d" % q)
    assert odo.keyframes(0).tobytes() != odo.keyframes(1).tobytes()
    odo.release(); ctx.close()


def test_capacity_reset_and_late_switch():
    B = 3
    r = base_runs()
    fr = frames(B)
    full = r["log_on"]
    ctx = capi.Context(capi.default_params(**KW), A, R)
    # five nodes per sequence
    odo = ctx.odometry(B)
    odo.record_keyframes(WHAT, 5, MAX_CELLS)
    rec = odo.replay_host(fr)
    for f in REC_FIELDS:
        assert rec[f].tobytes() == r["off"][f].tobytes(), f
    recorded, dropped = odo.keyframe_counts()
    assert list(recorded) == [5] * B and list(dropped) == [len(n) - 5 for n, _ in full]
    assert list(odo.status(per_sequence=True)) == [capi.STATUS_KEYFRAMES_DROPPED] * B
    odo.status()  # a full log is no error of the odometry
    for q in range(B):
        assert odo.keyframes(q).tobytes() == full[q][0][:5].tobytes()
    odo.record_keyframes(0, 0, 0)  # the bit goes with the log
    assert not odo.status(per_sequence=True).any()
    with pytest.raises(capi.CfearError, match="rc=-1"):
        odo.keyframe_counts()
    odo.release()
    # the cells end inside keyframe 3: keyframes 0-2 are intact, 3 and later dropped
    n3 = [int(full[q][0]["n_cells"][:3].sum()) for q in range(B)]
    total = [int(full[q][0]["n_cells"].sum()) for q in range(B)]
    cap = max(n3) + 50
    odo = ctx.odometry(B)
    odo.record_keyframes(WHAT, T, max(total))  # every sequence fits ...
    odo.replay_host(fr)
    assert not odo.keyframe_counts()[1].any() and not odo.status(per_sequence=True).any()
    odo.reset()
    odo.record_keyframes(0, 0, 0)  # off at any time
    odo.record_keyframes(WHAT, T, cap)  # ... and now none does: every sequence ends inside its keyframe 3 (their scans have ~200 cells)
    assert all(n3[q] <= cap < n3[q] + int(full[q][0]["n_cells"][3]) for q in range(B)), (n3, cap)
    odo.replay_host(fr)
    recorded, dropped = odo.keyframe_counts()
    assert list(recorded) == [3] * B and list(dropped) == [len(n) - 3 for n, _ in full]
    for q in range(B):
        assert odo.keyframes(q).tobytes() == full[q][0][:3].tobytes()
        for i in range(3):
            assert odo.keyframe_cells(q, i).tobytes() == full[q][1][i].tobytes()
        with pytest.raises(capi.CfearError, match="rc=-1"):
            odo.keyframe_cells(q, 3)
    odo.release()
    # a log that is full for some sequences only: the middle row barely fuses (a 50 m / 360 degree rule), its neighbours overflow five nodes
    rows = [capi.default_params(**KW), capi.default_params(**dict(KW, min_keyframe_dist=50.0, min_keyframe_rot_deg=360.0)), capi.default_params(**KW)]
    logs = {}
    for cap_kf in (T, 5):
        odo = ctx.odometry(B)
        odo.set_sequence_params(rows)
        odo.record_keyframes(capi.KF_NODES, cap_kf, 0)
        odo.replay_host(fr)
        logs[cap_kf] = [odo.keyframes(q) for q in range(B)]
        if cap_kf == 5:
            recorded, dropped = odo.keyframe_counts()
            n = [len(x) for x in logs[T]]
            assert n[1] <= 5 < min(n[0], n[2]), n
            assert list(recorded) == [5, n[1], 5] and list(dropped) == [n[0] - 5, 0, n[2] - 5]
            assert list(odo.status(per_sequence=True)) == [capi.STATUS_KEYFRAMES_DROPPED, 0, capi.STATUS_KEYFRAMES_DROPPED]
            assert logs[5][1].tobytes() == logs[T][1].tobytes() and all(logs[5][q].tobytes() == logs[T][q][:5].tobytes() for q in (0, 2))
        else:
            assert not odo.keyframe_counts()[1].any()
            assert logs[T][0].tobytes() == full[0][0].tobytes()  # (a row of the context's own values changes nothing)
        odo.release()
    # switching on after a sweep is refused; reset empties the log and recording continues
    odo = ctx.odometry(B)
    odo.record_keyframes(WHAT, T, MAX_CELLS)
    odo.replay_host(fr[:20])
    assert odo.keyframe_counts()[0].all()
    with pytest.raises(capi.CfearError, match="rc=-1.*sweeps"):
        odo.record_keyframes(WHAT, T, MAX_CELLS)
    odo.reset()
    assert not odo.keyframe_counts()[0].any() and not odo.keyframe_counts()[1].any() and not odo.status(per_sequence=True).any()
    odo.replay_host(fr[:10])
    for q in range(B):
        k = int(np.searchsorted(full[q][0]["sweep"], 10))
        assert odo.keyframes(q).tobytes() == full[q][0][:k].tobytes()
    odo.release()
    late = ctx.odometry(1)
    late.step_host(fr[0, :1])
    with pytest.raises(capi.CfearError, match="rc=-1.*sweeps"):
        late.record_keyframes(capi.KF_NODES, 8, 0)
    late.release()
    ctx.close()


def test_replay_device_and_a_blank_sweep():
    import torch
    B = 2
    fr = frames(3)[:, :B].copy()
    fr[33, 1] = 0  # a blank sweep in the middle of sequence 1: whatever the object's own keyframe logic does with it is what the log holds
    ctx = capi.Context(capi.default_params(**KW), A, R)
    a, b = ctx.odometry(B), ctx.odometry(B)
    for o in (a, b):
        o.record_keyframes(WHAT, T, MAX_CELLS)
    rec = a.replay_host(fr)
    d_frames = torch.from_numpy(fr).cuda()
    torch.cuda.synchronize()
    b.replay_device(d_frames, T)
    ctx.synchronize()
    logs_equal(log_of(a), log_of(b))
    for q in range(B):
        nodes = a.keyframes(q)
        assert [int(v) for v in nodes["n_cells"]] == [int(rec["n_cells"][int(t), q]) for t in nodes["sweep"]]
        for nd in nodes:
            assert nd["pose"].tobytes() == rec["pose"][int(nd["sweep"]), q].tobytes()
    assert int(rec["n_cells"][33, 1]) == 0
    assert a.keyframes(0).tobytes() == base_runs()["log_on"][0][0].tobytes()  # the neighbour is untouched
    recorded, dropped = a.keyframe_counts()
    assert not dropped.any() and list(recorded) == [len(a.keyframes(q)) for q in range(B)]
    a.release(); b.release(); ctx.close()


def test_scans_from_the_log_in_the_kd_tree_parity_mode():
    """cfear_tune NN_TIE_RULE = 2: the scans rebuilt from the log carry the kd-tree the parity mode's search walks - three at once, each
    answering GetClosestIdx exactly as a scan built by cfear_scan_from_cells from the same cells"""
    ctx = capi.Context(capi.default_params(**KW), A, R)
    ctx.tune(capi.TUNE_NN_TIE_RULE, 2)
    odo = ctx.odometry(1)
    odo.record_keyframes(WHAT, 16, 16 * 1024)
    rec = odo.replay_host(images()[:12])
    nodes = odo.keyframes(0)
    assert len(nodes) >= 4 and [int(v) for v in nodes["n_cells"]] == [int(rec["n_cells"][int(t), 0]) for t in nodes["sweep"]]
    scans = odo.keyframe_scans(0, [0, 2, 3])
    rng = np.random.default_rng(5)
    for s, i in zip(scans, (0, 2, 3)):
        cells = s.cells()
        assert len(cells) == int(nodes[i]["n_cells"])
        twin = ctx.scan_from_cells(cells)
        q = np.concatenate([cells["mean"][::3] + rng.normal(size=(len(cells[::3]), 2)) * 0.7, rng.uniform(-150, 150, size=(200, 2))])
        got, exp = s.closest(q, 2.0), twin.closest(q, 2.0)
        assert np.array_equal(got, exp) and (got >= 0).sum() > len(cells) // 4
        twin.release(); s.release()
    odo.release(); ctx.close()


def test_replay_grid_and_the_command_line_carry_the_graph(tmp_path):
    """replay.replay_grid(keyframes=...) with its default capacities over two rows, and replay.main --store_graph"""
    from cfear_radarodometry_code_public_amd import readers, replay
    n = 24
    rows = [capi.default_params(**KW), capi.default_params(**dict(KW, min_keyframe_dist=3.0))]
    full = base_runs()["log_on"][0]
    out = replay.replay_grid(images()[:n], rows, keyframes="cells")
    assert not out["keyframes_dropped"].any() and len(out["keyframes"]) == len(out["keyframe_cells"]) == 2
    k = int(np.searchsorted(full[0]["sweep"], n))
    assert out["keyframes"][0].tobytes() == full[0][:k].tobytes()  # row 0 is the context's own parameters: the drive of base_runs, cut at n
    assert all(a.tobytes() == b.tobytes() for a, b in zip(out["keyframe_cells"][0], full[1][:k]))
    assert 3 <= len(out["keyframes"][1]) < k
    for q in range(2):
        nodes = out["keyframes"][q]
        assert [int(v) for v in nodes["n_cells"]] == [int(out["records"]["n_cells"][int(t), q]) for t in nodes["sweep"]]
        assert [len(c) for c in out["keyframe_cells"][q]] == [int(v) for v in nodes["n_cells"]]
    nodes_only = replay.replay_grid(images()[:n], rows, keyframes="nodes")
    assert "keyframe_cells" not in nodes_only and all(a.tobytes() == b.tobytes() for a, b in zip(nodes_only["keyframes"], out["keyframes"]))
    assert "keyframes" not in replay.replay_grid(images()[:4], rows)
    # the command line: an Oxford PNG directory of the first sweeps -> the g2o text of the same run's nodes
    d = tmp_path / "radar"
    d.mkdir()
    for i in range(8):
        ts = 1547131046353776 + i * 250000
        readers.write_png_gray8(d / ("%d.png" % ts), readers.oxford_png_rows(images()[i], ts + np.arange(A) * 625), filter_type=2)
    g = tmp_path / "graph.g2o"
    res = replay.main(["--oxford_png_dir", str(d), "--est_directory", str(tmp_path / "est"), "--range-res", "0.0595238", "--z-min", "60", "--res", "3.0",
                       "--submap_scan_size", "4", "--weight_option", "4", "--store_graph", str(g)])
    k8 = int(np.searchsorted(full[0]["sweep"], 8))
    assert res["keyframes"] == k8 and res["keyframes_dropped"] == 0
    back = replay.read_g2o(g)
    for f in ("index", "prev", "pose", "t_be"):
        assert back[f].tobytes() == full[0][:k8][f].tobytes(), f
    assert open(g).read() == replay.g2o_text(full[0][:k8])
