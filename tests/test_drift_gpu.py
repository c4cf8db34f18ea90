"""KITTI drift of a batch's trajectories on the device (cfear_drift_plan_create / cfear_drift_device / cfear_drift_host, csrc/drift.hip)
against the host metric (kitti.drift_by_length, the numpy twin of kitti_drift_by_length in include/cfear_hip/kitti_metric.hpp).

Tolerances, from the arithmetic and not from what the kernel gives:
  translation: relative 1e-10 - a mean of 203 norms, each from O(10) double operations; the summation order adds at most 203 eps;
  rotation: relative 1e-7 - acos near 1 turns an error dc of a few eps into dc / r; with the smallest single-segment rotation error
    of these inputs (~9.4e-7 rad, asserted > 1e-8 below) that is <= 1e-9 rad on one segment of 203 against a row mean >= 6.7e-3 rad;
  counts: exact;  device against device: bit for bit (the 184 bytes of a row)."""
import ctypes as C

import numpy as np
import pytest

from cfear_radarodometry_code_public_amd import capi, kitti, replay, synth

pytestmark = pytest.mark.gpu

N, B = 400, 257  # B crosses a wavefront (64) and a 256-thread workgroup
T_TOL, R_TOL = 1e-10, 1e-7


def traj(n, seed, step=3.0):
    rng = np.random.default_rng(seed)
    th = np.cumsum(rng.normal(0, 0.02, n))
    v = step * (0.8 + 0.4 * rng.random(n))
    return np.stack([np.cumsum(v * np.cos(th)), np.cumsum(v * np.sin(th)), th], 1)


def planar_batch(xyt):
    """[..., 3] (x, y, theta) -> [..., 4, 4]"""
    return kitti.poses_from_xyt(xyt.reshape(-1, 3)).reshape(xyt.shape[:-1] + (4, 4))


class Problem:
    def __init__(self):
        self.g = traj(N, 1234)
        self.gt = kitti.poses_from_xyt(self.g)
        self.est = self.g[:, None, :] + np.cumsum(np.random.default_rng(99).normal(0, [0.02, 0.02, 2e-3], (N, B, 3)), 0)  # [n, B, 3]
        self.seg = kitti.segments(self.gt)
        self._ref = {}

    def ref(self, q, n=N):
        """the host metric of row q over the first n poses (computed once)"""
        if (q, n) not in self._ref:
            self._ref[(q, n)] = kitti.drift_by_length(self.gt[:n], kitti.poses_from_xyt(self.est[:n, q]))
        return self._ref[(q, n)]


@pytest.fixture(scope="module")
def problem():
    return Problem()


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(capi.default_params(), 400, 3360)
    yield c
    c.close()


@pytest.fixture(scope="module")
def plan(ctx, problem):
    p = ctx.drift_plan(problem.gt)
    yield p
    p.release()


@pytest.fixture(scope="module")
def clean(plan, problem):
    """all 257 rows, packed [n, B, 3], through the host route"""
    return plan.score(problem.est)


def raw(rows):
    return np.ascontiguousarray(rows).view(np.uint8).reshape(len(rows), 184)


def rel(a, b):
    return abs(a - b) / abs(b) if b != 0 else abs(a)


def assert_row(d, ref, what):
    assert int(d["segments"]) == ref["segments"] and d["segments_by_length"].tolist() == ref["by_length"]["segments"], what
    assert int(d["reserved"]) == 0
    worst_t = [rel(float(d["translation_percent"]), ref["translation_percent"])]
    worst_r = [rel(float(d["rotation_deg_per_100m"]), ref["rotation_deg_per_100m"])]
    for li in range(8):
        t, r = float(d["translation_percent_by_length"][li]), float(d["rotation_deg_per_100m_by_length"][li])
        if ref["by_length"]["segments"][li] == 0:
            assert t == 0.0 and r == 0.0, (what, li)
        else:
            worst_t.append(rel(t, ref["by_length"]["translation_percent"][li]))
            worst_r.append(rel(r, ref["by_length"]["rotation_deg_per_100m"][li]))
    assert max(worst_t) <= T_TOL and max(worst_r) <= R_TOL, (what, max(worst_t), max(worst_r))
    return max(worst_t), max(worst_r)


def test_against_the_host_metric_all_rows(problem, clean):
    p = problem
    # the conditioning the tolerances rest on, from the host side alone
    assert len(p.seg) == 203
    dist = np.concatenate([[0.0], np.cumsum(np.linalg.norm(np.diff(p.gt[:, :3, 3], axis=0), axis=1))])
    margin = min(np.min(np.abs(dist - (dist[f] + ln))) for f in range(0, N, kitti.STEP) for ln in kitti.LENGTHS)
    assert margin > 1e-6, margin  # no dist[i] so close to a threshold that two roundings of dist could choose different segments
    r_min = np.inf
    E = planar_batch(p.est)  # [n, B, 4, 4]
    for first, last, li in p.seg:
        e = np.linalg.inv(np.linalg.inv(E[first]) @ E[last]) @ (np.linalg.inv(p.gt[first]) @ p.gt[last])
        r_min = min(r_min, np.arccos(np.clip(0.5 * (np.trace(e[:, :3, :3], axis1=1, axis2=2) - 1.0), -1.0, 1.0)).min())
    assert r_min > 1e-8, r_min
    assert clean.shape == (B,) and clean.dtype == capi.DRIFT_DTYPE
    worst = np.array([assert_row(clean[q], p.ref(q), "row %d" % q) for q in range(B)])
    print("threshold margin %.3g m, smallest segment rotation %.3g rad; worst relative difference: translation %.3g, rotation %.3g"
          % (margin, r_min, worst[:, 0].max(), worst[:, 1].max()))


def test_a_row_does_not_depend_on_its_batch(plan, problem, clean):
    rows = [0, 63, 64, 255, 256]
    for q in rows:
        assert np.array_equal(raw(plan.score(problem.est[:, q:q + 1])), raw(clean[q:q + 1])), q  # alone
    pick = list(range(60)) + rows  # B = 65: the five rows at positions 60..64
    got = plan.score(problem.est[:, pick])
    assert np.array_equal(raw(got), raw(clean[pick]))
    assert np.array_equal(raw(plan.score(problem.est)), raw(clean))  # a second call on the same plan


def test_record_layout_on_the_device(ctx, plan, problem, clean):
    import torch
    rec = np.zeros((N, B), dtype=capi.SWEEP_RECORD_DTYPE)
    rec.view(np.uint8)[...] = 0xA5  # every other field holds a non-zero pattern
    rec["pose"] = problem.est
    d_rec = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    got = plan.score(d_rec, n_sweeps=N, n_sequences=B)  # strides 80 and B * 80
    assert np.array_equal(raw(got), raw(clean))
    assert np.array_equal(d_rec.cpu().numpy(), rec.view(np.uint8).reshape(-1))  # the input is only read
    # ... and asynchronously into a device buffer, packed poses with their own strides
    d_pose = torch.from_numpy(problem.est.copy()).cuda()
    d_out = torch.zeros(B * 184, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert plan.score(d_pose, n_sweeps=N, n_sequences=B, sweep_stride=B * 24, seq_stride=24, out=d_out) is None
    ctx.synchronize()
    assert np.array_equal(d_out.cpu().numpy().reshape(B, 184), raw(clean))
    assert np.array_equal(raw(plan.score(rec)), raw(clean))  # the record array through the host route


def test_a_plan_scores_a_shorter_replay(ctx, plan, problem, clean):
    p = problem
    got = plan.score(p.est, n_sweeps=120)
    assert p.ref(0, 120)["segments"] == 17
    for q in range(B):
        assert_row(got[q], p.ref(q, 120), "row %d, 120 sweeps" % q)
    short = ctx.drift_plan(p.gt[:120])  # the plan of the shorter ground truth: the same segments in the same order
    assert np.array_equal(raw(short.score(p.est[:120])), raw(got))
    short.release()
    for n in (30, 1, 0):  # 84 m: no segment; one pose; none
        z = plan.score(p.est, n_sweeps=n)
        assert not raw(z).any(), n
    longer = np.concatenate([p.est, p.est[-100:] + 1.0], axis=0)  # 500 sweeps against 400 ground-truth poses
    assert np.array_equal(raw(plan.score(longer, n_sweeps=500)), raw(clean))


def test_identical_trajectories(plan, problem):
    d = plan.score(np.repeat(problem.g[:, None, :], 3, axis=1))
    assert np.all(d["segments"] == 203)
    assert np.all(d["translation_percent"] < 1e-9)
    assert np.all(d["rotation_deg_per_100m"] < 1e-5)  # acos one eps below 1 is 1.5e-8 rad: 8.6e-7 deg / 100 m on a 100 m segment


def test_nan_stays_in_its_row(plan, problem, clean):
    est = problem.est.copy()
    est[200, 5, 0] = np.nan
    got = plan.score(est)
    touched = sorted({int(li) for f, l, li in problem.seg if f == 200 or l == 200})
    untouched = [li for li in range(8) if li not in touched]
    assert touched and untouched
    d = got[5]
    assert np.isnan(d["translation_percent"]) and np.isnan(d["rotation_deg_per_100m"])
    assert np.all(np.isnan(d["translation_percent_by_length"][touched])) and np.all(np.isnan(d["rotation_deg_per_100m_by_length"][touched]))
    assert np.array_equal(d["translation_percent_by_length"][untouched], clean[5]["translation_percent_by_length"][untouched])
    assert np.array_equal(d["rotation_deg_per_100m_by_length"][untouched], clean[5]["rotation_deg_per_100m_by_length"][untouched])
    assert int(d["segments"]) == 203 and np.array_equal(d["segments_by_length"], clean[5]["segments_by_length"])
    others = [q for q in range(B) if q != 5]
    assert np.array_equal(raw(got[others]), raw(clean[others]))
    host = kitti.drift_by_length(problem.gt, kitti.poses_from_xyt(est[:, 5]))  # the host metric does the same
    assert np.isnan(host["translation_percent"]) and np.isnan(host["rotation_deg_per_100m"])
    assert [li for li in range(8) if np.isnan(host["by_length"]["rotation_deg_per_100m"][li])] == touched


def test_ground_truth_that_is_not_orthonormal(ctx, problem, tmp_path):
    kitti.write_kitti(tmp_path / "gt.txt", problem.gt)
    gt6 = kitti.read_kitti(tmp_path / "gt.txt")  # 6 decimals
    assert np.abs(gt6[:, :3, :3] @ gt6[:, :3, :3].transpose(0, 2, 1) - np.eye(3)).max() > 1e-8
    rows = list(range(60)) + [63, 64, 255, 256]
    pl = ctx.drift_plan(gt6)
    got = pl.score(problem.est[:, rows])
    pl.release()
    for i, q in enumerate(rows[::4]):
        assert_row(got[4 * i], kitti.drift_by_length(gt6, kitti.poses_from_xyt(problem.est[:, q])), "row %d, rounded ground truth" % q)


def test_refusals_name_the_argument(ctx, plan, problem):
    import torch
    L, h = ctx._L, ctx._h
    err = lambda: L.cfear_last_error(h).decode()
    g34 = np.ascontiguousarray(problem.gt[:, :3, :]).reshape(-1, 12)
    out_plan = C.c_void_p()
    bad = g34.copy()
    bad[7, 11] = np.inf
    for args, name in (((None, N, C.byref(out_plan)), "gt34"), ((g34.ctypes.data, 0, C.byref(out_plan)), "n_gt"),
                       ((bad.ctypes.data, N, C.byref(out_plan)), "gt34"), ((g34.ctypes.data, N, None), "plan")):
        assert L.cfear_drift_plan_create(h, *args) == -1 and name in err(), (name, err())
    d_pose = torch.zeros(N * 4 * 3, dtype=torch.float64, device="cuda")
    d_out = torch.zeros(4 * 184, dtype=torch.uint8, device="cuda")
    h_pose, h_out = np.zeros((N, 4, 3)), np.zeros(4, dtype=capi.DRIFT_DTYPE)
    for fn, poses, out, pn, on in ((L.cfear_drift_device, d_pose.data_ptr(), d_out.data_ptr(), "d_poses", "d_out"),
                                   (L.cfear_drift_host, h_pose.ctypes.data, h_out.ctypes.data, "h_poses", "h_out")):
        ok = dict(plan=plan._h, poses=poses, sweep=96, seq=24, n=N, B=4, out=out)
        for change, name in ((dict(plan=None), "plan"), (dict(poses=None), pn), (dict(out=None), on), (dict(sweep=100), "sweep_stride"),
                             (dict(seq=28), "seq_stride"), (dict(seq=16), "seq_stride"), (dict(B=0), "n_sequences"), (dict(n=-1), "n_sweeps")):
            a = dict(ok, **change)
            assert fn(h, a["plan"], a["poses"], a["sweep"], a["seq"], a["n"], a["B"], a["out"]) == -1, (name, change)
            assert name in err(), (name, err())
        assert fn(h, ok["plan"], ok["poses"], ok["sweep"], ok["seq"], ok["n"], ok["B"], ok["out"]) == 0  # and the context still works
    ctx.synchronize()
    with pytest.raises(capi.CfearError, match="rc=-1.*gt34"):
        ctx.drift_plan(bad.reshape(-1, 3, 4))


# ---- end to end: a small grid replayed and scored --------------------------------------------------------------------------------------------
A, R, RR = 400, 3360, np.float32(0.0595238)  # the frame shape of the grid tests (tests/test_param_grid_gpu.py)


def test_replay_grid_scored_on_the_device():
    T = 24
    frames, _ = synth.world_sequence(T, A, R, RR, seed=11)
    base = capi.default_params(range_res=RR, k_strongest=12, z_min=60.0, res=3.0, weight_intensity=1, weight_opt=0, submap_scan_size=4)
    rows = replay.param_grid(base, res=[2.5, 3.0, 3.5])
    gt = kitti.poses_from_xyt(np.cumsum(np.tile([[1.0, 0.0, 0.0]], (T, 1)), axis=0))
    dev = replay.replay_grid(frames, rows, gt=gt, piece=16, drift_on="device")
    assert len(dev["drift"]) == 3
    for q in range(3):  # 24 m of ground truth: no segment, on either side
        host = kitti.drift(gt, kitti.poses_from_xyt(dev["poses"][:, q]))
        assert dev["drift"][q]["segments"] == host["segments"] == 0
        assert set(dev["drift"][q]) == {"translation_percent", "rotation_deg_per_100m", "segments", "by_length"}
    # a ground truth stretched to 30 m a sweep: segments exist and the numbers are compared
    far = kitti.poses_from_xyt(np.cumsum(np.tile([[30.0, 0.5, 0.01]], (T, 1)), axis=0))
    dev = replay.replay_grid(frames, rows, gt=far, piece=16, drift_on="device")
    host = replay.replay_grid(frames, rows, gt=far, piece=16)
    assert np.array_equal(dev["poses"], host["poses"])
    for q in range(3):
        d, h = dev["drift"][q], host["drift"][q]
        assert set(h) == {"translation_percent", "rotation_deg_per_100m", "segments"}  # the default return value is unchanged
        assert d["segments"] == h["segments"] > 0 and sum(d["by_length"]["segments"]) == d["segments"]
        assert rel(d["translation_percent"], h["translation_percent"]) <= T_TOL
        assert rel(d["rotation_deg_per_100m"], h["rotation_deg_per_100m"]) <= R_TOL
