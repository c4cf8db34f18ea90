"""KITTI drift with the per-length table, the parts that need no GPU: kitti.drift_by_length against kitti.drift and against a direct
restatement, the host-only segment search of the library (cfear_drift_segments) against the numpy one, the cfear_drift layout, and the
new replay_grid argument."""
import ctypes as C
import inspect

import numpy as np
import pytest

from cfear_radarodometry_code_public_amd import capi, kitti, replay


def traj(n, seed, step=3.0):
    rng = np.random.default_rng(seed)
    th = np.cumsum(rng.normal(0, 0.02, n))
    v = step * (0.8 + 0.4 * rng.random(n))
    return np.stack([np.cumsum(v * np.cos(th)), np.cumsum(v * np.sin(th)), th], 1)


@pytest.fixture(scope="module")
def problem():
    g = traj(400, 1234)
    est = g[:, None, :] + np.cumsum(np.random.default_rng(99).normal(0, [0.02, 0.02, 2e-3], (400, 257, 3)), 0)  # [n, B, 3]
    return g, kitti.poses_from_xyt(g), est


def test_inputs_are_the_ones_the_tolerances_were_derived_for(problem):
    g, gt, est = problem
    seg = kitti.segments(gt)
    assert len(seg) == 203 and np.bincount(seg[:, 2], minlength=8).tolist() == [37, 34, 30, 27, 24, 20, 17, 14]
    dist = np.concatenate([[0.0], np.cumsum(np.linalg.norm(np.diff(gt[:, :3, 3], axis=0), axis=1))])
    assert abs(dist[-1] - 1192.85) < 0.01


def test_drift_by_length_against_drift_and_a_restatement(problem):
    g, gt, est = problem
    seg = kitti.segments(gt)
    for q in (0, 100, 256):
        E = kitti.poses_from_xyt(est[:, q])
        a, b = kitti.drift(gt, E), kitti.drift_by_length(gt, E)
        assert b["segments"] == a["segments"] == 203
        assert abs(b["translation_percent"] - a["translation_percent"]) <= 1e-12 * a["translation_percent"]
        assert abs(b["rotation_deg_per_100m"] - a["rotation_deg_per_100m"]) <= 1e-12 * a["rotation_deg_per_100m"]
        bl = b["by_length"]
        assert bl["length_m"] == list(kitti.LENGTHS) and sum(bl["segments"]) == b["segments"]
        for li, ln in enumerate(kitti.LENGTHS):  # each per-length mean, restated
            t, r = [], []
            for first, last, _ in seg[seg[:, 2] == li]:
                e = np.linalg.inv(np.linalg.inv(E[first]) @ E[last]) @ (np.linalg.inv(gt[first]) @ gt[last])
                t.append(np.linalg.norm(e[:3, 3]) / ln)
                r.append(np.arccos(np.clip(0.5 * (np.trace(e[:3, :3]) - 1.0), -1.0, 1.0)) / ln)
            assert bl["segments"][li] == len(t) > 0
            assert abs(bl["translation_percent"][li] - 100.0 * np.mean(t)) <= 1e-12 * 100.0 * np.mean(t)
            assert abs(bl["rotation_deg_per_100m"][li] - np.degrees(np.mean(r)) * 100.0) <= 1e-12 * np.degrees(np.mean(r)) * 100.0


def test_drift_by_length_without_segments():
    gt = kitti.poses_from_xyt(traj(30, 1234))
    for n in (0, 1, 30):
        d = kitti.drift_by_length(gt[:n], gt[:n])
        assert (d["translation_percent"], d["rotation_deg_per_100m"], d["segments"]) == (0.0, 0.0, 0)
        assert d["by_length"]["segments"] == [0] * 8 and d["by_length"]["translation_percent"] == [0.0] * 8 and d["by_length"]["rotation_deg_per_100m"] == [0.0] * 8


@pytest.mark.parametrize("n,expected", [(1, 0), (2, 0), (30, 0), (34, 0), (120, 17), (400, 203)])
def test_segment_search_of_the_library_is_the_numpy_one(hip_lib, problem, n, expected):
    g, gt, est = problem
    got = capi.drift_segments(gt[:n])
    assert got.dtype == np.int32 and got.shape == (expected, 3)
    assert np.array_equal(got, kitti.segments(gt[:n]))
    if n == 120:  # one plan serves a shorter replay: the segments of gt[:n] are those of gt with last < n
        full = capi.drift_segments(gt)
        assert np.array_equal(got, full[full[:, 1] < n])


def test_segment_search_capacity_and_refusals(hip_lib, problem):
    g, gt, est = problem
    g34 = np.ascontiguousarray(gt[:, :3, :]).reshape(-1, 12)
    f, l, k = (np.full(5, -7, dtype=np.int32) for _ in range(3))
    m = C.c_int(-1)
    assert hip_lib.cfear_drift_segments(g34.ctypes.data, 400, f.ctypes.data, l.ctypes.data, k.ctypes.data, 5, C.byref(m)) == -6  # CFEAR_ERR_CAPACITY
    assert m.value == 203
    assert np.array_equal(np.stack([f, l, k], 1), kitti.segments(gt)[:5])
    assert hip_lib.cfear_drift_segments(g34.ctypes.data, 400, None, None, None, 0, C.byref(m)) == -6 and m.value == 203
    assert hip_lib.cfear_drift_segments(None, 400, None, None, None, 0, C.byref(m)) == -1
    assert hip_lib.cfear_drift_segments(g34.ctypes.data, 0, None, None, None, 0, C.byref(m)) == -1
    assert hip_lib.cfear_drift_segments(g34.ctypes.data, 400, None, None, None, 0, None) == -1
    bad = g34.copy()
    bad[17, 3] = np.nan
    assert hip_lib.cfear_drift_segments(bad.ctypes.data, 400, None, None, None, 0, C.byref(m)) == -1
    with pytest.raises(capi.CfearError):
        capi.drift_segments(bad)


def test_drift_layout_matches_the_header():
    assert C.sizeof(capi.Drift) == 184 and capi.DRIFT_DTYPE.itemsize == 184
    order = ["translation_percent", "rotation_deg_per_100m", "translation_percent_by_length", "rotation_deg_per_100m_by_length", "segments",
             "segments_by_length", "reserved"]
    offsets = [0, 8, 16, 80, 144, 148, 180]
    assert [f for f, _ in capi.Drift._fields_] == order and list(capi.DRIFT_DTYPE.names) == order
    for f, off in zip(order, offsets):
        assert getattr(capi.Drift, f).offset == off and capi.DRIFT_DTYPE.fields[f][1] == off, f


def test_replay_grid_scores_on_the_host_by_default():
    p = inspect.signature(replay.replay_grid).parameters["drift_on"]
    assert p.default == "host"
    with pytest.raises(ValueError):
        replay.replay_grid(np.zeros((1, 4, 8), dtype=np.uint8), [capi.Params()], drift_on="elsewhere")
