"""Cost surfaces on the device (GetSurface, n_scan_normal.cpp:29-65): cfear_get_surface against the numpy restatement (surface_ref.py),
its own invariants, the C++ mirror (GetSurface + PrintSurface through host/surface_check), and the batched route
(cfear_odometry_set_surface_recording / cfear_odometry_surface) against the per-call entry point on the same clouds."""
import json
import os
import subprocess

import numpy as np
import pytest

import surface_ref
from cfear_radarodometry_code_public_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cfear_radarodometry_code_public_amd", "host")
A, R, RR = 400, 3360, np.float32(0.0595238)
BASE = dict(range_res=RR, k_strongest=12, z_min=60.0, res=3.0, weight_intensity=1, loss_limit=0.1)


@pytest.fixture(scope="module")
def world():
    imgs, gt = synth.world_sequence(6, seed=29)
    return imgs, gt


def _scans(oracle, ctx, imgs, kw):
    p = oracle.default_params(**kw)
    osc, dsc = [], []
    for img in imgs:
        osc.append(oracle.Scan(oracle.cloud(oracle.filter_polar(img, int(p.z_min), p.k_strongest), p.range_res, p.min_distance), p))
        dsc.append(ctx.scan_create(ctx.filter_polar(img, peaks=False)[0]))
    return p, osc, dsc


def _close(got, exp, rtol):
    assert got.shape == exp.shape
    assert np.array_equal(np.isnan(got), np.isnan(exp))  # NaN exactly where the reference's loops never reach
    m = ~np.isnan(exp)
    assert np.all(np.abs(got[m] - exp[m]) <= rtol * np.maximum(np.abs(exp[m]), 1e-300)), np.max(np.abs(got[m] - exp[m]) / np.abs(exp[m]))


PRIOR = np.diag([0.05 ** 2, 0.04 ** 2, 1.0, 1.0, 1.0, 0.01 ** 2])


@pytest.mark.parametrize("cost,loss,wopt,itr,n,soft,res,width", [
    (1, 1, 4, 2, 3, False, 0.3, 1),   # 8 pixels, 7 visited: a NaN row and column
    (1, 2, 0, 1, 2, True, 0.25, 1),
    (2, 1, 1, 2, 4, False, 0.5, 2),
    (2, 3, 4, 1, 5, True, 0.3, 1),
    (0, 5, 0, 2, 3, True, 0.25, 1),
    (0, 4, 1, 1, 4, False, 0.5, 1),
    (1, 3, 1, 2, 5, False, 0.5, 1),
    (2, 2, 0, 2, 2, False, 0.3, 1),
])
def test_get_surface_matches_restatement(oracle, world, cost, loss, wopt, itr, n, soft, res, width):
    imgs, gt = world
    kw = dict(BASE, cost=cost, loss=loss, weight_opt=wopt)
    ctx = capi.Context(capi.default_params(**kw), A, R)
    p, osc, dsc = _scans(oracle, ctx, imgs[:n], kw)
    poses = gt[:n].copy()
    poses[-1] += [0.11, -0.06, 0.004]
    prior = PRIOR if soft else None
    got = ctx.get_surface(dsc, poses, res, width, itr=itr, prior_cov6=prior)
    exp = surface_ref.surface(oracle, osc, poses, p, itr, res, width, prior)
    _close(got, exp, 1e-9)
    ctx.close()


def test_surface_cell_at_estimate_is_get_cost(world):
    """width 0: one cell, at the round-tripped estimate itself = GetCost's score (same problem, same point)"""
    imgs, gt = world
    for cost in (0, 1, 2):
        ctx = capi.Context(capi.default_params(**dict(BASE, cost=cost, loss=2, weight_opt=4)), A, R)
        dsc = [ctx.scan_create(ctx.filter_polar(img, peaks=False)[0]) for img in imgs[:4]]
        poses = gt[:4].copy()
        poses[-1] += [0.2, 0.1, 7.0]  # (a yaw beyond pi: the round trip wraps it)
        for itr in (1, 2):
            s = ctx.get_surface(dsc, poses, 0.1, 0, itr=itr)
            score, _ = ctx.get_cost(dsc, poses, itr=itr)
            assert s.shape == (1, 1) and abs(s[0, 0] - score) <= 1e-12 * abs(score), (cost, itr, s[0, 0], score)
        ctx.close()


def test_surface_repeats_bit_for_bit_and_large_grid(world):
    imgs, gt = world
    ctx = capi.Context(capi.default_params(**dict(BASE, cost=1, loss=1, weight_opt=4)), A, R)
    dsc = [ctx.scan_create(ctx.filter_polar(img, peaks=False)[0]) for img in imgs[:4]]
    poses = gt[:4].copy()
    a = ctx.get_surface(dsc, poses, 0.05, 2, itr=2)
    b = ctx.get_surface(dsc, poses, 0.05, 2, itr=2)
    assert a.shape == (81, 81) and np.array_equal(a, b, equal_nan=True)
    _, nx, ny = capi.surface_dims(0.05, 2, poses[-1, 0], poses[-1, 1])
    assert np.all(np.isfinite(a[:nx, :ny])) and np.all(np.isnan(a[nx:, :])) and np.all(np.isnan(a[:, ny:]))
    # the cost is smallest near the registered estimate, not at the corners of a 4 m window
    assert a[:nx, :ny].min() < min(a[0, 0], a[nx - 1, ny - 1])
    ctx.close()


def test_surface_without_residuals(oracle, world):
    """nothing is refused for too few residuals: a problem without blocks is all zeros (and no prior: :370-377)"""
    imgs, gt = world
    kw = dict(BASE, cost=1, loss=1, weight_opt=4)
    ctx = capi.Context(capi.default_params(**kw), A, R)
    p, osc, dsc = _scans(oracle, ctx, imgs[:2], kw)
    poses = gt[:2].copy()
    poses[-1, :2] += 500.0  # far from the keyframe: no association
    assert ctx.get_cost(dsc, poses) is None
    got = ctx.get_surface(dsc, poses, 0.5, 1, prior_cov6=PRIOR)
    assert np.all(got == 0.0)
    _close(got, surface_ref.surface(oracle, osc, poses, p, 2, 0.5, 1, PRIOR), 0)
    ctx.close()


def test_mirror_print_surface_matches_python(world, tmp_path):
    """host/surface_check: MapPointNormal, Register, GetSurface, PrintSurface through the C++ mirror; the file is '%g' of the
    Python surface at the same poses and itr_, token for token"""
    from cfear_radarodometry_code_public_amd import build
    build.build()
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    imgs, gt = world
    f = tmp_path / "three.u8"
    imgs[:3].tofile(f)
    out = tmp_path / "surface.txt"
    for soft in (0, 1):
        r = subprocess.run([os.path.join(HOST, "surface_check"), str(f), str(out), "0.3", "1", str(soft)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        meta = json.loads(r.stdout)
        ctx = capi.Context(capi.default_params(**dict(BASE, cost=1, loss=1, weight_opt=4)), A, R)
        dsc = [ctx.scan_create(ctx.filter_polar(img, peaks=False)[0]) for img in imgs[:3]]
        prior = np.array(meta["cov"]).reshape(6, 6) if soft else None
        s = ctx.get_surface(dsc, np.array(meta["poses"]), 0.3, 1, itr=meta["itr"], prior_cov6=prior)
        lines = out.read_text().splitlines()
        assert len(lines) == meta["pixels"] == s.shape[0]
        for i, line in enumerate(lines):
            assert line.split(" ") == ["%g" % v for v in s[i]], i
        ctx.close()


# ---- the batched route ---------------------------------------------------------------------------------------------------
KWB = dict(BASE, cost=1, loss=1, weight_opt=4, use_keyframe=0, compensate=0, submap_scan_size=3)


@pytest.fixture(scope="module")
def drive():
    imgs, gt = synth.world_sequence(30, seed=41)
    rev = np.ascontiguousarray(imgs[:, ::-1])
    return [imgs, rev, np.roll(imgs, 100, axis=1), np.roll(rev, 37, axis=1)]


def _batch(drive, t, B):
    return np.ascontiguousarray(np.stack([drive[q % 4][t] for q in range(B)]))


def test_batched_surfaces_match_per_call(oracle, drive):
    T, B = 30, 64
    ctxs = [capi.Context(capi.default_params(**KWB), A, R) for _ in range(2)]
    odos = [c.odometry(B) for c in ctxs]
    with pytest.raises(capi.CfearError, match="rc=-1"):
        odos[0].surface(0.05, 1)  # neither recording nor sampling is on
    odos[0].set_surface_recording(True)
    ctx = ctxs[0]
    check_at = (1, 7, T - 1)
    for t in range(T):
        batch = _batch(drive, t, B)
        for odo in odos:
            odo.step_host(batch)
        assert np.array_equal(odos[0].poses(), odos[1].poses()), t
        assert np.array_equal(odos[0].covariances(), odos[1].covariances()), t
        for q in range(0, B, 7):
            S0, S1 = odos[0].summary(q)[0], odos[1].summary(q)[0]
            assert bytes(S0) == bytes(S1), (t, q)
        if t == 0:
            s = odos[0].surface(0.05, 1)
            assert tuple(s.shape) == (B, 41, 41) and bool(s.isnan().all())  # no registration on the first sweep
            continue
        if t not in check_at:
            continue
        s, n_used, itr_used, poses_used = odos[0].surface(0.05, 1, details=True)
        s = s.cpu().numpy()
        for q in range(B):
            n = int(n_used[q])
            assert n == min(t + 1, KWB["submap_scan_size"] + 1), (t, q, n)
            imgs = [drive[q % 4][t - n + 1 + i] for i in range(n)]
            dsc = [ctx.scan_create(ctx.filter_polar(img, peaks=False)[0]) for img in imgs]
            exp = ctx.get_surface(dsc, poses_used[q, :n], 0.05, 1, itr=int(itr_used[q]))
            _close(s[q], exp, 1e-12)
        if t == T - 1:  # and the restatement, on a coarser grid, for a few sequences
            s2, n_used, itr_used, poses_used = odos[0].surface(0.25, 1, details=True)
            s2 = s2.cpu().numpy()
            p = oracle.default_params(**KWB)
            for q in (0, 1, 2, 3, 61):
                n = int(n_used[q])
                osc = [oracle.Scan(oracle.cloud(oracle.filter_polar(drive[q % 4][t - n + 1 + i], 60, 12), p.range_res, p.min_distance), p)
                       for i in range(n)]
                _close(s2[q], surface_ref.surface(oracle, osc, poses_used[q, :n], p, int(itr_used[q]), 0.25, 1), 1e-9)
    # kept across reset; after a reset (no step yet) the surfaces are all NaN
    odos[0].reset()
    assert bool(odos[0].surface(0.5, 1).isnan().all())
    odos[0].step_host(_batch(drive, 0, B))
    odos[0].step_host(_batch(drive, 1, B))
    assert not bool(odos[0].surface(0.5, 1).isnan().all())
    odos[0].set_surface_recording(False)
    with pytest.raises(capi.CfearError, match="rc=-1"):
        odos[0].surface(0.5, 1)
    for odo, c in zip(odos, ctxs):
        odo.release(); c.close()
