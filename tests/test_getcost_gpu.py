"""cfear_get_cost (n_scan_normal_reg::GetCost) on the device against the oracle, through the C ABI."""
import numpy as np
import pytest

from cfear_radarodometry_code_public_amd import capi, synth

pytestmark = pytest.mark.gpu
RR = np.float32(0.0595238)


def build(oracle, frames, **kw):
    base = dict(range_res=RR, z_min=60.0, res=3.0, weight_intensity=1)
    base.update(kw)
    po, pg = oracle.default_params(**base), capi.default_params(**base)
    imgs, gt = synth.world_sequence(frames, seed=23)
    ctx = capi.Context(pg, 400, 3360)
    so, sg = [], []
    for t in range(frames):
        slots = oracle.filter_polar(imgs[t], int(po.z_min), po.k_strongest)
        xyi = oracle.cloud(slots, po.range_res, po.min_distance)
        so.append(oracle.Scan(xyi, po))
        sg.append(ctx.scan_create(ctx.cloud_upload(xyi)))
    return po, ctx, so, sg, gt


@pytest.mark.parametrize("cost,loss,wopt,itr", [(1, 1, 4, 1), (1, 1, 0, 2), (0, 1, 4, 2), (2, 2, 4, 2), (1, 4, 3, 3), (2, 0, 1, 1)])
def test_get_cost_matches_oracle(oracle, cost, loss, wopt, itr):
    po, ctx, so, sg, gt = build(oracle, 4, cost=cost, loss=loss, weight_opt=wopt, loss_limit=0.1, regularization=0.1)
    poses = gt[:4].copy()
    poses[3] += [0.12, -0.07, 0.004]
    exp = oracle.get_cost(so, poses, po, itr=itr)
    got = ctx.get_cost(sg, poses, itr=itr)
    assert exp is not None and got is not None
    assert len(got[1]) == len(exp[1]) > 200
    assert np.allclose(got[1], exp[1], rtol=0, atol=1e-9)
    assert abs(got[0] - exp[0]) < 1e-9 * max(1.0, abs(exp[0]))
    ctx.close()


def test_get_cost_false_and_capacity(oracle, hip_lib):
    import ctypes as C
    po, ctx, so, sg, gt = build(oracle, 2, cost=1)
    poses = gt[:2].copy()
    far = poses.copy(); far[1, :2] += 500.0
    assert oracle.get_cost(so, far, po) is None and ctx.get_cost(sg, far) is None  # reference: "too few residuals", false
    # a short residual buffer still reports the full count
    arr = (C.c_void_p * 2)(*[s._h for s in sg])
    P = np.ascontiguousarray(poses)
    res = np.full(8, -1.0)
    score, m = C.c_double(), C.c_int()
    rc = hip_lib.cfear_get_cost(ctx.handle, arr, 2, P.ctypes.data, 2, C.byref(score), res.ctypes.data, 5, C.byref(m))
    exp = oracle.get_cost(so, poses, po, itr=2)
    assert rc == 0 and m.value == len(exp[1]) and np.allclose(res[:5], exp[1][:5], atol=1e-9) and np.all(res[5:] == -1.0)
    ctx.close()


@pytest.mark.parametrize("steps,xy,yaw,cost", [(3, 0.4, 0.0043625, 1), (5, 0.4, 0.0043625, 1), (3, 1.0, 0.02, 2), (2, 0.4, 0.0043625, 0)])
def test_cov_by_sampling_matches_oracle(oracle, steps, xy, yaw, cost):
    """approximateCovarianceBySampling (odometrykeyframefuser.cpp:261-380): all sample poses in one launch"""
    po, ctx, so, sg, gt = build(oracle, 4, cost=cost, loss=1, weight_opt=4, loss_limit=0.1)
    poses = gt[:4].copy()
    ret, P, cov_reg, S = oracle.register(so, poses, po)  # processFrame samples around the registered pose
    itr = S.outer_iterations
    ok_o, cov_o, costs_o = oracle.cov_by_sampling(so, P, po, S.final_cost, S.num_residuals, itr=itr, xy_range=xy, yaw_range=yaw, steps=steps)
    ok_g, cov_g, costs_g = ctx.cov_by_sampling(sg, P, S.final_cost, S.num_residuals, itr=itr, xy_range=xy, yaw_range=yaw, steps=steps)
    assert np.allclose(costs_g, costs_o, rtol=1e-10, atol=1e-10)
    assert ok_g == ok_o
    if ok_o:
        assert np.allclose(cov_g, cov_o, rtol=1e-5, atol=1e-12)
    # independent statement of odometrykeyframefuser.cpp:277-373 in numpy on the device's own sampled costs (the library's least
    # squares is a one-sided Jacobi SVD, the oracle's an eigen-decomposition of the normal matrix: neither is numpy's)
    xs, ths = np.linspace(-xy / 2, xy / 2, steps), np.linspace(-yaw / 2, yaw / 2, steps)
    rows = [[x * x, y * y, z * z, x * y, y * z, z * x, x, y, z, 1.0] for z in ths for x in xs for y in xs]
    c = np.linalg.lstsq(np.array(rows), costs_g, rcond=10 * np.finfo(float).eps)[0]  # Eigen's rank threshold: min(rows, cols) * eps (SVDBase::threshold)
    H = np.array([[2 * c[0], c[3], c[5]], [c[3], 2 * c[1], c[4]], [c[5], c[4], 2 * c[2]]])
    convex = bool(np.all(np.linalg.eigvalsh(H) > 0))
    assert ok_g == (convex and S.num_residuals - 3 != 0)
    if ok_g:
        C3 = 2.0 * np.linalg.inv(H) * (S.final_cost / (S.num_residuals - 3)) * 4.0
        exp = np.eye(6)
        exp[:2, :2] = C3[:2, :2]; exp[5, 5] = C3[2, 2]; exp[0, 5] = C3[0, 2]; exp[1, 5] = C3[1, 2]; exp[5, 0] = C3[2, 0]; exp[5, 1] = C3[2, 1]
        assert np.allclose(cov_g, exp, rtol=1e-6, atol=1e-14)
    ctx.close()


def test_cov_by_sampling_keeps_a_weak_yaw_direction_like_eigen(oracle):
    """Nearly rank-deficient sample design: the yaw range is so small that the yaw^2 column's singular value sits between Eigen's
    rank threshold (min(rows, cols) * eps * sigma_max = 10 eps, SVDBase::threshold(), what bdcSvd().solve() at
    odometrykeyframefuser.cpp:337 uses) and numpy's default (max(rows, cols) * eps = 125 eps with 5 samples per axis). Eigen keeps
    the direction - the fitted Hessian then has the cost's real curvature in yaw and is convex -, the higher threshold would cut it
    (H[2][2] = 0: 'not convex', no covariance)."""
    po, ctx, so, sg, gt = build(oracle, 4, cost=1, loss=1, weight_opt=4, loss_limit=0.1)
    ret, P, cov_reg, S = oracle.register(so, gt[:4].copy(), po)
    steps, xy, eps = 5, 0.4, np.finfo(float).eps
    xs = np.linspace(-xy / 2, xy / 2, steps)

    def design(yaw):
        ths = np.linspace(-yaw / 2, yaw / 2, steps)
        return np.array([[x * x, y * y, z * z, x * y, y * z, z * x, x, y, z, 1.0] for z in ths for x in xs for y in xs])
    yaw = 1e-6
    for _ in range(60):  # geometric bisection on the range: smallest singular value at ~35 eps of the largest
        sv = np.linalg.svd(design(yaw), compute_uv=False)
        ratio = sv[-1] / sv[0]
        if 30 * eps < ratio < 42 * eps:
            break
        yaw *= np.sqrt(35 * eps / ratio)  # sigma_min ~ yaw^2
    assert 10 * eps * 2 < ratio < 125 * eps / 2
    ok_g, cov_g, costs_g = ctx.cov_by_sampling(sg, P, S.final_cost, S.num_residuals, itr=S.outer_iterations, xy_range=xy, yaw_range=yaw, steps=steps)
    Am = design(yaw)

    def fit(rcond):
        c = np.linalg.lstsq(Am, costs_g, rcond=rcond)[0]
        return np.array([[2 * c[0], c[3], c[5]], [c[3], 2 * c[1], c[4]], [c[5], c[4], 2 * c[2]]])
    H_eigen, H_numpy_default = fit(10 * eps), fit(None)
    assert H_numpy_default[2, 2] < 1e-3 * abs(H_eigen[2, 2])  # the direction is gone under the higher threshold
    convex = bool(np.all(np.linalg.eigvalsh(H_eigen) > 0))
    assert convex and ok_g  # the registration cost is convex in yaw around its minimum
    C3 = 2.0 * np.linalg.inv(H_eigen) * (S.final_cost / (S.num_residuals - 3)) * 4.0
    assert np.allclose(cov_g[:2, :2], C3[:2, :2], rtol=1e-3) and np.isclose(cov_g[5, 5], C3[2, 2], rtol=0.3)  # (a singular value at 35 eps is known to ~10 %)
    ctx.close()


@pytest.mark.parametrize("cost,sig", [(1, 1.0), (1, 0.05), (2, 0.2), (0, 1e-3)])
def test_register_soft_matches_oracle(oracle, cost, sig):
    """Register(..., soft_constraints=true) (n_scan_normal.cpp:373-377): poses, iteration counts and covariance"""
    po, ctx, so, sg, gt = build(oracle, 4, cost=cost, loss=1, weight_opt=4, loss_limit=0.1, regularization=0.1)
    poses = gt[:4].copy()
    poses[3] += [0.25, -0.15, 0.01]
    C = np.eye(6) * sig ** 2
    C[0, 1] = C[1, 0] = 0.3 * sig ** 2
    C[0, 5] = C[5, 0] = -0.1 * sig ** 2
    ro = oracle.register_soft(so, poses, C, po)
    rg = ctx.register_soft(sg, poses, C)
    So, Sg = ro[3], rg[3]
    assert Sg.outer_iterations == So.outer_iterations and list(Sg.inner_iterations[:8]) == list(So.inner_iterations[:8])
    assert Sg.num_residuals == So.num_residuals == So.num_residual_blocks * (1 if cost == 1 else 2) + 3
    assert np.all(np.abs(rg[1][:, :2] - ro[1][:, :2]) < 1e-4) and np.all(np.abs(rg[1][:, 2] - ro[1][:, 2]) < 1e-5)
    assert bool(ro[0]) == rg[0]
    assert np.allclose(rg[2], ro[2], rtol=1e-6, atol=1e-12)
    assert abs(Sg.final_cost - So.final_cost) < 1e-9 * max(1.0, So.final_cost)
    ctx.close()


def test_scan_from_cells_round_trip_and_tune_knobs(oracle):
    """cfear_scan_from_cells (raw / transformed-copy maps are built on the host and handed over as cells): a scan rebuilt from the
    downloaded cells of another scan answers GetClosestIdx identically and registers identically; cfear_tune rejects unknown
    keys and its launch-shape knobs change the launch shape and not the results."""
    RRl = np.float32(0.0595238)
    imgs, _ = synth.world_sequence(3, seed=33)
    p = capi.default_params(range_res=RRl, res=3.0, weight_intensity=1, weight_opt=4)
    ctx = capi.Context(p, 400, 3360)
    scans = []
    for t in range(3):
        c, _ = ctx.filter_polar(imgs[t], peaks=False)
        scans.append(ctx.scan_create(c))
    rebuilt = [ctx.scan_from_cells(s.cells()) for s in scans]
    for a, b in zip(scans, rebuilt):
        assert a.size == b.size
        ca, cb = a.cells(), b.cells()
        for f in ("mean", "cov", "normal", "scale", "nsamples"):
            assert np.array_equal(ca[f], cb[f]), f
        rng = np.random.default_rng(1)
        q = ca["mean"][rng.integers(0, len(ca), 300)] + rng.normal(0, 1.5, (300, 2))
        assert np.array_equal(a.closest(q, 2.0), b.closest(q, 2.0))
    poses = np.array([[0, 0, 0], [1.0, 0.02, 0.02], [2.1, 0.08, 0.05]])
    r1 = ctx.register(scans, poses)
    r2 = ctx.register(rebuilt, poses)
    assert np.array_equal(r1[1], r2[1]) and r1[3].outer_iterations == r2[3].outer_iterations
    assert list(r1[3].inner_iterations[:8]) == list(r2[3].inner_iterations[:8])
    # launch-shape knobs: filter occupancy variant / rows per wave
    base = ctx.kstrongest_host(imgs[:2])
    for occ, rows in ((5, 1), (6, 8), (7, 4)):
        ctx.tune(capi.TUNE_FILTER_OCCUPANCY, occ); ctx.tune(capi.TUNE_FILTER_ROWS_PER_WAVE, rows)
        assert np.array_equal(ctx.kstrongest_host(imgs[:2]), base)
    # ... which at two sweeps (800 rows: one per wave whatever the cap) launches one shape three times. Many tiny sweeps on a second context: the
    # three settings give three launch shapes - 1, 6 (ceil(35861 / 6144) under the cap of 8) and 4 rows per wave -, same slots, the oracle's
    n, A2, R2 = 5123, 7, 37
    rng = np.random.default_rng(7)
    small = rng.integers(0, 256, size=(n * A2, R2), dtype=np.uint8)
    quiet = (np.arange(n * A2) // 2) % 3 == 0  # two rows below z_min but for a few bins, four uniform rows, in turn
    small[quiet] = np.where(rng.random((quiet.sum(), R2)) < 0.1, small[quiet], small[quiet] % 60)
    small = small.reshape(n, A2, R2)
    exp = np.stack([oracle.filter_polar(small[s], int(p.z_min), p.k_strongest) for s in range(n)])
    ctx2 = capi.Context(p, A2, R2)
    knobs = ((5, 1), (6, 8), (7, 4))
    shapes = []
    for occ, rows in knobs:
        ctx2.tune(capi.TUNE_FILTER_OCCUPANCY, occ); ctx2.tune(capi.TUNE_FILTER_ROWS_PER_WAVE, rows)
        shapes.append(ctx2.kstrongest_launch_shape(n))
    assert [s[0] for s in shapes] == [1, 6, 4] and len(set(s[1] for s in shapes)) == 3 and [s[2] for s in shapes] == [5, 6, 7]
    for occ, rows in knobs:
        ctx2.tune(capi.TUNE_FILTER_OCCUPANCY, occ); ctx2.tune(capi.TUNE_FILTER_ROWS_PER_WAVE, rows)
        assert np.array_equal(ctx2.kstrongest_host(small), exp)
    ctx2.close()
    with pytest.raises(capi.CfearError):
        ctx.tune(99, 1)
    with pytest.raises(capi.CfearError):
        ctx.scan_from_cells(np.zeros(0, dtype=capi.CELL_DTYPE))
    ctx.close()
