"""The fuser's soft_constraint and use_guess on the batched routes (cfear_odometry_set_fuser_options), host side: the reference fuser the
GPU tests compare against (tests/fuser_ref.py) is pinned to the oracle's own Fuser, the switches are shown to move the trajectories
of the GPU tests' drives by more than ten times the pose bar (a condition on the reference alone: it is what makes the GPU
comparisons able to fail), the residual / cost accounting of a soft sweep, and the grid / POD helpers."""
import ctypes as C

import numpy as np
import pytest

import fuser_ref as fr


# ---- 1. the Python state machine is the oracle's ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw", [("P2L compensated", dict(fr.BASE, cost=fr.P2L, compensate=1)), ("P2L uncompensated", dict(fr.BASE, cost=fr.P2L, compensate=0)),
                                     ("P2D", dict(fr.BASE, cost=fr.P2D, loss=0)), ("P2P weight_opt 4", dict(fr.BASE, cost=fr.P2P, loss=0, weight_opt=4))])
def test_defaults_reproduce_the_oracle_fuser(oracle, name, kw):
    frames = fr.drive(*fr.SEQS[0])
    assert len(frames) == 12
    got = fr.run(oracle, kw, frames)
    fu = oracle.Fuser(oracle.default_params(**kw))
    for t, img in enumerate(frames):
        e = fu.process_polar(img)
        S = fu.last_summary()
        no = max(int(S.outer_iterations), 0)
        exp = (int(S.outer_iterations), [int(v) for v in S.inner_iterations[:min(no, 8)]], int(S.num_residuals), int(fu.num_keyframes), len(fu.last_cells()))
        g, pose = got[t]
        print("%s sweep %d: counts %r / %r, pose diff %.2e" % (name, t, g, exp, np.abs(pose - e).max()))
        assert g == exp, (name, t, g, exp)
        assert np.all(np.abs(pose - e) <= 1e-12), (name, t, pose, e)
    assert got[-1][0][3] >= 4  # keyframes


# ---- 2. the switches move the GPU tests' trajectories -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cost", sorted(fr.COSTS))
@pytest.mark.parametrize("q", range(len(fr.SEQS)))
def test_switches_move_the_trajectories_of_the_gpu_drives(oracle, cost, q):
    kw, seq = fr.COSTS[cost], fr.SEQS[q]
    traj = {o: np.array([p for _, p in fr.reference(oracle, cost, kw, seq, *o)]) for o in fr.OPTIONS}

    def moved(a, b):
        d = np.abs(traj[a] - traj[b])
        print("%s %r: %r against %r: %.2e m, %.2e rad" % (cost, seq, a, b, d[:, :2].max(), d[:, 2].max()))
        return d[:, :2].max() > 1e-3 or d[:, 2].max() > 1e-4

    assert moved((1, 1), (0, 1)) and moved((1, 0), (0, 0))  # soft against free, under either guess
    assert moved((0, 0), (0, 1)) and moved((1, 0), (1, 1))  # use_guess = 0 against 1, free and soft
    assert fr.reference(oracle, cost, kw, seq, 0, 1)[-1][0][3] >= 4  # four keyframes form


# ---- 3. residual and cost accounting of a soft sweep -------------------------------------------------------------------------------------
@pytest.mark.parametrize("cost", sorted(fr.COSTS))
def test_soft_counts_three_more_residuals_and_no_less_cost(oracle, cost):
    """Residuals: the problem of the FIRST outer iteration is built at the guess, where the prior changes nothing yet - with one outer
    iteration allowed, Register with and without the prior hold the same associations, and the soft one counts three residuals more.
    Cost: the fuser's own soft sweeps - final_cost is the converged problem's cost plus the prior block (a sum of squares), so it is at
    least the prior-free cost at the solution, which is what GetCost gives there (it builds without the prior, n_scan_normal.cpp:202;
    itr = the outer iterations of the Register, as the cost sampling calls it)."""
    p = oracle.default_params(**fr.COSTS[cost])
    p1 = oracle.default_params(**dict(fr.COSTS[cost], max_itr_association=1, min_itr=0))
    fu = fr.Fuser(oracle, p, soft_constraint=1)
    checked = 0
    for t, img in enumerate(fr.drive(*fr.SEQS[0])[:8]):
        fu.process_polar(img)
        if fu.reg_scans is None:
            continue
        guess = np.array(fu.reg_poses)
        guess[-1] = fu.reg_guess
        _, _, _, free = oracle.register(fu.reg_scans, guess, p1)
        _, _, _, soft = oracle.register_soft(fu.reg_scans, guess, np.eye(6), p1)
        assert soft.outer_iterations == free.outer_iterations and soft.inner_iterations[1] == 0  # (one problem was built and solved)
        assert soft.num_residuals == free.num_residuals + 3, (t, soft.num_residuals, free.num_residuals)
        assert soft.num_residual_blocks == free.num_residual_blocks
        S = fu.summary
        assert S.usable and S.num_residuals == S.num_residual_blocks * (1 if cost == "P2L" else 2) + 3
        score, _ = oracle.get_cost(fu.reg_scans, fu.reg_poses, p, itr=S.outer_iterations)
        d = fr.Aff.from_xyt(*fu.reg_guess).xyt() - fu.reg_poses[-1]
        prior = 0.5 * fu.n_cells * float(d @ d)  # 1/2 |L alpha (guess - x)|^2 with L = I, alpha^2 = the current scan's cells
        print("%s sweep %d: residuals %d / %d, final cost %.9g, prior-free cost at the solution %.9g, prior block %.9g" %
              (cost, t, soft.num_residuals, free.num_residuals, S.final_cost, score, prior))
        assert S.final_cost >= score and S.final_cost >= prior > 0
        checked += 1
    assert checked >= 6


# ---- 4. the grid and the POD -----------------------------------------------------------------------------------------------------------
def test_fuser_grid_order():
    from cfear_radarodometry_code_public_amd import capi, replay
    base = capi.Params()
    base.res, base.compensate = 3.0, 1
    rows, opts = replay.fuser_grid(base, compensate=[1, 0], res=[3.0, 3.5], soft_constraint=[0, 1], use_guess=[1, 0])
    got = [(o.soft_constraint, r.compensate, r.res, o.use_guess) for r, o in zip(rows, opts)]
    exp = [(s, c, r, g) for s in (0, 1) for c in (1, 0) for r in (3.0, 3.5) for g in (1, 0)]  # soft outside compensate, use_guess innermost, job 1 first
    assert got == exp
    # radar_ccw nests outside soft_constraint (utils/worker:40-46)
    rows, opts = replay.fuser_grid(base, soft_constraint=[0, 1], radar_ccw=[0, 1])
    assert [(r.radar_ccw, o.soft_constraint) for r, o in zip(rows, opts)] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    # without the fuser's axes: param_grid, and the base options everywhere
    rows, opts = replay.fuser_grid(base, base_options=capi.FuserOptions(1, 0), res=[3.0, 3.5], compensate=[1, 0])
    ref = replay.param_grid(base, res=[3.0, 3.5], compensate=[1, 0])
    assert [bytes(r) for r in rows] == [bytes(r) for r in ref]
    assert all((o.soft_constraint, o.use_guess) == (1, 0) for o in opts)
    with pytest.raises(AttributeError):
        replay.fuser_grid(base, no_such_field=[1])
    with pytest.raises(AttributeError):
        replay.param_grid(base, soft_constraint=[0, 1])  # param_grid itself does not change


def test_fuser_options_pod(hip_lib):
    from cfear_radarodometry_code_public_amd import capi
    assert C.sizeof(capi.FuserOptions) == 8
    assert (capi.FuserOptions.soft_constraint.offset, capi.FuserOptions.use_guess.offset) == (0, 4)
    o = capi.default_fuser_options()
    assert (o.soft_constraint, o.use_guess) == (0, 1)
    o = capi.default_fuser_options(soft_constraint=1)
    assert (o.soft_constraint, o.use_guess) == (1, 1)
    with pytest.raises(AttributeError):
        capi.default_fuser_options(nope=1)
    for name in ("cfear_default_fuser_options", "cfear_odometry_set_fuser_options", "cfear_odometry_fuser_options"):
        assert name in capi.EXPORTS and hasattr(hip_lib, name)
