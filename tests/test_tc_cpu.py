"""Time-continuous registration without a GPU: the numpy restatement tc_ref pinned to the C oracle (with a zero velocity it is
Register / Register with the soft prior, decision for decision), its internal consistency (a P2P time-continuous registration is
the plain registration of hand-compensated source cells), and the ABI of cfear_register_time_continuous."""
import ctypes as C

import numpy as np
import pytest

import tc_ref
from cfear_radarodometry_code_public_amd import synth

RR = np.float32(0.0595238)
PRIOR = np.diag([0.05 ** 2, 0.04 ** 2, 1.0, 1.0, 1.0, 0.01 ** 2])


def mk(mod, **kw):
    base = dict(range_res=RR, k_strongest=12, z_min=60.0, res=3.0, weight_intensity=1, weight_opt=4, cost=1, loss=1, loss_limit=0.1,
                regularization=0.1, covar_scale=1.0)
    base.update(kw)
    return mod.default_params(**base)


@pytest.fixture(scope="module")
def world(oracle):
    imgs, gt = synth.world_sequence(6, seed=31, world_seed=555)
    p = mk(oracle)
    scans = [oracle.Scan(oracle.cloud(oracle.filter_polar(imgs[t], 60, 12), RR, 2.5), p) for t in range(6)]
    return scans, gt


def same_registration(ref, exp, pose_tol=(1e-4, 1e-5)):
    """tests/test_register_fuzz_gpu.py::compare between two (ret, poses, cov, summary) results; the first one is tc_ref's"""
    retr, Pr, covr, Sr = ref
    rete, Pe, cove, Se = exp
    n_solves = len(Sr.inner_iterations)
    assert bool(retr) == bool(rete) and Sr.usable == Se.usable and Sr.success == Se.success
    assert Sr.outer_iterations == Se.outer_iterations, (Sr.outer_iterations, Se.outer_iterations)
    assert list(Sr.inner_iterations) == list(Se.inner_iterations[:n_solves]) and not any(Se.inner_iterations[n_solves:8])
    assert list(Sr.termination) == list(Se.termination[:n_solves])
    assert Sr.num_residuals == Se.num_residuals and Sr.num_residual_blocks == Se.num_residual_blocks
    assert np.all(np.abs(Pr[:, :2] - Pe[:, :2]) < pose_tol[0]) and np.all(np.abs(Pr[:, 2] - Pe[:, 2]) < pose_tol[1])
    if Sr.usable:
        assert np.allclose(Se.final_cost, Sr.final_cost, rtol=1e-9, atol=1e-12)
    assert np.allclose(cove, np.zeros((6, 6)) if covr is None else covr, rtol=1e-6, atol=1e-12)


def no_cell_on_the_stamp_edge(scan):
    assert tc_ref.stamp_margin(scan.cells()) >= 1e-9


@pytest.mark.parametrize("cost,loss,wopt,nkf,soft", [(1, 1, 4, 3, False), (2, 1, 4, 2, False), (0, 1, 2, 4, False), (1, 2, 0, 4, True),
                                                     (2, 2, 2, 3, True), (0, 1, 4, 2, True)])
def test_zero_velocity_is_the_oracle_register(oracle, world, cost, loss, wopt, nkf, soft):
    scans, gt = world
    sel = list(range(nkf)) + [nkf]
    sc = [scans[i] for i in sel]
    no_cell_on_the_stamp_edge(sc[-1])
    poses = gt[sel].copy()
    poses[-1] += [0.25, -0.15, 0.01]
    p = mk(oracle, cost=cost, loss=loss, weight_opt=wopt)
    exp = oracle.register_soft(sc, poses, PRIOR, p) if soft else oracle.register(sc, poses, p)
    assert exp[3].usable == 1
    for ccw in (False, True):
        same_registration(tc_ref.register(oracle, sc, poses, p, (0.0, 0.0, 0.0), ccw, PRIOR if soft else None), exp, (1e-9, 1e-9))
    same_registration(tc_ref.register(oracle, sc, poses, p, None, False, PRIOR if soft else None), exp, (1e-9, 1e-9))


def test_zero_velocity_failure_is_the_oracle_failure(oracle, world):
    """no overlap: nothing associates, Register fails without residuals and hands the last pose back"""
    scans, gt = world
    sc = scans[:2]
    poses = gt[:2].copy()
    poses[-1] += [500.0, 300.0, 0.0]
    p = mk(oracle)
    exp = oracle.register(sc, poses, p)
    got = tc_ref.register(oracle, sc, poses, p, (0.0, 0.0, 0.0))
    assert exp[0] == 0 and got[3].num_residuals <= 1 and got[2] is None
    same_registration(got, exp, (1e-12, 1e-12))


@pytest.mark.parametrize("vel,ccw", [((3.5, -0.4, 0.1), False), ((-2.0, 0.5, -0.3), True)])
def test_p2p_is_the_plain_registration_of_compensated_cells(oracle, world, vel, ccw):
    scans, gt = world
    sc = scans[:4]
    no_cell_on_the_stamp_edge(sc[-1])
    poses = gt[:4].copy()
    poses[-1] += [0.2, 0.1, -0.008]
    p = mk(oracle, cost=0, weight_opt=4)
    tc = tc_ref.register(oracle, sc, poses, p, vel, ccw)
    src = sc[-1].cells()
    comp = tc_ref.compensate_cells(src, vel, ccw)
    assert np.max(np.abs(comp["mean"] - src["mean"])) > 0.1  # (the velocity moves the cells by decimetres: something is being tested)
    plain = tc_ref.register(oracle, sc, poses, p, None, False, None, src_cells=comp)
    assert tc[3].usable == 1 and tc_ref.decisions(tc[3]) == tc_ref.decisions(plain[3])
    assert np.allclose(tc[1], plain[1], rtol=0, atol=1e-9) and np.allclose(tc[3].final_cost, plain[3].final_cost, rtol=1e-9)
    assert np.allclose(tc[2], plain[2], rtol=1e-6, atol=1e-12)
    # ... and not the registration of the cells as they are
    raw = tc_ref.register(oracle, sc, poses, p, None)
    assert np.max(np.abs(raw[1][-1] - tc[1][-1])) > 1e-4 or raw[3].num_residual_blocks != tc[3].num_residual_blocks


def test_q19_variant_differs_in_the_restatement(oracle, world):
    """P2L with the corrected mean in the residual (what a reader would expect) is another problem than the reference's"""
    scans, gt = world
    sc = scans[:3]
    poses = gt[:3].copy()
    poses[-1] += [0.2, 0.1, -0.008]
    p = mk(oracle, cost=1)
    a = tc_ref.register(oracle, sc, poses, p, (3.5, -0.4, 0.1), False)
    b = tc_ref.register(oracle, sc, poses, p, (3.5, -0.4, 0.1), False, corrected_residual=True)
    assert a[3].usable == 1 and b[3].usable == 1
    assert np.max(np.abs(a[1][-1, :2] - b[1][-1, :2])) > 1e-4 or abs(a[1][-1, 2] - b[1][-1, 2]) > 1e-5


def test_abi_exports_and_argument_checks(hip_lib):
    """the library exports cfear_register_time_continuous, capi binds it, and a null context / velocity is CFEAR_ERR_INVALID
    before anything touches a device"""
    import subprocess
    from cfear_radarodometry_code_public_amd import capi
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path()]).decode()
    assert " T cfear_register_time_continuous" in out
    assert "cfear_register_time_continuous" in capi.EXPORTS
    fn = hip_lib.cfear_register_time_continuous
    assert fn.restype is C.c_int and len(fn.argtypes) == 9
    assert hasattr(capi.Context, "register_time_continuous")
    poses, vel, cov = np.zeros((2, 3)), np.array([1.0, 0.1, 0.02]), np.zeros(36)
    scans = (C.c_void_p * 2)()
    S = capi.RegSummary()
    CFEAR_ERR_INVALID = -1
    assert fn(None, scans, 2, poses.ctypes.data, vel.ctypes.data, 0, None, cov.ctypes.data, C.byref(S)) == CFEAR_ERR_INVALID
    assert fn(None, scans, 2, poses.ctypes.data, None, 0, None, cov.ctypes.data, C.byref(S)) == CFEAR_ERR_INVALID
    assert np.all(cov == 0) and np.all(poses == 0)
