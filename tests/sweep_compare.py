"""One sweep of a batched odometry object against the oracle's fuser: the comparison and its bars, shared by the GPU tests that walk sweeps."""
import numpy as np


def assert_sweep_is_the_fusers(odo, q, t, pose, fuser, exp):
    """sequence q of a batched object after sweep t against the oracle's fuser after the same sweep (exp: the pose it returned): cells
    exactly; from the second sweep on keyframes, iteration and residual counts exactly, the pose at 1e-4 m / 1e-5 rad
    (test_odometry_fuzz_gpu.py's many-bearings test and the slot-route cases of test_feature_seams_gpu.py)"""
    S, nc, nk = odo.summary(q)
    So = fuser.last_summary()
    assert nc == len(fuser.last_cells()), (t, q, nc, len(fuser.last_cells()))
    if t > 0:
        assert (nk, S.outer_iterations, S.num_residuals) == (fuser.num_keyframes, So.outer_iterations, So.num_residuals), (t, q)
        assert list(S.inner_iterations[:8]) == list(So.inner_iterations[:8]), (t, q)
        assert np.all(np.abs(pose[:2] - exp[:2]) < 1e-4) and abs(pose[2] - exp[2]) < 1e-5, (t, q, pose, exp)
