"""The host side of the cost-sampling covariance (csrc/cov_design.h: linspace, cov_sample_design, jacobi10, lstsq10_svd, pinv10_svd) through
host/cov_design_check, against numpy and without a GPU. The fit decides whether a covariance is "convex"; cfear_cov_by_sampling and
cfear_odometry_set_cov_sampling run exactly this code.

The design is compared exactly (the same IEEE operations in the same order). The fit is compared with np.linalg.lstsq / np.linalg.pinv at
Eigen's rank threshold, rcond = min(m, 10) * eps (SVDBase::threshold(), what bdcSvd().solve() at odometrykeyframefuser.cpp:337 uses).

Tolerances are not chosen: for every input, numpy's own two routes to the same quantity - lstsq (gelsd, divide and conquer) and
pinv(A) @ b (gesdd) - are compared, and the header may be FACTOR = 10 times as far from lstsq as pinv(A) @ b is (one-sided Jacobi and the
two LAPACK drivers are all backward stable and round differently). "pred": the predictions A c, max |difference| / max |reference|
(they are all of the cost's size). "hess": the Hessian entries 2 c0, 2 c1, 2 c2, c3, c4, c5 (full-rank inputs only), each relative to
itself, the largest of the six: the yaw entry is 1e3 .. 1e4 times the others, the convexity verdict needs each to its own scale, and
normalised by the largest entry numpy's two routes agree to 1e-15 .. 1e-14 only because they share their bidiagonalisation and with it
their error there (against a 60-digit solution of the same inputs both are 2e-13 .. 5e-13 off in that entry, the Jacobi fit 1e-14 .. 3e-14:
the header is the closest of the three). Measured here with numpy's bundled OpenBLAS on x86-64 (python tests/test_cov_design_cpu.py
prints them again):

    input            m    rank  pred       hess
    ref steps 3      27   10    7.83e-15   3.11e-13
    ref steps 4      64   10    7.83e-15   4.27e-13
    ref steps 5      125  10    8.09e-15   2.20e-13
    ref steps 2      8    7     1.03e-15   -          (m < 10: the minimum-norm solution)
    ref steps 1      1    1     1.29e-16   -
    yaw_range 0      27   6     7.77e-16   -          (duplicate and zero columns)

The same bound holds P b (pinv10_svd) against lstsq10_svd's c. The Moore-Penrose identities A P A = A and P A P = P get ten times the
residual np.linalg.pinv itself leaves on the input (max |residual| / max |A| resp. max |P|: PENROSE below, 2.2e-16 .. 1.2e-15 and
1.2e-16 .. 5.6e-13, printed by the same command).

The weak-yaw design (sigma_min ~ 35 eps sigma_max, tests/test_getcost_gpu.py::test_cov_by_sampling_keeps_a_weak_yaw_direction_like_eigen)
gets the rank assertion - as many singular values above the threshold as numpy finds at that rcond: all ten - and that GPU test's
tolerance on the yaw entry (rtol 0.3: a singular value at 35 eps is known to ~10 %), nothing tighter.

Every case runs through the plain build; the -fsanitize=address,undefined build of the same stand-alone program runs every command once
(skipped where the sanitizer runtime is missing)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cfear_radarodometry_code_public_amd", "host")
EPS = np.finfo(float).eps
XY, YAW = 0.4, 0.0043625  # the reference's ranges (cov_sampling_xy_range, cov_sampling_yaw_range)
FACTOR = 10.0
# numpy's lstsq against its pinv(A) @ b per input (the table above): (pred, hess)
MEASURED = {"ref3": (7.83e-15, 3.11e-13), "ref4": (7.83e-15, 4.27e-13), "ref5": (8.09e-15, 2.20e-13), "ref2": (1.03e-15, None),
            "ref1": (1.29e-16, None), "yaw0": (7.77e-16, None)}
# ... and what np.linalg.pinv leaves of A P A = A and of P A P = P on each
PENROSE = {"ref3": (8.9e-16, 2.2e-13), "ref4": (1.2e-15, 3.8e-13), "ref5": (1.1e-15, 5.6e-13), "ref2": (4.4e-16, 2.5e-14), "ref1": (2.2e-16, 1.2e-16),
           "yaw0": (6.7e-16, 1.6e-15)}
INPUTS = {"ref3": (XY, YAW, 3), "ref4": (XY, YAW, 4), "ref5": (XY, YAW, 5), "ref2": (XY, YAW, 2), "ref1": (XY, YAW, 1), "yaw0": (XY, 0.0, 3)}


def _sanitizer_runtime():
    src = os.path.join(HOST, "_san_probe_cov.cpp")
    exe = os.path.join(HOST, "_san_probe_cov")
    try:
        with open(src, "w") as f:
            f.write("int main() { return 0; }\n")
        ok = subprocess.run(["g++", "-fsanitize=address,undefined", "-o", exe, src], capture_output=True).returncode == 0
        return ok and subprocess.run([exe], capture_output=True).returncode == 0
    finally:
        for p in (src, exe):
            if os.path.exists(p):
                os.remove(p)


@pytest.fixture(scope="module")
def prog():
    subprocess.check_call(["make", "-C", HOST, "cov_design_check"], stdout=subprocess.DEVNULL)
    return os.path.join(HOST, "cov_design_check")


def run(prog, *commands):
    """one array of numbers per command (each command a tuple of words; floats travel as repr, which reads back exactly)"""
    out = subprocess.run([prog] + [repr(float(w)) if isinstance(w, float) else str(w) for c in commands for w in c], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", (out.returncode, out.stderr)  # (a sanitizer report is on stderr and in the exit status)
    lines = [l.split() for l in out.stdout.splitlines()]
    assert len(lines) == len(commands) and all(l[0] == c[0] for l, c in zip(lines, commands))
    return [np.array([float(x) for x in l[1:]]) for l in lines]


def linspace_ref(a, b, n):  # odometrykeyframefuser.cpp:497-524
    if n == 1:
        return np.array([a])
    d = (b - a) / (n - 1.0)
    return np.array([a + d * i for i in range(n - 1)] + [b])


def design(xy, yaw, steps):
    """(offsets [m][3], rows [m][10]) as tests/test_getcost_gpu.py:72-73 states them: yaw outermost, then x, then y"""
    xs, ths = linspace_ref(-xy * 0.5, xy * 0.5, steps), linspace_ref(-yaw * 0.5, yaw * 0.5, steps)
    offs = np.array([[x, y, z] for z in ths for x in xs for y in xs])
    rows = np.array([[x * x, y * y, z * z, x * y, y * z, z * x, x, y, z, 1.0] for z in ths for x in xs for y in xs])
    return offs, rows


def costs(offs, seed):
    """a convex quadratic of the registration's kind (stiff in yaw) plus seeded noise"""
    H = np.array([[30.0, 5.0, 40.0], [5.0, 20.0, -60.0], [40.0, -60.0, 5.0e4]])
    assert np.all(np.linalg.eigvalsh(H) > 0)
    g = np.array([0.3, -0.2, 4.0])
    return 12.5 + offs @ g + 0.5 * np.einsum("ki,ij,kj->k", offs, H, offs) + 1e-3 * np.random.default_rng(seed).standard_normal(len(offs))


def hess(c):
    return np.array([2 * c[0], 2 * c[1], 2 * c[2], c[3], c[4], c[5]])


def far(got, ref):
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


def far_each(got, ref):
    return float(np.max(np.abs(got - ref) / np.abs(ref)))


def rcond(m):
    return min(m, 10) * EPS


# ---- the design ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [1, 2, 3, 5])
def test_design_is_the_references(prog, steps):
    (d,) = run(prog, ("design", XY, YAW, steps))
    m = steps ** 3
    assert d[0] == m and len(d) == 1 + 13 * m
    offs, rows = design(XY, YAW, steps)
    assert np.array_equal(d[1:1 + 3 * m].reshape(m, 3), offs)
    assert np.array_equal(d[1 + 3 * m:].reshape(m, 10), rows)
    if steps == 5:  # ... which is numpy's own linspace here, as the GPU test builds it
        xs, ths = np.linspace(-XY / 2, XY / 2, steps), np.linspace(-YAW / 2, YAW / 2, steps)
        assert np.array_equal(offs, np.array([[x, y, z] for z in ths for x in xs for y in xs]))


def test_linspace_ends_on_end(prog):
    cases = [(-0.2, 0.2, 5), (-0.00218125, 0.00218125, 3), (0.1, 0.7, 7), (-1.0, 1.0 / 3.0, 8), (0.0, 0.0, 4), (-0.2, 0.2, 1), (0.0, 1.0, 0)]
    for (a, b, n), got in zip(cases, run(prog, *[("linspace", a, b, n) for a, b, n in cases])):
        assert len(got) == max(n, 0)
        if n >= 2:
            assert got[-1] == b and got[0] == a and np.array_equal(got, linspace_ref(a, b, n))
        elif n == 1:
            assert got[0] == a


# ---- the fit -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(INPUTS))
def test_lstsq_against_numpy(prog, name):
    xy, yaw, steps = INPUTS[name]
    offs, A = design(xy, yaw, steps)
    m = len(A)
    b = costs(offs, seed=steps)
    c, sv = run(prog, ("lstsq", xy, yaw, steps) + tuple(float(v) for v in b), ("svd", xy, yaw, steps))
    ref, _, rank, s = np.linalg.lstsq(A, b, rcond=rcond(m))
    assert int(np.sum(sv[1:] > sv[0])) == rank  # the directions kept
    assert sv[0] == min(m, 10) * EPS * np.max(sv[1:])
    tol_pred, tol_hess = MEASURED[name]
    print(name, "m", m, "rank", rank, "pred", far(A @ c, A @ ref), "of", FACTOR * tol_pred, "hess", far_each(hess(c), hess(ref)) if tol_hess else "-")
    assert far(A @ c, A @ ref) <= FACTOR * tol_pred
    if tol_hess is not None:
        assert rank == 10
        assert far_each(hess(c), hess(ref)) <= FACTOR * tol_hess


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_pinv_is_the_same_fit_and_a_pseudo_inverse(prog, name):
    xy, yaw, steps = INPUTS[name]
    offs, A = design(xy, yaw, steps)
    m = len(A)
    bs = [costs(offs, seed=100 + k) for k in range(3)]
    out = run(prog, ("pinv", xy, yaw, steps), *[("lstsq", xy, yaw, steps) + tuple(float(v) for v in b) for b in bs])
    assert out[0][0] == m
    P = out[0][1:].reshape(10, m)
    tol_pred, tol_hess = MEASURED[name]
    for b, c in zip(bs, out[1:]):
        assert far(A @ (P @ b), A @ c) <= FACTOR * tol_pred
        if tol_hess is not None:
            assert far_each(hess(P @ b), hess(c)) <= FACTOR * tol_hess
    own = PENROSE[name]
    got = (far(A @ P @ A, A), far(P @ A @ P, P))
    print(name, "A P A = A", got[0], "numpy", own[0], "P A P = P", got[1], "numpy", own[1])
    assert got[0] <= FACTOR * own[0] and got[1] <= FACTOR * own[1]


def weak_yaw():
    """the yaw range at which the design's smallest singular value is ~35 eps of its largest (the bisection of the GPU test)"""
    steps, yaw = 5, 1e-6
    for _ in range(60):
        sv = np.linalg.svd(design(XY, yaw, steps)[1], compute_uv=False)
        ratio = sv[-1] / sv[0]
        if 30 * EPS < ratio < 42 * EPS:
            break
        yaw *= np.sqrt(35 * EPS / ratio)
    assert 10 * EPS * 2 < ratio < 125 * EPS / 2
    return steps, float(yaw)


def test_lstsq_keeps_a_weak_yaw_direction_like_eigen(prog):
    steps, yaw = weak_yaw()
    offs, A = design(XY, yaw, steps)
    b = costs(offs, seed=5)
    c, sv = run(prog, ("lstsq", XY, yaw, steps) + tuple(float(v) for v in b), ("svd", XY, yaw, steps))
    ref, _, rank, s = np.linalg.lstsq(A, b, rcond=rcond(len(A)))
    assert rank == 10 and np.linalg.lstsq(A, b, rcond=None)[2] == 9  # numpy's default threshold would cut the direction
    assert int(np.sum(sv[1:] > sv[0])) == rank
    print("weak yaw", yaw, "sigma_min / sigma_max", np.min(sv[1:]) / np.max(sv[1:]), "2 c2", 2 * c[2], "numpy", 2 * ref[2])
    assert np.isclose(2 * c[2], 2 * ref[2], rtol=0.3)


# ---- the same commands under the sanitizers, once --------------------------------------------------------------------------------------
def test_every_command_under_the_sanitizers():
    if not _sanitizer_runtime():
        pytest.skip("no -fsanitize=address,undefined runtime for g++ here: the sanitized run does not happen")
    subprocess.check_call(["make", "-C", HOST, "cov_design_check_san"], stdout=subprocess.DEVNULL)
    san = os.path.join(HOST, "cov_design_check_san")
    commands = [("linspace", -0.2, 0.2, 5), ("linspace", -0.2, 0.2, 1), ("linspace", 0.0, 1.0, 0)]
    steps_w, yaw_w = weak_yaw()
    for xy, yaw, steps in list(INPUTS.values()) + [(XY, yaw_w, steps_w)]:
        b = costs(design(xy, yaw, steps)[0], seed=steps)
        commands += [("design", xy, yaw, steps), ("svd", xy, yaw, steps), ("pinv", xy, yaw, steps), ("lstsq", xy, yaw, steps) + tuple(float(v) for v in b)]
    plain = os.path.join(HOST, "cov_design_check")
    subprocess.check_call(["make", "-C", HOST, "cov_design_check"], stdout=subprocess.DEVNULL)
    for a, b in zip(run(san, *commands), run(plain, *commands)):
        assert np.array_equal(a, b)  # (-O2 in both, no contraction on this target: the same numbers)


if __name__ == "__main__":  # the table of the docstring: numpy's two routes against each other
    for name in ["ref3", "ref4", "ref5", "ref2", "ref1", "yaw0"]:
        xy, yaw, steps = INPUTS[name]
        offs, A = design(xy, yaw, steps)
        m = len(A)
        b = costs(offs, seed=steps)
        c, _, rank, _ = np.linalg.lstsq(A, b, rcond=rcond(m))
        Pn = np.linalg.pinv(A, rcond=rcond(m))
        c2 = Pn @ b
        print("%-6s m %3d rank %2d pred %.2e hess %s   A P A = A %.1e  P A P = P %.1e" % (
            name, m, rank, far(A @ c2, A @ c), "%.2e" % far_each(hess(c2), hess(c)) if rank == 10 else "-", far(A @ Pn @ A, A), far(Pn @ A @ Pn, Pn)))
