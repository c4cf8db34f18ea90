"""The k-strongest filter without the axial non-max suppression (kstrongest_kernel<.., PEAKS = false>, csrc/kstrongest.hip): the instantiation the
batched odometry routes launch, because nothing there reads the peak flag (bit 25 of a slot).

cfear_tune FILTER_PEAKS = 0 puts the per-call slot entries on that instantiation too, so its slots can be read back: bits 0..24 - range, intensity,
valid, and with them the order and the zero fill - must equal the oracle's bit for bit and bit 25 must be 0 everywhere. With the knob at 1 or at
its default the per-call entries return the oracle's full words. The batched routes must give the same bytes whether their filter computes the
flag (knob 1) or not (default)."""
import numpy as np
import pytest

from cfear_radarodometry_code_public_amd import capi, synth

import test_kstrongest_gpu as ks

pytestmark = pytest.mark.gpu

LOW25 = np.uint32(0x1FFFFFF)
PEAK = np.uint32(1 << 25)


def run_nopeaks(oracle, img, k, z_min, tune=(), shape=None):
    """knob = 0: bits 0..24 of every slot against the oracle, bit 25 clear. -> the oracle's slots"""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    if img.ndim == 2:
        img = img[None]
    n, A, R = img.shape
    ctx = capi.Context(capi.default_params(k_strongest=k, z_min=float(z_min)), A, R)
    try:
        ctx.tune(capi.TUNE_FILTER_PEAKS, 0)
        for key, v in tune:
            ctx.tune(key, v)
        if shape is not None:
            assert ctx.kstrongest_launch_shape(n)[:2] == shape
        got = ctx.kstrongest_host(img)
    finally:
        ctx.close()
    exp = np.stack([oracle.filter_polar(img[s], z_min, k) for s in range(n)])
    assert not np.any(got & PEAK), "bit 25 set in %d slots (A=%d R=%d k=%d zmin=%d)" % (int(((got & PEAK) != 0).sum()), A, R, k, z_min)
    if not np.array_equal(got & LOW25, exp & LOW25):
        s, b = np.argwhere(((got ^ exp) & LOW25).any(axis=2))[0]
        raise AssertionError("scan %d row %d differs in bits 0..24 (A=%d R=%d k=%d zmin=%d)\n got %s\n exp %s" % (
            s, b, A, R, k, z_min, [hex(x) for x in got[s][b]], [hex(x) for x in exp[s][b]]))
    return exp


# ---- slot level, knob = 0 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,R", [(8, 64), (5, 37), (16, 100), (7, 1), (3, 4000), (24, 3360)])
@pytest.mark.parametrize("k", [1, 12, 40])
def test_uniform_random(oracle, A, R, k):
    rng = np.random.default_rng(A * 7919 + R * 13 + k)
    run_nopeaks(oracle, rng.integers(0, 256, size=(A, R), dtype=np.uint8), k, 60)


def test_heavy_ties(oracle):
    R = 333
    run_nopeaks(oracle, synth.ties_scan(64, R, seed=3), 12, 60)
    run_nopeaks(oracle, synth.ties_scan(64, R, seed=4, levels=(60, 61)), 12, 60)
    run_nopeaks(oracle, synth.ties_scan(64, R, seed=5, levels=(10, 200), p=[0.999, 0.001]), 12, 60)
    run_nopeaks(oracle, synth.ties_scan(64, R, seed=6, levels=(10, 200), p=[0.97, 0.03]), 40, 60)


@pytest.mark.parametrize("val", [0, 59, 60, 255])
@pytest.mark.parametrize("z_min", [0, 60, 255])
def test_constant_rows(oracle, val, z_min):
    run_nopeaks(oracle, np.full((6, 3360), val, dtype=np.uint8), 12, z_min)


def test_zmin_zero_sparse(oracle):
    rng = np.random.default_rng(5)
    img = np.zeros((32, 3360), dtype=np.uint8)
    for b in range(32):
        n = b % 15  # fewer than k non-zero bins on some rows -> zero-valued bins must fill up
        img[b, rng.integers(0, 3360, n)] = rng.integers(1, 256, n)
    run_nopeaks(oracle, img, 12, 0)
    run_nopeaks(oracle, img[:, :9], 12, 0)  # R < k


@pytest.mark.parametrize("R", [40, 25, 24, 23, 16, 13])
@pytest.mark.parametrize("k", [12, 3])
def test_kept_points_at_the_row_ends(oracle, R, k):
    """the rows whose suppression took the edge paths: selection and emit must not depend on them"""
    img = ks.row_end_image(np.random.default_rng(R * 31 + k), 96, R)
    exp = run_nopeaks(oracle, img, k, 60)
    assert np.any(exp & PEAK)  # (the oracle does flag peaks on these rows: masking bit 25 is not vacuous)


def test_batch_edge_rows_and_scan_boundaries(oracle):
    """five scans, strong returns at both ends of every row: the first and last row of a scan are loaded without the scan masking here, and the
    window no longer reaches past the row end"""
    rng = np.random.default_rng(11)
    imgs = rng.integers(0, 256, size=(5, 24, 3360), dtype=np.uint8)
    imgs[:, :, :7] = rng.integers(200, 256, size=(5, 24, 7))
    imgs[:, :, -7:] = rng.integers(200, 256, size=(5, 24, 7))
    exp = run_nopeaks(oracle, imgs, 12, 60)
    assert np.any(exp & PEAK)


def test_seven_rows_per_wave_last_wave_partial(oracle):
    """5 x 127 images, 8603 of them: 43015 rows > 6 * 7168, so under a cap of 7 a wave walks 7 rows (the carried threshold, the scan wrap at every
    phase of a wave), and 43015 is no multiple of 28: the last wave and the last workgroup are partial"""
    A, R, n, k, z_min = 5, 127, 8603, 12, 60
    assert (n * A) % 28 != 0
    rows = ks.mixed_rows(np.random.default_rng(A * R), n * A, R, k, z_min)
    run_nopeaks(oracle, rows.reshape(n, A, R), k, z_min, tune=[(capi.TUNE_FILTER_ROWS_PER_WAVE, 7)], shape=(7, ks.ceil_div(ks.ceil_div(n * A, 7), 4)))


# ---- batched routes: knob 1 against the default, and the per-call API afterwards ------------------------------------------------------------------
A, R, RR = 400, 3360, np.float32(0.0595238)
T, B = 8, 3
BASE = dict(range_res=RR, k_strongest=12, z_min=60.0, res=3.0, weight_intensity=1, weight_opt=4, submap_scan_size=4)
_FRAMES = []


def frames():
    """[T, B, A, R]: a short drive, the same drive with the azimuths reversed, a second drive"""
    if not _FRAMES:
        a = synth.world_sequence(T, A, R, RR, seed=11)[0]
        b = synth.world_sequence(T, A, R, RR, seed=12)[0]
        _FRAMES.append(np.ascontiguousarray(np.stack([a, a[:, ::-1], b], axis=1)))
    return _FRAMES[0]


def state_bytes(odo):
    poses, cov = odo.poses(), odo.covariances()
    return [(poses[q].tobytes(), cov[q].tobytes(), bytes(odo.summary(q)[0]), odo.summary(q)[1:]) for q in range(odo.B)]


def run_route(odo, fr, route):
    """every pose, covariance and registration summary the route gives, as bytes"""
    if route == "replay_host":
        rec, cov = odo.replay_host(fr, covariances=True)
        return [rec.tobytes(), cov.tobytes()] + state_bytes(odo)
    out = []
    if route == "step_device":
        import torch
        dev = torch.from_numpy(fr).cuda()
        torch.cuda.synchronize()
    for t in range(fr.shape[0]):
        if route == "step_device":
            odo.step_device(dev[t])
        else:
            odo.step_host(fr[t])
        out.append(state_bytes(odo))
    return out


def batched(ctx_kw, rows, route, knob, then=None):
    ctx = capi.Context(capi.default_params(**ctx_kw), A, R)
    try:
        if knob is not None:
            ctx.tune(capi.TUNE_FILTER_PEAKS, knob)
        odo = ctx.odometry(B)
        if rows:
            odo.set_sequence_params([capi.default_params(**kw) for kw in rows])
        out = run_route(odo, frames(), route)
        if then:
            then(ctx)
        odo.release()
    finally:
        ctx.close()
    return out


@pytest.mark.parametrize("route", ["step_device", "step_host", "replay_host"])
def test_batched_routes_do_not_depend_on_the_flag(route):
    with_flag = batched(BASE, None, route, 1)
    default = batched(BASE, None, route, None)
    assert len(default) > 0 and default == with_flag
    last = np.frombuffer(default[-1][0][0] if route != "replay_host" else default[2][0], dtype=np.float64)
    assert np.all(np.isfinite(last)) and np.abs(last[:2]).max() > 0.5  # (the drive moved: the routes did register)


@pytest.mark.parametrize("route", ["step_device", "step_host", "replay_host"])
def test_batched_routes_with_per_sequence_k_and_z_min(route):
    """rows with k_strongest < K and their own z_min: the cloud pass takes a window of each bearing's slots by the valid bits and their order"""
    ctx_kw = dict(BASE, k_strongest=40, z_min=50.0)
    rows = [dict(ctx_kw, k_strongest=k, z_min=z) for k, z in ((5, 60.0), (12, 70.0), (40, 50.0))]
    assert batched(ctx_kw, rows, route, None) == batched(ctx_kw, rows, route, 1)


# ---- per-call API: the flag is there, also in a context whose odometry object has just stepped without it --------------------------------------
@pytest.mark.parametrize("knob", [None, 1])
def test_per_call_slots_carry_the_flag_after_a_batched_step(oracle, knob):
    img = frames()[:2, 0]
    exp = np.stack([oracle.filter_polar(img[s], 60, 12) for s in range(2)])
    assert np.any(exp & PEAK)
    seen = []

    def per_call(ctx):
        seen.append(ctx.kstrongest_host(img))
        cloud, peaks = ctx.filter_polar(img[0])
        seen.append((cloud.size, peaks.size))
        cloud.release(); peaks.release()

    batched(BASE, None, "step_host", knob, then=per_call)
    assert np.array_equal(seen[0], exp)  # the full 32-bit words
    n_valid = int((((exp[0] >> 24) & 1) != 0).sum())
    assert 0 < seen[1][1] < seen[1][0] <= n_valid
