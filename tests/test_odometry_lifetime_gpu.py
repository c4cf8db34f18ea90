"""Who owns the device memory of a batched odometry object, a context and a drift plan (csrc/common.h: DevBuf): a buffer that grows,
is released or is created late changes no result, destroying everything gives all of it back, and a refused call leaves the object as
it was.

Equality is bit for bit: the sequences are independent and no arithmetic depends on the size of a buffer. The object under test walks
every grow path from its smallest size up; the object it is compared with is given every buffer once, at its final size (one replay of
all the sweeps; the larger sampling design and the larger surface requested before the first sweep), and is otherwise driven alike."""
import numpy as np
import pytest
import torch

from cfear_radarodometry_code_public_amd import capi
import test_param_grid_gpu as pg

pytestmark = pytest.mark.gpu

A, R = pg.A, pg.R
B = 3
BASE = dict(pg.BASE, cost=pg.P2L, submap_scan_size=3)
CFAR = dict(BASE, z_min=20.0, filter_type=capi.FILTER_CACFAR, cfar_window_size=10, cfar_nb_guard_cells=20, cfar_false_alarm_rate=0.01)
SRC = np.array([0, 1, 0], dtype=np.int32)


def frames(T):
    """[T, B, A, R]: the short synthetic drives of tests/test_param_grid_gpu.py, one per sequence"""
    return np.ascontiguousarray(np.stack([pg.drive("canyon", 24, 10 + q, 20 + q)[:T] for q in range(B)], axis=1))


def state(odo, samples=False):
    out = [odo.poses().tobytes(), odo.covariances().tobytes(), odo.status(per_sequence=True).tobytes()]
    for q in range(odo.B):
        S, n_cells, n_keyframes = odo.summary(q)
        out += [bytes(S), n_cells, n_keyframes]
    if samples:
        for q in range(odo.B):
            costs, sampled = odo.cov_samples(q)
            out += [costs.tobytes(), sampled]
    return out


def surface(odo, res, width):
    s, n_used, itr_used, poses_used = odo.surface(res, width, details=True)
    return [s.cpu().numpy().tobytes(), n_used.tobytes(), itr_used.tobytes(), poses_used.tobytes()]


def walk(odo, fr, grow):
    """Every optional buffer of a k-strongest object -> what was read at each stage. grow: from the smallest size up; otherwise every
    buffer at its final size from the start. fr: [13, B, A, R]."""
    got = {}
    odo.set_surface_recording(True)
    if not grow:
        odo.set_cov_sampling(True, samples_per_axis=3)
        odo.set_cov_sampling(False)
        odo.surface(0.25, 3)
    # replay: chunk, staging, record and per-sweep covariance buffers
    if grow:
        assert odo.replay_host(fr[:2], records=False) is None
        rec, cov = odo.replay_host(fr[2:8], covariances=True)
    else:
        rec, cov = odo.replay_host(fr[:8], covariances=True)
        rec, cov = rec[2:], cov[2:]
    got["replay"] = [rec.tobytes(), cov.tobytes()] + state(odo)
    # cost sampling: 8, then 27 samples (the first step_host creates the object's staging buffer)
    for spa, t in ((2, 8), (3, 9)):
        odo.set_cov_sampling(True, samples_per_axis=spa)
        odo.step_host(fr[t])
        got["sampling %d" % spa] = state(odo, samples=True)
    got["surface small"] = surface(odo, 0.5, 1)
    got["surface large"] = surface(odo, 0.25, 3)
    # a source map (two sweeps per step: smaller slot buffers, the staging and chunk buffers released), then none again
    odo.reset()
    odo.set_sequence_sources(SRC, 2)
    odo.step_host(fr[10, :2])
    got["source map"] = state(odo, samples=True)
    rec = odo.replay_host(fr[11:13, :2])
    got["source map replay"] = [rec.tobytes()] + state(odo, samples=True)
    odo.reset()
    odo.set_sequence_sources(None)
    # phase times on, read, off
    odo.phase_times(None, light=True)
    odo.step_host(fr[11])
    got["phase times on"] = state(odo, samples=True)
    assert odo.phase_times(True).any()
    odo.phase_times(False)
    odo.step_host(fr[12])
    got["step_host"] = state(odo, samples=True) + surface(odo, 0.25, 3)
    return got


def run(params, script, *args, tune=()):
    ctx = capi.Context(capi.default_params(**params), A, R)
    for k, v in tune:
        ctx.tune(k, v)
    odo = ctx.odometry(B)
    try:
        return script(odo, *args)
    finally:
        odo.release(); ctx.close()


def assert_same(grown, fresh):
    assert list(grown) == list(fresh)
    for stage in grown:
        assert grown[stage] == fresh[stage], stage


def test_growth_does_not_change_results():
    fr = frames(13)
    grown, fresh = run(BASE, walk, fr, True), run(BASE, walk, fr, False)
    assert_same(grown, fresh)
    assert grown["sampling 2"] != grown["sampling 3"] and grown["surface small"] != grown["surface large"]  # (the stages are not one answer)


def walk_replay(odo, fr, grow, and_step):
    """2 sweeps, then the rest (grow) or all at once -> records and covariances from sweep 2 on; fr: [T (+ 1 for the step), B, A, R]"""
    T = len(fr) - (1 if and_step else 0)
    if grow:
        odo.replay_host(fr[:2], records=False)
        rec, cov = odo.replay_host(fr[2:T], covariances=True)
    else:
        rec, cov = odo.replay_host(fr[:T], covariances=True)
        rec, cov = rec[2:], cov[2:]
    got = {"replay": [rec.tobytes(), cov.tobytes()] + state(odo)}
    if and_step:
        odo.step_host(fr[T])
        got["step"] = state(odo)
    return got


@pytest.mark.parametrize("persistent_max", [256, 0])
def test_growth_does_not_change_results_ca_cfar(persistent_max):
    fr = frames(9)
    tune = [(capi.TUNE_REPLAY_PERSISTENT_MAX, persistent_max)]
    assert_same(run(CFAR, walk_replay, fr, True, True, tune=tune), run(CFAR, walk_replay, fr, False, True, tune=tune))


def test_growth_does_not_change_results_large_submap():
    fr = frames(12)
    params = dict(BASE, submap_scan_size=8, min_keyframe_dist=0.3)  # the first size past the 8-scan kernels: another pair_cap, a longer scan ring
    assert_same(run(params, walk_replay, fr, True, False), run(params, walk_replay, fr, False, False))


def test_nothing_is_left_behind():
    """Free device memory after five cycles of create-everything / destroy-everything against free memory after one.
    The bound is a decline of 0 bytes: allocation and free are deterministic here, every cycle asks for the same blocks, and an owner that
    frees all it allocated (as the hand-kept lists before DevBuf did) gives each of them back. Nothing between the two readings allocates
    through torch (the surfaces go into tensors made beforehand)."""
    fr = frames(13)
    gt = np.tile(np.eye(4), (300, 1, 1))
    gt[:, 0, 3] = 1.5 * np.arange(300)  # 450 m: segments of 100 to 400 m
    poses = np.zeros((300, B, 3))
    poses[:, :, 0] = gt[:, None, 0, 3] * [1.0, 1.01, 0.98]
    dev = torch.device("cuda:0")
    out = {w: torch.empty((B, capi.surface_dims(res, w)[0], capi.surface_dims(res, w)[0]), dtype=torch.float64, device=dev) for res, w in ((0.5, 1), (0.25, 3))}

    class Odo(capi.Odometry):  # surface() into the tensors above
        def surface(self, res, width, details=False):
            c = self._ctx
            n_used, itr_used, poses_used = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32), np.zeros((B, 64, 3))
            c._check(c._L.cfear_odometry_surface(c._h, self._h, float(res), int(width), out[width].data_ptr(), n_used.ctypes.data, itr_used.ctypes.data,
                                                 poses_used.ctypes.data), "cfear_odometry_surface")
            c.synchronize()
            return out[width], n_used, itr_used, poses_used

    def cycle():
        ctx = capi.Context(capi.default_params(**BASE), A, R)
        odo = Odo(ctx, B)
        walk(odo, fr, True)
        plan = ctx.drift_plan(gt)
        drift = plan.score(poses)
        assert drift["segments"][0] > 0
        plan.release(); odo.release(); ctx.close()
        ctx = capi.Context(capi.default_params(**CFAR), A, R)
        odo = ctx.odometry(B)
        walk_replay(odo, fr[:9], True, True)
        odo.release(); ctx.close()

    cycle()
    torch.cuda.synchronize(dev)
    free0 = torch.cuda.mem_get_info(dev)[0]
    for _ in range(5):
        cycle()
    torch.cuda.synchronize(dev)
    free1 = torch.cuda.mem_get_info(dev)[0]
    print("free device memory after the warm-up cycle %d bytes, after five more %d bytes: decline %d bytes" % (free0, free1, free0 - free1))
    assert free0 - free1 <= 0


@pytest.mark.parametrize("params", [BASE, CFAR], ids=["k_strongest", "ca_cfar"])
@pytest.mark.parametrize("overlap", [0, 2])
def test_streams_are_given_back(params, overlap):
    """An object's streams (the overlap mode's, the replay's) leave the context's list when the object goes: the context synchronizes after
    the release, a second object on the same context runs like the first, and both like one on a fresh context. (With CA-CFAR the
    library runs without overlap streams whatever the tune says: the replay stream is the one given back.)"""
    fr = frames(4)

    def context():
        ctx = capi.Context(capi.default_params(**params), A, R)
        ctx.tune(capi.TUNE_ODOMETRY_OVERLAP, overlap)
        return ctx

    def drive(ctx):
        odo = ctx.odometry(B)
        odo.step_host(fr[0]); odo.step_host(fr[1])
        odo.replay_host(fr[2:4])  # (the replay stream exists from here on)
        got = state(odo)
        odo.release()
        ctx.synchronize()  # waits for no stream that is gone
        return got

    ctx = context()
    first, second = drive(ctx), drive(ctx)
    ctx.close()
    ctx = context()
    fresh = drive(ctx)
    ctx.close()
    assert first == second and first == fresh


def test_a_refused_call_leaves_the_object_usable():
    fr = frames(4)

    def script(odo, refusals):
        def refused():
            if not refusals:
                return
            n_sources = odo.n_sources
            with pytest.raises(capi.CfearError, match="rc=-3"):
                odo.set_cov_sampling(True, samples_per_axis=9)  # more than 8 per axis
            with pytest.raises(capi.CfearError, match="rc=-1"):
                odo.set_sequence_sources(np.array([0, 2, 1], dtype=np.int32), 2)  # an entry out of range
            assert odo.n_sources == n_sources
        got = {}
        refused()  # on a fresh object: nothing allocated yet
        odo.set_cov_sampling(True, samples_per_axis=2)
        odo.set_surface_recording(True)
        odo.step_host(fr[0]); odo.step_host(fr[1])
        got["first steps"] = state(odo, samples=True)
        refused()  # with the sampling buffers in use
        odo.step_host(fr[2])
        got["next step"] = state(odo, samples=True) + surface(odo, 0.5, 1)
        odo.reset()
        odo.set_sequence_sources(SRC, 2)
        refused()  # with a source map set: it stays
        odo.step_host(fr[3, :2])
        got["with a source map"] = state(odo, samples=True)
        return got

    assert_same(run(BASE, script, True), run(BASE, script, False))
