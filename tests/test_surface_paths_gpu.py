"""Cost surfaces past the easy corner (surface_dev.h, surface_build_kernel / surface_build_step_kernel / surface_eval_kernel<COST, PPT>):
problems with more residual blocks than the LDS match array holds (the copy-out of surface_build_block takes blocks from LDS and from
memory), the grouped and the general association path, the two-pixels-per-thread tiles, and the batched route in the configurations
the registration supports. The reference is surface_ref.surface_grid (the restatement of test_surface_gpu.py, vectorised over the
pixels; tests/test_surface_cpu.py holds it against surface_ref.surface) at 1e-9 relative, the batched route against cfear_get_surface
on the recorded scans and poses at 1e-12. Every case asserts the regime it is meant to be in (block count against the LDS capacity,
source cells against one block of threads, keyframes against one group, tiles against the two-pixel rule) before it compares, and
prints what it saw ("[regime] ..."; pytest -rA shows the lines)."""
import math
import os

import numpy as np
import pytest

import surface_ref
from match_caps import CSRC, LDS_CAP, REG_BLOCK, _define  # the LDS match array's capacities per cost, one block of source cells
from cfear_radarodometry_code_public_amd import capi, synth

pytestmark = pytest.mark.gpu
A, R, RR = 400, 3360, np.float32(0.0595238)
BASE = dict(range_res=RR, k_strongest=12, z_min=60.0, res=3.0, weight_intensity=1, loss_limit=0.1)
PRIOR = np.diag([0.05 ** 2, 0.04 ** 2, 1.0, 1.0, 1.0, 0.01 ** 2])
CFAR = dict(window_size=40, nb_guard_cells=10, false_alarm_rate=0.01)
COST_NAME = {0: "P2P", 1: "P2L", 2: "P2D"}


SURF_BLOCK = _define("surface_dev.h", "CFEAR_SURFACE_BLOCK")
SURF_CHUNK = _define("surface_dev.h", "CFEAR_SURFACE_CHUNK")


def test_the_constants_this_file_restates():
    assert LDS_CAP == {2: 622, 1: 710, 0: 995} and SURF_BLOCK == 128 and SURF_CHUNK == 256 and REG_BLOCK == 256
    src = open(os.path.join(CSRC, "pipeline.hip")).read()
    assert "(long long)t2 * problems >= 512" in src  # launch_surface_eval's rule, restated by _tiles


def _tiles(pixels, problems):
    """launch_surface_eval: (two-pixel tiles per problem x problems, whether the two-pixel instantiation runs)"""
    t2 = (pixels * pixels + 2 * SURF_BLOCK - 1) // (2 * SURF_BLOCK)
    return t2 * problems, t2 * problems >= 512


def _close(got, exp, rtol):
    assert got.shape == exp.shape
    assert np.array_equal(np.isnan(got), np.isnan(exp))  # NaN exactly where the reference's loops never reach
    m = ~np.isnan(exp)
    if m.any():
        assert np.all(np.abs(got[m] - exp[m]) <= rtol * np.maximum(np.abs(exp[m]), 1e-300)), np.max(np.abs(got[m] - exp[m]) / np.abs(exp[m]))


def _say(*a):
    print("[regime]", *a)


# ---- inputs: once per module ------------------------------------------------------------------------------------------------------
def _drive(T, kind, ws=3, s=5):
    frames = np.empty((T, A, R), dtype=np.uint8)
    for t0, chunk in synth.drive_chunks(T, kind, ws, s, A, R, RR, ccw=False):
        frames[t0:t0 + len(chunk)] = chunk
    return frames


@pytest.fixture(scope="module")
def world():
    return synth.world_sequence(33, seed=29)  # (imgs, gt): test_surface_gpu.py's world, 182 to 223 cells per scan


@pytest.fixture(scope="module")
def canyon():
    return _drive(14, "canyon")  # 518 to 586 cells per scan at k = 12


@pytest.fixture(scope="module")
def street():
    return _drive(6, "street")


def _oscan(oracle, p, img):
    return oracle.Scan(oracle.cloud(oracle.filter_polar(img, int(p.z_min), p.k_strongest), p.range_res, p.min_distance), p)


def _dscan(ctx, img):
    return ctx.scan_create(ctx.filter_polar(img, peaks=False)[0])


@pytest.fixture(scope="module")
def canyon_poses(oracle, canyon):
    """the oracle's own registration of the canyon sweeps, each against up to three before it, per cost: matches as a drive has them"""
    out = {}
    for cost in (0, 1, 2):
        p = oracle.default_params(**dict(BASE, cost=cost, loss=2, weight_opt=4))
        sc = [_oscan(oracle, p, f) for f in canyon[:8]]
        poses = [np.zeros(3)]
        for t in range(1, len(sc)):
            k0 = max(0, t - 3)
            _, P, _, _ = oracle.register(sc[k0:t + 1], np.array(poses[k0:t] + [poses[-1]]), p)
            poses.append(P[-1].copy())
        out[cost] = np.array(poses)
        assert abs(out[cost][-1, 0]) > 1.0  # the vehicle moves
    return out


def _per_call(oracle, kw, imgs, poses, res, width, itr=2, prior=None, tie=0, want_path=None, want_mixed=None, want_nsrc=None, want_nk=None):
    """one cfear_get_surface against surface_grid, after the regime's assertions. want_*: True / False / None (not asserted)"""
    p = oracle.default_params(**kw)
    ctx = capi.Context(capi.default_params(**kw), A, R)
    if tie:
        ctx.tune(capi.TUNE_NN_TIE_RULE, tie)
    osc = [_oscan(oracle, p, img) for img in imgs]
    dsc = [_dscan(ctx, img) for img in imgs]
    exp, nblk = surface_ref.surface_grid(oracle, osc, poses, p, itr, res, width, prior, with_blocks=True)
    nsrc, nk, cap = len(osc[-1].cells()), len(imgs) - 1, LDS_CAP[kw["cost"]]
    S = ctx.register(dsc, poses)[3]  # (its own poses move; the path depends on the tie rule, the keyframes and the source cells only)
    tiles, two = _tiles(exp.shape[0], 1)
    _say("per call %s loss %d itr %d prior %d: blocks %d (LDS capacity %d), source cells %d, keyframes %d, assoc_path %d, grid %d^2, two-pixel tiles %d (%s)"
         % (COST_NAME[kw["cost"]], kw["loss"], itr, prior is not None, nblk, cap, nsrc, nk, S.assoc_path, exp.shape[0], tiles, "PPT 2" if two else "PPT 1"))
    if want_mixed is not None:
        assert (nblk > cap) == want_mixed, (nblk, cap)
    if want_nsrc is not None:
        assert (nsrc > REG_BLOCK) == want_nsrc, nsrc
    if want_nk is not None:
        assert (nk > 4) == want_nk, nk
    if want_path is not None:
        assert S.assoc_path == want_path, S.assoc_path
    got = ctx.get_surface(dsc, poses, res, width, itr=itr, prior_cov6=prior)
    _close(got, exp, 1e-9)
    return ctx, dsc, got, exp


# ---- B: dense problems and the other association paths, per call ------------------------------------------------------------------
@pytest.mark.parametrize("cost,loss,n,itr,soft", [
    (2, 2, 3, 2, False),   # 687 blocks > 622
    (2, 5, 4, 1, True),    # Tukey: the generic loss_eval
    (1, 2, 4, 2, True),    # 1028 > 710
    (1, 3, 3, 1, False),   # 740 > 710: thirty blocks from memory
    (0, 2, 5, 1, False),   # 1486 > 995
    (0, 5, 5, 2, True),
])
def test_mixed_lds_and_memory_blocks(oracle, canyon, canyon_poses, cost, loss, n, itr, soft):
    """more residual blocks than the LDS match array holds: surface_build_block takes the first match_lds_cap from LDS and the rest
    from memory. Canyon scans have more than 256 cells: the grouped path with one group. The grid: 30 x 30, 29 visited either way
    (2 / 0.07 = 28.57), 900 pixels - neither a multiple of the tile nor, with these block counts, of the chunk"""
    kw = dict(BASE, cost=cost, loss=loss, weight_opt=4)
    ctx, dsc, got, exp = _per_call(oracle, kw, canyon[:n], canyon_poses[cost][:n], 0.07, 1, itr, PRIOR if soft else None,
                                   want_path=2, want_mixed=True, want_nsrc=True, want_nk=False)
    assert exp.shape == (30, 30) and np.all(np.isnan(exp[29])) and np.all(np.isnan(exp[:, 29])) and np.all(np.isfinite(exp[:29, :29]))
    ctx.close()


@pytest.mark.parametrize("cost,loss", [(2, 2), (1, 5)])
def test_mixed_blocks_in_one_block_of_cells(oracle, world, cost, loss):
    """a stop: the same sweep five times. At most 256 source cells and four keyframes (association path 1, the matches in registers),
    and nearly every cell matches in every keyframe: more blocks than the P2D and the P2L capacity (P2P's 995 is out of reach of
    4 x 223 cells)"""
    imgs, gt = world
    poses = np.tile(gt[3], (5, 1))
    poses[-1] += [0.05, -0.03, 0.002]
    kw = dict(BASE, cost=cost, loss=loss, weight_opt=4)
    ctx, _, _, _ = _per_call(oracle, kw, [imgs[3]] * 5, poses, 0.07, 1, 2, None, want_path=1, want_mixed=True, want_nsrc=False, want_nk=False)
    ctx.close()


@pytest.mark.parametrize("cost", [0, 1, 2])
def test_more_than_256_source_cells_few_keyframes(oracle, canyon, canyon_poses, cost):
    """the grouped path with one group, everything in LDS (one keyframe)"""
    kw = dict(BASE, cost=cost, loss=2, weight_opt=4)
    ctx, _, _, _ = _per_call(oracle, kw, canyon[:2], canyon_poses[cost][:2], 0.25, 1, 2, PRIOR, want_path=2, want_mixed=False, want_nsrc=True,
                             want_nk=False)
    ctx.close()


@pytest.mark.parametrize("cost,loss,n,mixed", [(1, 2, 9, True), (0, 3, 9, False), (2, 2, 33, True), (0, 2, 33, True), (1, 1, 64, True)])
def test_more_than_four_keyframes(oracle, world, cost, loss, n, mixed):
    """the grouped path with 2, 8 and 16 groups of four keyframes (n = 64: the scans of the world twice, the largest problem accepted);
    755 blocks with nine scans: past the P2L capacity, inside P2P's"""
    imgs, gt = world
    idx = [i % 32 for i in range(n - 1)] + [32]
    poses = gt[idx].copy()
    poses[-1] += [0.11, -0.06, 0.004]
    kw = dict(BASE, cost=cost, loss=loss, weight_opt=4)
    ctx, dsc, _, _ = _per_call(oracle, kw, imgs[idx], poses, 0.3, 1, 2, PRIOR if n == 9 else None, want_path=2, want_mixed=mixed, want_nsrc=False,
                               want_nk=True)
    if n == 64:
        with pytest.raises(capi.CfearError, match="rc=-3"):  # CFEAR_ERR_UNSUPPORTED
            ctx.get_surface(dsc + [dsc[0]], np.vstack([poses, poses[:1]]), 0.3, 1)
        assert np.all(np.isfinite(ctx.get_surface(dsc, poses, 0.5, 1)))  # and the context stays usable
    ctx.close()


@pytest.mark.parametrize("rule,pert", [(1, "nn_tie_high"), (2, "nn_tie_flann")])
def test_tie_rules_take_the_general_path(oracle, canyon, canyon_poses, rule, pert):
    """cfear_tune NN_TIE_RULE 1 / 2: the pair-by-pair general path (3) with the rule's search, against the restatement under the
    oracle's perturbation of the same name (Scan.closest honours it); mixed blocks as well (1028 > 710)"""
    kw = dict(BASE, cost=1, loss=2, weight_opt=4)
    n, poses = 4, canyon_poses[1][:4]
    oracle.set_perturbation([pert])
    try:
        ctx, dsc, got, exp = _per_call(oracle, kw, canyon[:n], poses, 0.07, 1, 2, None, tie=rule, want_path=3, want_mixed=True)
    finally:
        oracle.set_perturbation(0)
    p = oracle.default_params(**kw)
    base = surface_ref.surface_grid(oracle, [_oscan(oracle, p, img) for img in canyon[:n]], poses, p, 2, 0.07, 1)
    m = ~np.isnan(exp)
    # (these scans have cells with equal float means - test_tie_rule_gpu.py asserts it - and the rules pick differently among them)
    assert np.any(exp[m] != base[m]), "the tie rule changes no match of these scans: the comparison above says nothing about the rule"
    ctx0 = capi.Context(capi.default_params(**kw), A, R)
    _close(ctx0.get_surface([_dscan(ctx0, img) for img in canyon[:n]], poses, 0.07, 1), base, 1e-9)  # the production rule next to it
    assert not np.array_equal(got[m], base[m])
    ctx.close(); ctx0.close()


def _dense_clouds(n, side=50, seed=3):
    """n views of one synthetic yard of side^2 short wall pieces, one per 3 m voxel: about side^2 cells per scan"""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(side) - side / 2, np.arange(side) - side / 2)
    ctr = np.column_stack([gx.ravel(), gy.ravel()]) * 3.0 + 1.5
    ang = rng.uniform(0, np.pi, len(ctr))
    t = np.linspace(-0.9, 0.9, 7)
    W = (ctr[:, None, :] + t[None, :, None] * np.stack([np.cos(ang), np.sin(ang)], 1)[:, None, :]).reshape(-1, 2)
    poses = np.column_stack([0.05 * np.arange(n), 0.02 * np.arange(n), 0.0005 * np.arange(n)])
    out = []
    for x, y, th in poses:
        c, s = np.cos(th), np.sin(th)
        P = (W - [x, y]) @ np.array([[c, -s], [s, c]]) + rng.normal(0, 0.03, W.shape)  # R(-th) (W - t) + noise
        out.append(np.column_stack([P, rng.integers(61, 256, len(P))]).astype(np.float32))
    return out, poses


def test_general_path_without_a_tie_rule(oracle):
    """keyframes x source cells > 65535 (the grouped path numbers residual blocks in 16-bit fields): 32 keyframes x about 2500 cells,
    clouds uploaded as they are (cloud_upload, as test_feature_fuzz_gpu.py does)"""
    kw = dict(BASE, cost=1, loss=2, weight_opt=4)
    p = oracle.default_params(**kw)
    clouds, poses = _dense_clouds(33)
    poses = poses.copy()
    poses[-1] += [0.04, -0.03, 0.001]
    ctx = capi.Context(capi.default_params(**kw), A, R)
    osc = [oracle.Scan(c, p) for c in clouds]
    dsc = [ctx.scan_create(ctx.cloud_upload(c)) for c in clouds]
    nsrc, nk = len(osc[-1].cells()), len(osc) - 1
    assert dsc[-1].size == nsrc and nk * nsrc > 65535, (nk, nsrc)
    exp, nblk = surface_ref.surface_grid(oracle, osc, poses, p, 2, 0.07, 1, PRIOR, with_blocks=True)
    S = ctx.register(dsc, poses)[3]
    _say("per call P2L dense clouds: blocks %d (LDS capacity %d), source cells %d, keyframes %d, keyframes x cells %d, assoc_path %d"
         % (nblk, LDS_CAP[1], nsrc, nk, nk * nsrc, S.assoc_path))
    assert S.assoc_path == 3 and nblk > LDS_CAP[1]
    _close(ctx.get_surface(dsc, poses, 0.07, 1, prior_cov6=PRIOR), exp, 1e-9)
    ctx.close()


def test_cell_at_estimate_is_get_cost_on_dense_problems(oracle, canyon, canyon_poses):
    """test_surface_gpu.py's invariant past the LDS capacity: width 0, one cell at the round-tripped estimate = GetCost's score"""
    for cost in (0, 1, 2):
        kw = dict(BASE, cost=cost, loss=2, weight_opt=4)
        p = oracle.default_params(**kw)
        ctx = capi.Context(capi.default_params(**kw), A, R)
        dsc = [_dscan(ctx, img) for img in canyon[:5]]
        poses = canyon_poses[cost][:5].copy()
        poses[-1] += [0.1, 0.05, 2 * math.pi]  # (a yaw beyond pi: the round trip wraps it to the same rotation, the matches stay)
        for itr in (1, 2):
            nblk = len(surface_ref.build_blocks([_oscan(oracle, p, img) for img in canyon[:5]], poses, p, itr)[1])
            assert nblk > LDS_CAP[cost], (cost, itr, nblk)
            s = ctx.get_surface(dsc, poses, 0.1, 0, itr=itr)
            score, _ = ctx.get_cost(dsc, poses, itr=itr)
            _say("width 0 %s itr %d: blocks %d (LDS capacity %d)" % (COST_NAME[cost], itr, nblk, LDS_CAP[cost]))
            assert s.shape == (1, 1) and abs(s[0, 0] - score) <= 1e-12 * abs(score), (cost, itr, s[0, 0], score)
        ctx.close()


# ---- C: the two-pixel tiles ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cost,loss,dense", [(2, 2, True), (0, 5, True), (1, 1, False)])
def test_two_pixel_tiles_per_call(oracle, world, canyon, canyon_poses, cost, loss, dense):
    """365 x 365 pixels: 521 tiles of 256, surface_eval_kernel<COST, 2> on a single problem. The last tile holds 105 pixels (its second
    half lies past the end); 365 is odd, so a thread's two pixels sit in different rows now and then"""
    kw = dict(BASE, cost=cost, loss=loss, weight_opt=4)
    if dense:
        imgs, poses = canyon[:5], canyon_poses[cost][:5]
    else:
        imgs, poses = world[0][:3], world[1][:3].copy()
        poses[-1] += [0.11, -0.06, 0.004]
    tiles, two = _tiles(365, 1)
    assert two and tiles == 521 and 365 * 365 - 520 * 256 <= 128
    ctx, _, got, exp = _per_call(oracle, kw, imgs, poses, 0.011, 2, 2, PRIOR if cost == 2 else None, want_mixed=dense, want_nsrc=dense)
    assert exp.shape == (365, 365)
    ctx.close()


def _streams(imgs, B):
    """B different streams of one drive: the sweeps rotated by q x 13 azimuths, every other one reversed - B different pose histories,
    so that the grids' visited counts differ from sequence to sequence"""
    return [np.ascontiguousarray(np.roll(imgs[:, ::-1] if q & 1 else imgs, 13 * q, axis=1)) for q in range(B)]


@pytest.fixture(scope="module")
def drive64():
    imgs, _ = synth.world_sequence(7, seed=41)
    return _streams(imgs, 64)




def _batched_against_per_call(ctx, odo, seq_scans, grids, every=1):
    """odo.surface at each grid against ctx.get_surface on the recorded poses: 1e-12, then bit for bit. seq_scans(q, n) -> the n device scans of sequence
    q's last registration. -> {(res, width): set of (nx == pixels, ny == pixels)}"""
    seen = {}
    for res, width in grids:
        s, n_used, itr_used, poses_used = odo.surface(res, width, details=True)
        s = s.cpu().numpy()
        pixels = s.shape[1]
        tiles, two = _tiles(pixels, odo.B)
        same = True
        for q in range(0, odo.B, every):
            n = int(n_used[q])
            assert n >= 2, (q, n)
            exp = ctx.get_surface(seq_scans(q, n), poses_used[q, :n], res, width, itr=int(itr_used[q]))
            assert not _tiles(pixels, 1)[1]  # the per-call side runs one pixel per thread
            _close(s[q], exp, 1e-12)
            same = same and np.array_equal(s[q], exp, equal_nan=True)
            _, nx, ny = capi.surface_dims(res, width, poses_used[q, n - 1, 0], poses_used[q, n - 1, 1])
            assert np.all(np.isnan(s[q][nx:])) and np.all(np.isnan(s[q][:, ny:])) and np.all(np.isfinite(s[q][:nx, :ny]))
            seen.setdefault((res, width), set()).add((nx == pixels, ny == pixels))
        _say("batched %d sequences, grid %d^2 (res %g width %d): two-pixel tiles %d (%s), bit-identical to the one-pixel launch: %s, visited (x full, y full): %s"
             % (odo.B, pixels, res, width, tiles, "PPT 2" if two else "PPT 1", same, sorted(seen[(res, width)])))
        assert two
        # surface_dev.h: "a pixel's value depends on nothing but its own coordinates and the blocks, whatever the launch shape" - measured on
        # an MI355X: identical in all eight grids of this file (3 x 64 sequences at 81^2, 512 sequences at 8^2, 9^2, 12^2, 17^2, 21^2)
        assert same, "the two-pixel launch and the one-pixel launch differ in some bit"
    return seen


KWC = dict(BASE, cost=1, loss=1, weight_opt=4, use_keyframe=0, compensate=0, submap_scan_size=3)


def test_two_pixel_tiles_batched(drive64):
    """64 sequences at (0.05, 2): 81 x 81, 26 x 64 tiles of 256 pixels - the two-pixel instantiation - against cfear_get_surface on the
    same scans and recorded poses, which runs one pixel per thread (52 tiles)"""
    B, T = 64, 7
    ctx = capi.Context(capi.default_params(**KWC), A, R)
    odo = ctx.odometry(B)
    odo.set_surface_recording(True)
    scans = {}
    seen = set()
    for t in range(T):
        odo.step_host(np.stack([drive64[q][t] for q in range(B)]))
        for q in range(B):
            scans[(q, t)] = _dscan(ctx, drive64[q][t])
        if t in (1, 4, T - 1):
            got = _batched_against_per_call(ctx, odo, lambda q, n: [scans[(q, t - n + 1 + i)] for i in range(n)], [(0.05, 2)])
            seen |= got[(0.05, 2)]
    # 81 and 80 values visited occur along x and along y (all four combinations: test_two_pixel_tile_edges)
    assert {a for a, _ in seen} == {True, False} and {b for _, b in seen} == {True, False}, seen
    odo.release(); ctx.close()


def test_two_pixel_tile_edges(drive64):
    """512 sequences, so that even a grid of one tile runs two pixels per thread: 8 x 8 and 9 x 9 (fewer than 128 pixels: every second
    pixel is past the end), 17 x 17 (289 = 256 + 33: the last tile's second half lies entirely past the end), 21 x 21 (441 = 256 + 185:
    partly), 12 x 12 (144: the first tile's second half holds 16 pixels)"""
    B, T = 512, 3
    ctx = capi.Context(capi.default_params(**KWC), A, R)
    odo = ctx.odometry(B)
    odo.set_surface_recording(True)
    for t in range(T):
        odo.step_host(np.stack([drive64[q % 64][t] for q in range(B)]))
    scans = {(q, t): _dscan(ctx, drive64[q][t]) for q in range(64) for t in range(T)}
    grids = [(0.3, 1), (0.25, 1), (0.125, 1), (0.1, 1), (0.19, 1)]
    assert [capi.surface_dims(r, w)[0] for r, w in grids] == [8, 9, 17, 21, 12]
    assert 8 * 8 < 128 and 9 * 9 < 128 and 0 < 17 * 17 - 256 <= 128 and 21 * 21 - 256 > 128 and 128 < 12 * 12 < 256
    seen = _batched_against_per_call(ctx, odo, lambda q, n: [scans[(q % 64, T - n + i)] for i in range(n)], grids)
    both = set().union(*seen.values())
    assert both == {(True, True), (True, False), (False, True), (False, False)}, seen  # pixels - 1 in x only, in y only, in both, in neither
    odo.release(); ctx.close()


# ---- D: the batched route in the configurations the registration supports --------------------------------------------------------
def _run_config(oracle, kw, streams, T, check_at, hip_kw=None, odo_kw=None, tune=(), pert=None, per_call_cloud=None, oracle_cloud=None,
                grid=(0.05, 1), ref_grid=(0.25, 1), ref_seqs=(0,), expect_n=None):
    """streams[q][t]: the sweeps. Two objects, one recording: poses, covariances and summaries bit-identical at every sweep; at the
    sweeps of check_at every sequence's surface against cfear_get_surface on what was recorded (1e-12), at the last one ref_seqs
    against the restatement (1e-9). The scans a record names are found by their poses: a keyframe's pose is the pose its sweep was
    registered at. -> per checked sweep and sequence, the sweeps the record used"""
    B = len(streams)
    ctxs, odos = [], []
    for rec in (True, False):
        ctx = capi.Context(capi.default_params(**(hip_kw or kw)), A, R)
        for k, v in tune:
            ctx.tune(k, v)
        odo = ctx.odometry(B, **(odo_kw or {}))
        if rec:
            odo.set_surface_recording(True)
        ctxs.append(ctx); odos.append(odo)
    ctx, odo = ctxs[0], odos[0]
    p = oracle.default_params(**kw)
    dcache, ocache = {}, {}

    def dscan(q, t):
        if (q, t) not in dcache:
            dcache[(q, t)] = ctx.scan_create(per_call_cloud(ctx, streams[q][t])) if per_call_cloud else _dscan(ctx, streams[q][t])
        return dcache[(q, t)]

    def oscan(q, t):
        if (q, t) not in ocache:
            ocache[(q, t)] = oracle.Scan(oracle_cloud(streams[q][t]), p) if oracle_cloud else _oscan(oracle, p, streams[q][t])
        return ocache[(q, t)]

    hist, used = [], {}
    for t in range(T):
        batch = np.ascontiguousarray(np.stack([streams[q][t] for q in range(B)]))
        for o in odos:
            o.step_host(batch)
        assert np.array_equal(odos[0].poses(), odos[1].poses()), t
        assert np.array_equal(odos[0].covariances(), odos[1].covariances()), t
        for q in range(B):
            assert bytes(odos[0].summary(q)[0]) == bytes(odos[1].summary(q)[0]), (t, q)
        hist.append(odo.poses().copy())
        if t not in check_at:
            continue
        s, n_used, itr_used, poses_used = odo.surface(*grid, details=True)
        s = s.cpu().numpy()
        if t == T - 1:
            s2 = odo.surface(*ref_grid).cpu().numpy()
        for q in range(B):
            n = int(n_used[q])
            assert n >= 2 and (expect_n is None or n == expect_n(t)), (t, q, n)
            assert np.all(np.abs(poses_used[q, n - 1] - hist[t][q, :3]) <= 1e-12), (t, q)  # the registered pose of this sweep (before its round trip)
            sweeps = []
            for i in range(n - 1):  # the sweep a keyframe came from: the one registered at its pose (the first of them, during a stop)
                d = [float(np.max(np.abs(hist[u][q, :3] - poses_used[q, i]))) for u in range(t)]
                u = int(np.argmin(d))
                assert d[u] <= 1e-12, (t, q, i, d[u])
                sweeps.append(u)
            assert sweeps == sorted(set(sweeps)), (t, q, sweeps)
            sweeps.append(t)
            used[(t, q)] = sweeps
            dsc = [dscan(q, u) for u in sweeps]
            _close(s[q], ctx.get_surface(dsc, poses_used[q, :n], grid[0], grid[1], itr=int(itr_used[q])), 1e-12)
            if t == T - 1 and q in ref_seqs:
                if pert:
                    oracle.set_perturbation([pert])
                try:
                    exp, nblk = surface_ref.surface_grid(oracle, [oscan(q, u) for u in sweeps], poses_used[q, :n], p, int(itr_used[q]), ref_grid[0],
                                                         ref_grid[1], with_blocks=True)
                finally:
                    if pert:
                        oracle.set_perturbation(0)
                S = odo.summary(q)[0]
                _say("batched %s sweep %d sequence %d: scans %d (sweeps %s), blocks %d (LDS capacity %d), source cells %d, assoc_path %d"
                     % (COST_NAME[kw["cost"]], t, q, n, sweeps, nblk, LDS_CAP[kw["cost"]], len(oscan(q, t).cells()), S.assoc_path))
                _close(s2[q], exp, 1e-9)
                used[("blocks", q)] = nblk
                used[("path", q)] = int(S.assoc_path)
    for o, c in zip(odos, ctxs):
        o.release(); c.close()
    return used


@pytest.fixture(scope="module")
def drive4():
    imgs, _ = synth.world_sequence(16, seed=41)
    return _streams(imgs, 4)


@pytest.mark.parametrize("cost", [2, 0])
def test_batched_p2d_and_p2p(oracle, drive4, cost):
    kw = dict(KWC, cost=cost, loss=2)
    T = 8
    used = _run_config(oracle, kw, drive4, T, (1, 4, T - 1), ref_seqs=(0, 3), expect_n=lambda t: min(t + 1, 4))
    assert used[(T - 1, 2)] == [T - 4, T - 3, T - 2, T - 1]  # every sweep a keyframe
    assert used[("path", 0)] == 1


@pytest.mark.parametrize("cost", [1, 2])
def test_batched_keyframes_through_a_stop(oracle, drive4, cost):
    """use_keyframe = 1 on a drive that stops twice: sweeps that add no keyframe, and records that go on naming the keyframes used -
    not the last sweeps. During the stop the same sweep is registered against itself among the keyframes (every cell matches)"""
    order = [0, 1, 2, 3, 3, 3, 3, 4, 5, 6, 6, 6, 7, 8]
    streams = [s[order] for s in drive4]
    kw = dict(KWC, cost=cost, loss=2, use_keyframe=1)
    T = len(order)
    check_at = (2, 5, 6, 8, 11, T - 1)
    used = _run_config(oracle, kw, streams, T, check_at, ref_seqs=(0, 1))
    # a checked sweep whose newest keyframe is older than the sweep before it: that sweep added none
    stale = [(t, q) for t in check_at for q in range(4) if used[(t, q)][-2] < t - 1]
    _say("use_keyframe 1 %s: records at (sweep, sequence) whose previous sweep added no keyframe: %s" % (COST_NAME[cost], stale))
    assert stale


def test_batched_cacfar(oracle, street):
    """CA-CFAR as the stage-1 filter: the per-call scans come from cfear_filter_cfar, the restatement's from the oracle's"""
    kw = dict(KWC, cost=2, loss=2)
    hip_kw = dict(kw, filter_type=capi.FILTER_CACFAR, cfar_window_size=CFAR["window_size"], cfar_nb_guard_cells=CFAR["nb_guard_cells"],
                  cfar_false_alarm_rate=CFAR["false_alarm_rate"])
    streams = [street, np.ascontiguousarray(street[:, ::-1])]
    _run_config(oracle, kw, streams, 6, (1, 3, 5), hip_kw=hip_kw, ref_seqs=(0, 1),
                per_call_cloud=lambda ctx, img: ctx.filter_cfar(img, **CFAR),
                oracle_cloud=lambda img: oracle.cfar(img, float(RR), float(kw["z_min"]), 2.5, **CFAR))


@pytest.mark.parametrize("large_kernel,cost", [(1, 0), (2, 2)])
def test_batched_large_submap(oracle, canyon, large_kernel, cost):
    """submap_scan_size = 10 with both large-submap kernels, in the canyon: eleven scans, three groups of keyframes, thousands of
    blocks (mixed LDS / memory on the batched route)"""
    kw = dict(KWC, cost=cost, loss=2, submap_scan_size=10)
    streams = [canyon, np.ascontiguousarray(canyon[:, ::-1])]
    T = 12
    used = _run_config(oracle, kw, streams, T, (5, T - 1), odo_kw=dict(large_kernel=large_kernel), ref_seqs=(0, 1),
                       expect_n=lambda t: min(t + 1, 11))
    assert len(used[(T - 1, 0)]) == 11 and used[("path", 0)] == 2 and used[("blocks", 0)] > LDS_CAP[cost]


@pytest.mark.parametrize("cost", [2, 1, 0])
def test_batched_canyon_mixed_blocks(oracle, canyon, cost):
    kw = dict(KWC, cost=cost, loss=2, submap_scan_size=4)
    streams = [canyon, np.ascontiguousarray(canyon[:, ::-1])]
    T = 6
    used = _run_config(oracle, kw, streams, T, (2, T - 1), ref_seqs=(0, 1), expect_n=lambda t: min(t + 1, 5))
    assert used[("blocks", 0)] > LDS_CAP[cost] and used[("blocks", 1)] > LDS_CAP[cost] and used[("path", 0)] == 2


def test_batched_overlapping_streams(oracle, drive4):
    kw = dict(KWC, cost=0, loss=2)
    _run_config(oracle, kw, drive4, 6, (1, 3, 5), odo_kw=dict(overlap=2), ref_seqs=(1, 2), expect_n=lambda t: min(t + 1, 4))


def test_batched_flann_tie_rule(oracle, canyon):
    """NN_TIE_RULE = 2 on the batched step: the build stage follows the rule (general path), as cfear_get_surface under the same rule
    and the restatement under the oracle's nn_tie_flann do"""
    kw = dict(KWC, cost=1, loss=2)
    streams = [canyon, np.ascontiguousarray(canyon[:, ::-1])]
    used = _run_config(oracle, kw, streams, 5, (1, 4), tune=((capi.TUNE_NN_TIE_RULE, 2),), pert="nn_tie_flann", ref_seqs=(0, 1))
    assert used[("path", 0)] == 3


def test_surface_with_cost_sampling_on_and_recording_off(drive4):
    """cfear_odometry_surface needs the record, not the switch: with the cost-sampling covariance on (which keeps the same record) and
    the surface recording off it gives the surfaces of a twin with the recording on, bit for bit, and leaves cov_samples and the
    covariances alone"""
    B, T = 4, 5
    ctxs = [capi.Context(capi.default_params(**dict(KWC, cost=2, loss=2)), A, R) for _ in range(2)]
    odos = [c.odometry(B) for c in ctxs]
    odos[0].set_cov_sampling(True, 0.4, 0.0043625, 3, 4.0)
    odos[1].set_cov_sampling(True, 0.4, 0.0043625, 3, 4.0)
    odos[1].set_surface_recording(True)
    for t in range(T):
        batch = np.ascontiguousarray(np.stack([drive4[q][t] for q in range(B)]))
        for o in odos:
            o.step_host(batch)
        if t == 0:
            continue
        cov0, smp0 = odos[0].covariances(), [odos[0].cov_samples(q) for q in range(B)]
        a = odos[0].surface(0.05, 1, details=True)
        b = odos[1].surface(0.05, 1, details=True)
        assert np.array_equal(a[0].cpu().numpy(), b[0].cpu().numpy(), equal_nan=True) and bool(a[0].isfinite().any()), t
        for x, y in zip(a[1:], b[1:]):
            assert np.array_equal(x, y), t
        assert np.all(a[1] == min(t + 1, 4))
        assert np.array_equal(odos[0].covariances(), cov0) and np.array_equal(cov0, odos[1].covariances()), t
        for q in range(B):
            c, ok = odos[0].cov_samples(q)
            assert np.array_equal(c, smp0[q][0]) and ok == smp0[q][1], (t, q)
            c1, ok1 = odos[1].cov_samples(q)
            assert np.array_equal(c, c1) and ok == ok1, (t, q)
        assert np.array_equal(odos[0].poses(), odos[1].poses())
    for o, c in zip(odos, ctxs):
        o.release(); c.close()


@pytest.mark.parametrize("sampling", [False, True])
def test_surface_after_a_replay(drive4, sampling):
    """The replay routes do not record (include/cfear_hip.h): after replay_host the surfaces are all NaN with n_used = 0 - also with
    the cost sampling on, whose stage does write the record during a replay (surf_ready says the record is not a step's). One
    further step_host registers the new sweep against the keyframes the replay left (the object is not reset), records it, and the
    surfaces are valid: 'no step since the last reset / replay' of the header, not 'first sweep'. They equal cfear_get_surface on
    the sweeps the record names."""
    B, T = 4, 5
    ctx = capi.Context(capi.default_params(**dict(KWC, cost=1, loss=2)), A, R)
    odo = ctx.odometry(B)
    odo.set_surface_recording(True)
    if sampling:
        odo.set_cov_sampling(True, 0.4, 0.0043625, 3, 4.0)
    odo.step_host(np.ascontiguousarray(np.stack([drive4[q][0] for q in range(B)])))
    odo.step_host(np.ascontiguousarray(np.stack([drive4[q][1] for q in range(B)])))
    assert bool(odo.surface(0.25, 1).isfinite().any())
    odo.reset()
    frames = np.ascontiguousarray(np.stack([np.stack([drive4[q][t] for q in range(B)]) for t in range(T)]))
    rec = odo.replay_host(frames)
    s, n_used, itr_used, poses_used = odo.surface(0.25, 1, details=True)
    assert bool(s.isnan().all()) and np.all(n_used == 0) and np.all(itr_used == 0) and np.all(poses_used == 0)
    odo.step_host(np.ascontiguousarray(np.stack([drive4[q][T] for q in range(B)])))
    s, n_used, itr_used, poses_used = odo.surface(0.25, 1, details=True)
    s = s.cpu().numpy()
    assert np.all(n_used == 4)
    assert np.all(np.abs(poses_used[:, 3] - odo.poses()[:, :3]) <= 1e-12)
    assert np.all(np.abs(poses_used[:, 2] - rec[-1]["pose"][:, :3]) <= 1e-12)  # the newest keyframe: the replay's last sweep
    for q in range(B):
        dsc = [_dscan(ctx, drive4[q][u]) for u in range(T - 3, T + 1)]
        _close(s[q], ctx.get_surface(dsc, poses_used[q, :4], 0.25, 1, itr=int(itr_used[q])), 1e-12)
        assert np.all(np.isfinite(s[q][:8, :8]))
    odo.release(); ctx.close()


def test_surface_reports_the_capacity_error(canyon):
    """max_cells too small for the canyon: surface() fails as the other readers do (CFEAR_ERR_CAPACITY with the limit in the message),
    and after a reset the object works again"""
    B = 2
    streams = [canyon, np.ascontiguousarray(canyon[:, ::-1])]
    ctx = capi.Context(capi.default_params(**dict(KWC, cost=1, loss=2)), A, R)
    odo = ctx.odometry(B, max_cells=200)
    odo.set_surface_recording(True)
    for t in range(3):
        odo.step_host(np.ascontiguousarray(np.stack([s[t] for s in streams])))
    with pytest.raises(capi.CfearError, match=r"rc=-6.*more than 200 oriented surface points"):
        odo.surface(0.25, 1)
    with pytest.raises(capi.CfearError, match="rc=-6"):
        odo.poses()
    odo.reset()
    assert bool(odo.surface(0.25, 1).isnan().all())
    odo.release()
    odo = ctx.odometry(B)  # (sized for every filtered point again) the context is as usable as before
    odo.set_surface_recording(True)
    for t in range(2):
        odo.step_host(np.ascontiguousarray(np.stack([s[t] for s in streams])))
    s = odo.surface(0.25, 1)
    assert bool(s.isfinite().any()) and not bool(s.isnan().all())
    odo.release(); ctx.close()
