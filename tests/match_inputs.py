"""Inputs whose last registration has an exact number of residual blocks (test_match_inputs_cpu.py, test_match_capacity_gpu.py): the
count M decides where a registration kernel keeps its compacted matches (registration_dev.h: all in the LDS match array up to
match_lds_cap(cost), the rest in memory beyond) and how many trips the evaluation's pair loop makes, so the tests want M at a
capacity and one to either side - not "somewhere above".

The worlds are small, well separated clusters: 8 points on a segment of 0.8 m, centres on a grid of 7.5 m, integer intensities
80 .. 200, seen from poses that advance by 2 m per sweep (every sweep a keyframe). Every sweep has its own point jitter: without it
the optimum has cost zero and a residual block that went missing would not show. A cluster is one or two oriented surface points
(its points can straddle a voxel of the sensor-anchored grid), so the count is steered with the oracle's fuser in the loop: first the
number of clusters, then clusters that exist only from some sweep on, which match in the last j keyframes only - down to j = 1, the
step of one or two blocks. Deterministic from the seed, memoised per request. Plain numpy and the oracle; no GPU.

Two producers: clouds (steer_cloud: the batched step from clouds and the per-call entries) and polar sweeps of the same kind of
world (steer_polar: the replay takes only images). In the polar worlds the segments point away from the sensor's path, so that
the eight points fall into eight range bins of one or two azimuths."""
import math

import numpy as np

from oracle import binding as oracle

GRID = 7.5          # m between cluster centres
PTS = 8             # points per cluster
HALF = 0.4          # half length of a cluster's segment
STEP = 2.0          # m per sweep along x (> min_keyframe_dist: every sweep becomes a keyframe)
MAX_SLOTS = 1000    # clusters a world can have: clouds of at most 8000 points
PAD0 = 700          # first slot of the clusters that only pad the source scan (seen by the last sweep alone: cells without a match)
# polar sweeps: 800 azimuths x k = 6 (4800 slots: the compact feature path, the cloud pass's per-bearing table), 0.0595 m bins out to
# 80 m. Segments at 45 degrees to the line of sight: a cluster's eight points fall into eight range bins of two or three azimuths
POLAR_A, POLAR_R, POLAR_RR, POLAR_K = 800, 1344, np.float32(0.0595238), 6

BASE = dict(res=3.0, weight_intensity=1, weight_opt=4, regularization=0.1, covar_scale=1.0, compensate=0, use_keyframe=1,
            z_min=60.0, min_distance=2.5)
# the three ways evaluate_partial_t evaluates a loss: Huber inline, Cauchy inline, any other through loss_eval - here Tukey. Tukey's
# derivative is zero beyond its limit, and a fuser's first registration starts a whole step (2 m; whitened by P2D's covariance up to
# 6.3) from the answer, where a limit of 0.1 leaves no gradient at all: its rows run with a limit of 8 (rho' = (1 - s / 64)^2)
HUBER, CAUCHY, TUKEY = 1, 2, 5
LOSS_LIMIT = {HUBER: 0.1, CAUCHY: 0.1, TUKEY: 8.0}
_MEMO = {}


def params_kw(cost, loss, submap, polar=False):
    kw = dict(BASE, cost=cost, loss=loss, loss_limit=LOSS_LIMIT[loss], submap_scan_size=submap)
    if polar:
        kw.update(range_res=POLAR_RR, k_strongest=POLAR_K)
    return kw


def _slots(polar, T):
    """cluster centres, nearest to the middle of the path first: a world of n clusters is the first n of them. No centre within
    3.75 m of the path (the sensor never drives through a cluster)"""
    n, mid = 20, STEP * (T - 1) / 2
    gx, gy = np.meshgrid(np.arange(-n, n) * GRID + 1.0, np.arange(-n, n) * GRID + GRID / 2)
    c = np.column_stack([gx.ravel(), gy.ravel()])
    d = np.hypot(c[:, 0] - mid, c[:, 1])
    if polar:  # inside the image from every pose of the path
        far = float(POLAR_RR) * POLAR_R - mid - 2.0
        c, d = c[d < far], d[d < far]
    return c[np.argsort(d, kind="stable")][:MAX_SLOTS], mid


class World:
    """the clusters and every sweep's jitter, drawn once from the seed: slot s of sweep t has the same points whatever else is in the world"""

    def __init__(self, T, sigma, seed, polar=False):
        rng = np.random.default_rng([seed, T, int(polar)])
        self.T, self.polar = T, polar
        self.ctr, mid = _slots(polar, T)
        S = len(self.ctr)
        if polar:
            ang = np.arctan2(self.ctr[:, 1], self.ctr[:, 0] - mid) + rng.choice([-1.0, 1.0], S) * (np.pi / 4 + rng.uniform(-0.2, 0.2, S))
        else:
            ang = rng.uniform(0, np.pi, S)
        t = np.linspace(-HALF, HALF, PTS)
        self.pts = self.ctr[:, None, :] + t[None, :, None] * np.stack([np.cos(ang), np.sin(ang)], 1)[:, None, :]  # [S, PTS, 2]
        self.inten = rng.integers(80, 201, (S, PTS)).astype(np.float32)
        self.jit = rng.normal(0.0, sigma, (T, S, PTS, 2))
        self.poses = np.column_stack([STEP * np.arange(T), 0.07 * np.arange(T), 0.004 * np.arange(T)])

    def cloud(self, t, n, extras):
        """sweep t: the first n clusters and those of extras = [(slot, j)] that exist by then (j: the keyframes of the last sweep that saw
        the cluster: it exists from sweep T - 1 - j on), in the sensor's frame -> float32 [points, 3]"""
        idx = list(range(n)) + [s for s, j in extras if t >= self.T - 1 - j]
        x, y, th = self.poses[t]
        c, s = math.cos(th), math.sin(th)
        W = self.pts[idx] + self.jit[t, idx]
        P = (W - [x, y]).reshape(-1, 2) @ np.array([[c, -s], [s, c]])  # R(-th) (W - t)
        return np.column_stack([P, self.inten[idx].reshape(-1)]).astype(np.float32)

    def clouds(self, n, extras):
        return [self.cloud(t, n, extras) for t in range(self.T)]


def render_polar(cloud, A=POLAR_A, R=POLAR_R, range_res=POLAR_RR):
    """a cloud as a polar sweep: a point goes to pixel (round(theta A / 2 pi), round(rho / range_res)) with its intensity"""
    img = np.zeros((A, R), dtype=np.uint8)
    th = np.mod(np.arctan2(cloud[:, 1], cloud[:, 0]), 2 * np.pi)
    a = np.mod(np.rint(th * A / (2 * np.pi)).astype(np.int64), A)
    r = np.rint(np.hypot(cloud[:, 0], cloud[:, 1]) / float(range_res)).astype(np.int64)
    ok = r < R
    assert ok.all(), "the world leaves the image"
    np.maximum.at(img, (a[ok], r[ok]), cloud[ok, 2].astype(np.uint8))
    return img


def copy_summary(S):
    return oracle.RegSummary.from_buffer_copy(bytes(memoryview(S)))


def run_oracle(kw, sweeps, polar=False):
    """the oracle's fuser over the sweeps -> per sweep (pose, summary, keyframes after the sweep, cells of the sweep, 6 x 6 covariance)"""
    fu = oracle.Fuser(oracle.default_params(**kw))
    out = []
    for s in sweeps:
        pose = fu.process_polar(s) if polar else fu.process_cloud(s)
        out.append((pose.copy(), copy_summary(fu.last_summary()), int(fu.num_keyframes), len(fu.last_cells()), fu.last_cov().copy()))
    return out


class Case:
    """sweeps: the T clouds (or polar images) of one sequence; ref: run_oracle's result on them; blocks: of the last registration"""

    def __init__(self, kw, sweeps, ref, polar, n, extras, seed):
        self.kw, self.sweeps, self.ref, self.polar, self.n, self.extras, self.seed = kw, sweeps, ref, polar, n, extras, seed
        self.blocks = int(ref[-1][1].num_residual_blocks)
        self.cells = ref[-1][3]
        self.keyframes = ref[-1][2]


def _search(world, kw, target, pad, polar):
    """the number of clusters n and the extras that give `target` residual blocks in the last registration, or None"""
    K, T = kw["submap_scan_size"], world.T
    pads = [(PAD0 + i, 0) for i in range(pad)]
    runs = [0]

    def sweeps(n, extras):
        cl = world.clouds(n, pads + extras)
        return [render_polar(c) for c in cl] if polar else cl

    def count(n, extras):
        runs[0] += 1
        return int(run_oracle(kw, sweeps(n, extras), polar)[-1][1].num_residual_blocks)

    limit = PAD0 if pad else len(world.ctr) - 40
    n = max(2, min(limit, int(target / (1.3 * K))))
    b = count(n, [])
    for _ in range(8):  # the count is close to additive in the clusters: secant steps on blocks per cluster
        if 0 <= target - b < 2 * K:
            break
        step = int(round((target - b) * n / max(b, 1)))
        if step == 0:
            step = 1 if b < target else -1
        n = max(2, min(limit, n + step))
        b = count(n, [])
    while b > target and n > 2:
        n -= 1
        b = count(n, [])
    if b > target:
        return None
    extras, slot = [], n
    while b < target and slot < limit and runs[0] < 400:
        d = target - b
        for j in sorted({min(K, d), max(1, min(K, d) // 2), 1}, reverse=True):  # j = 1: a cluster one keyframe saw, the step of one (or two)
            b2 = count(n, extras + [(slot, j)])
            if b < b2 <= target:
                extras.append((slot, j))
                b = b2
                break
        slot += 1
    if b != target:
        return None
    return n, extras, sweeps(n, extras)


def final_build(case):
    """the blocks of the fuser's last association, restated: cfo_get_cost on Scans of the same clouds at the fuser's poses, the last one
    at the pose the last build started from, with the radius of that outer iteration -> (robustified residuals per block [M, nr], M)
    or None where the restatement does not reproduce the fuser's block count (the fuser's own scans are not reachable: polar sweeps
    go through the filter)"""
    kw, ref = case.kw, case.ref
    p = oracle.default_params(**kw)
    if case.polar:
        clouds = [oracle.cloud(oracle.filter_polar(s, int(kw["z_min"]), kw["k_strongest"]), kw["range_res"], kw["min_distance"]) for s in case.sweeps]
    else:
        clouds = case.sweeps
    T, K = len(clouds), case.keyframes
    S = ref[-1][1]
    no = min(int(S.outer_iterations), p.max_itr_association)
    poses = np.array([ref[t][0] for t in range(T - 1 - K, T)])
    if no >= 2:
        poses[-1] = list(S.outer_pose[no - 2])
    else:
        return None
    scans = [oracle.Scan(c, p) for c in clouds[T - 1 - K:]]
    got = oracle.get_cost(scans, poses, p, itr=no)
    if got is None:
        return None
    nr = 1 if kw["cost"] == 1 else 2
    res = got[1].reshape(-1, nr)
    if len(res) != case.blocks:
        return None
    return res, 0.5 * float(np.sum(res * res))


def seam_blocks(M, cap):
    return sorted({i for i in (cap - 2, cap - 1, cap, cap + 1, M - 1) if 0 <= i < M})


def seam_is_loud(case, cap):
    """the blocks cap - 2 .. cap + 1 and M - 1 each carry at least 1e-5 of the robustified cost (vacuous where final_build gives None)
    -> (True / False / None, the smallest share)"""
    fb = final_build(case)
    if fb is None:
        return None, None
    res, total = fb
    share = [0.5 * float(np.sum(res[i] ** 2)) / total for i in seam_blocks(case.blocks, cap)]
    return min(share) >= 1e-5, min(share)


def steer(cost, loss, submap, target, cap, pad=0, polar=False, sigma=0.04, seed=7):
    """a Case whose last registration has exactly `target` residual blocks at the oracle, with submap keyframes, and whose blocks at the
    seam of `cap` are not quiet. Tries the solution found for Huber first (the count rarely depends on the loss), then searches; a
    seam block that is too quiet, or a target the search misses, moves on to the next seed. Raises where eight seeds fail."""
    key = (cost, loss, submap, target, cap, pad, polar, sigma, seed)
    if key in _MEMO:
        return _MEMO[key]
    kw = params_kw(cost, loss, submap, polar)
    T = submap + 1
    case = None
    if loss != 1:
        first = steer(cost, 1, submap, target, cap, pad, polar, sigma, seed)
        ref = run_oracle(kw, first.sweeps, polar)
        cand = Case(kw, first.sweeps, ref, polar, first.n, first.extras, first.seed)
        if cand.blocks == target and seam_is_loud(cand, cap)[0] is not False:
            case = cand
    sd = seed
    while case is None:
        if sd >= seed + 8:
            raise AssertionError("no world of %d residual blocks for cost %d loss %d submap %d (polar %s) in eight seeds" % (target, cost, loss, submap, polar))
        world = _world(T, sigma, sd, polar)
        got = _search(world, kw, target, pad, polar)
        if got is not None:
            n, extras, sw = got
            cand = Case(kw, sw, run_oracle(kw, sw, polar), polar, n, extras, sd)
            assert cand.blocks == target
            if seam_is_loud(cand, cap)[0] is not False:
                case = cand
        sd += 1
    _MEMO[key] = case
    return case


def _world(T, sigma, seed, polar):
    key = ("world", T, sigma, seed, polar)
    if key not in _MEMO:
        _MEMO[key] = World(T, sigma, seed, polar)
    return _MEMO[key]


# ---- the named cases -------------------------------------------------------------------------------------------------------------------
# route -> (instantiation of match_caps.INSTANTIATIONS, submap_scan_size, polar sweeps?)
#   step4:  cfear_odometry_step_cloud_device, submap_scan_size 4: register_step_kernel (register_step.hip)
#   step64: the same entry, submap_scan_size 8, cfear_tune LARGE_SUBMAP_KERNEL 1: the 64-scan step kernel of pipeline.hip
#   large:  the same, LARGE_SUBMAP_KERNEL 2: register_step_large_kernel
#   replay: cfear_odometry_replay_host on rendered sweeps, submap_scan_size 11 (twelve sweeps): replay_chunk_kernel
#   call:   cfear_register / cfear_get_cost and the other per-call entries on scans of the clouds, four keyframes (percall.hip; their kernels are pipeline.hip's)
ROUTES = {"step4": ("register_step", 4, False), "step64": ("pipeline", 8, False), "large": ("register_step_large", 8, False),
          "replay": ("replay", 11, True), "call": ("pipeline", 4, False)}
LOSS_NAME = {HUBER: "huber", CAUCHY: "cauchy", TUKEY: "tukey"}
COSTS = (2, 1, 0)  # P2D, P2L, P2P
PAD_GROUPED = 80   # clusters only the last sweep sees: more than 256 source cells (the grouped association) at a block count 256 cells reach


class Named:
    def __init__(self, family, route, cost, loss, target, cap, nthr, pad=0):
        inst, submap, polar = ROUTES[route]
        self.family, self.route, self.inst, self.cost, self.loss, self.target, self.cap, self.nthr, self.pad = family, route, inst, cost, loss, target, cap, nthr, pad
        self.submap, self.polar = submap, polar
        self.name = "%s-%s-%s-%d-%s%s" % (family, route, {0: "P2P", 1: "P2L", 2: "P2D"}[cost], target, LOSS_NAME[loss], "-grouped" if pad else "")

    def steer(self):
        return steer(self.cost, self.loss, self.submap, self.target, self.cap, self.pad, self.polar)

    def want_path(self, cells):
        """association path 1 needs at most four keyframes and at most 256 source cells (one block of threads): otherwise the grouped path"""
        return 1 if self.submap <= 4 and cells <= 256 else 2


def named_cases(instantiations):
    """instantiations: match_caps.INSTANTIATIONS -> the cases of test_match_capacity_gpu.py, each a Named.
    Family A, the capacity seam: cap - 1 .. cap + 2 per instantiation and cost, under the three ways a loss is evaluated (P2D on the step
    kernel once with 256 cells at most and once with more: both association paths).
    Family B, the pair loop's trips: nthr - 1 .. nthr + 1 and 2 nthr - 1 .. 2 nthr + 1 blocks, all in LDS, per instantiation and cost;
    (the per-call entries too: they reach the evaluation through the run-time dispatch on cost and loss, not the instantiations per cost
    of the step kernels), and M - cap in {nthr, nthr + 1} once per instantiation (1 and 2 are family A's cap + 1 and cap + 2): the clamped prefetch indices of
    the memory half. nthr: the threads that evaluate, from the sources (256 everywhere but register_step_large.hip's 512: replay.hip's
    workgroup has 512 threads of which waves 4 .. 7 sit out the evaluation) - and for the replay also 512, its workgroup size."""
    out = []
    for route in ("step4", "step64", "large", "replay"):
        caps, nthr = instantiations[ROUTES[route][0]]
        for cost in COSTS:
            cap = caps[cost]
            for loss in (HUBER, CAUCHY, TUKEY):
                for target in (cap - 1, cap, cap + 1, cap + 2):
                    out.append(Named("A", route, cost, loss, target, cap, nthr))
                    if route == "step4" and cost == 2:
                        out.append(Named("A", route, cost, loss, target, cap, nthr, PAD_GROUPED))
            for n in ((nthr, 512) if route == "replay" else (nthr,)):
                for target in (n - 1, n, n + 1, 2 * n - 1, 2 * n, 2 * n + 1):
                    out.append(Named("B", route, cost, HUBER, target, cap, n))
        cost = {"step4": 1, "step64": 0, "large": 2, "replay": 2}[route]
        for n in ((nthr, 512) if route == "replay" else (nthr,)):
            for target in (caps[cost] + n, caps[cost] + n + 1):
                out.append(Named("B", route, cost, CAUCHY, target, caps[cost], n))
    caps, nthr = instantiations["pipeline"]
    for cost in COSTS:
        for target in (caps[cost] - 1, caps[cost], caps[cost] + 1):
            out.append(Named("A", "call", cost, HUBER, target, caps[cost], nthr))
        for target in (nthr - 1, nthr, nthr + 1, 2 * nthr - 1, 2 * nthr, 2 * nthr + 1):  # the per-call entries dispatch on cost and loss at run time
            out.append(Named("B", "call", cost, HUBER, target, caps[cost], nthr))
    seen = set()  # (the replay's 2 x 256 + 1 is its 512 + 1)
    return [c for c in out if not (c.name in seen or seen.add(c.name))]


def call_inputs(case):
    """the fuser's last registration as a per-call problem: the clouds of the keyframes and the last sweep, the keyframes' poses and the
    fuser's guess for the last one (T_prev Tmot: the motion of the sweep before, once more)"""
    T, K = len(case.sweeps), case.keyframes
    poses = np.array([case.ref[t][0] for t in range(T - 1 - K, T)])

    def aff(p):
        c, s = math.cos(p[2]), math.sin(p[2])
        return np.array([[c, -s, p[0]], [s, c, p[1]], [0, 0, 1.0]])
    a, b = aff(case.ref[T - 3][0]), aff(case.ref[T - 2][0])
    g = b @ (np.linalg.inv(a) @ b)
    poses[-1] = [g[0, 2], g[1, 2], math.atan2(g[1, 0], g[0, 0])]
    return case.sweeps[T - 1 - K:], poses
