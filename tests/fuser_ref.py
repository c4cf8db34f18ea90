"""OdometryKeyframeFuser::processFrame (odometrykeyframefuser.cpp:143-259, 470-494) written out in Python with the two switches the
oracle's own Fuser does not have - Parameters::soft_constraint and Parameters::use_guess (odometrykeyframefuser.h:94) - for the
fuser-option tests. Composed of the oracle's per-call pieces only: filter_polar / cloud / cfar, compensate, Scan, register,
register_soft, cov_by_sampling. The state machine (guess, FormatScans, sanity check, keyframe rule, AddToReference) follows
oracle/cfear_oracle.c's cfo_fuser_process_cloud line by line, in the same order of floating-point operations;
tests/test_fuser_options_cpu.py pins it to oracle.Fuser with both switches at their defaults.

    soft_constraint = 1: Register(scans_vek, T_vek, cov_vek, true) (:186) - the prior's covariance is cov_vek.back(), which FormatScans
                         leaves at Identity66 (:486-491); its centre is Tsrc.back() = Tguess, its weight sqrt(cells of the current scan)
                         (n_scan_normal.cpp:370-377, inside register_soft)
    use_guess = 0:       Tguess = T_prev (:167-168): the start of the registration, the fallback of the sanity check (:199) and the
                         centre of the prior. Compensation still uses Tmot (:146-150)."""
import math

import numpy as np


class Aff:
    """a 2-D affine map as the oracle keeps it: linear part row-major + translation"""
    __slots__ = ("l", "t")

    def __init__(self, l=(1.0, 0.0, 0.0, 1.0), t=(0.0, 0.0)):
        self.l, self.t = tuple(float(v) for v in l), tuple(float(v) for v in t)

    @staticmethod
    def from_xyt(x, y, th):  # vectorToAffine3d, registration.cpp:130-136
        c, s = math.cos(th), math.sin(th)
        return Aff((c, -s, s, c), (x, y))

    def mul(A, B):
        a, b = A.l, B.l
        return Aff((a[0] * b[0] + a[1] * b[2], a[0] * b[1] + a[1] * b[3], a[2] * b[0] + a[3] * b[2], a[2] * b[1] + a[3] * b[3]),
                   ((a[0] * B.t[0] + a[1] * B.t[1]) + A.t[0], (a[2] * B.t[0] + a[3] * B.t[1]) + A.t[1]))

    def inv(A):  # Eigen's Affine inverse: general linear inverse, t' = -L^-1 t
        a = A.l
        det = a[0] * a[3] - a[1] * a[2]
        d = 1.0 / det
        i = (a[3] * d, -a[1] * d, -a[2] * d, a[0] * d)
        return Aff(i, (-(i[0] * A.t[0] + i[1] * A.t[1]), -(i[2] * A.t[0] + i[3] * A.t[1])))

    def xyt(self):  # Affine3dToVectorXYeZ, utils.cpp:115-122
        return np.array([self.t[0], self.t[1], math.atan2(self.l[2], self.l[3])])


class Fuser:
    """One sequence. params: the oracle's Params. After every sweep: pose (x, y, theta), summary (the RegSummary of the sweep's Register,
    None on the first sweep), num_keyframes, n_cells, cov_current [6, 6]; reg_scans / reg_poses / reg_guess: what the sweep's Register
    was given and returned (the scans, the poses after the solve, the guess the prior sat on), costs: the sampled costs."""

    def __init__(self, oracle, params, soft_constraint=0, use_guess=1, cfar=None):
        self.o, self.p = oracle, params
        self.soft, self.use_guess, self.cfar = bool(soft_constraint), bool(use_guess), cfar
        self.T_prev, self.Tmot, self.Tcurrent = Aff(), Aff(), Aff()
        self.kf_scan, self.kf_pose = [], []
        self.summary, self.n_cells, self.frames = None, 0, 0
        self.cov_current = np.eye(6)
        self.cov_sampling = None
        self.reg_scans = self.reg_poses = self.reg_guess = self.costs = None
        self.cov_sampled = False

    def set_cov_sampling(self, enable=True, xy_range=0.4, yaw_range=0.0043625, steps=3, scaler=4.0):
        self.cov_sampling = dict(xy_range=xy_range, yaw_range=yaw_range, steps=steps, cov_scaler=scaler) if enable else None

    @property
    def num_keyframes(self):
        return len(self.kf_scan)

    def _add_to_reference(self, scan, T):  # :470-476
        self.kf_scan.append(scan); self.kf_pose.append(T)
        if len(self.kf_scan) > self.p.submap_scan_size:
            self.kf_scan.pop(0); self.kf_pose.pop(0)

    def process_polar(self, img):
        p = self.p
        if self.cfar is not None:  # radar_driver.cpp:52-56
            xyi = self.o.cfar(img, float(np.float32(p.range_res)), float(p.z_min), float(p.min_distance), **self.cfar)
        else:  # :58-59 (float z_min -> const int)
            xyi = self.o.cloud(self.o.filter_polar(img, int(p.z_min), p.k_strongest), p.range_res, p.min_distance)
        return self.process_cloud(xyi)

    def process_cloud(self, xyi):
        o, p = self.o, self.p
        TprevMot = self.Tmot  # :146
        if p.compensate:
            xyi = o.compensate(xyi, TprevMot.xyt(), p.radar_ccw)  # :147
        cur = o.Scan(xyi, p)  # :161
        self.n_cells = cur.size
        Tguess = self.T_prev.mul(TprevMot) if self.use_guess else self.T_prev  # :165-168
        self.frames += 1
        if not self.kf_scan:  # :171-177
            self._add_to_reference(cur, Aff())
            self.summary = None
            self.reg_scans = None
            return self.Tcurrent.xyt()
        # FormatScans (:478-494): keyframes oldest first, the current scan last, every covariance Identity66
        scans = list(self.kf_scan) + [cur]
        poses = np.array([T.xyt() for T in self.kf_pose] + [Tguess.xyt()])
        if self.soft:  # :186
            _, poses_out, cov6, S = o.register_soft(scans, poses, np.eye(6), p)
        else:
            _, poses_out, cov6, S = o.register(scans, poses, p)
        # (what Register leaves in cov_vek.back(): the covariance where the solution is usable, the Identity66 it was given otherwise)
        self.cov_current = np.array(cov6) if S.usable else np.eye(6)  # :196
        self.summary, self.reg_scans, self.reg_poses, self.reg_guess = S, scans, np.array(poses_out), poses[-1].copy()
        self.costs, self.cov_sampled = None, False
        if self.cov_sampling:  # :202-208: GetCost samples without the prior (n_scan_normal.cpp:202), the soft Register's scaler (:435-441)
            ok, cs, costs = o.cov_by_sampling(scans, poses_out, p, S.final_cost, S.num_residuals, itr=S.outer_iterations, **self.cov_sampling)
            self.costs, self.cov_sampled = costs, ok
            if ok:
                self.cov_current = cs
        Tcurrent = Aff.from_xyt(*poses_out[-1])  # :195
        Tpi = self.T_prev.inv()
        Tmc = Tpi.mul(Tcurrent)
        # AccelerationVelocitySanityCheck (:76-94)
        dt, lim = 0.25, 200
        vel = math.sqrt(Tmc.t[0] * Tmc.t[0] + Tmc.t[1] * Tmc.t[1]) / dt
        ax, ay = (Tmc.t[0] - self.Tmot.t[0]) / (dt * dt), (Tmc.t[1] - self.Tmot.t[1]) / (dt * dt)
        acc = math.sqrt(ax * ax + ay * ay)
        if acc > lim or vel > lim:
            Tcurrent = Tguess  # :198-199
        self.Tmot = Tpi.mul(Tcurrent)  # :200
        self.Tcurrent = Tcurrent
        Tkeydiff = self.kf_pose[-1].inv().mul(Tcurrent)  # KeyFrameBasedFuse (:62-73)
        fuse = True
        if p.use_keyframe:
            tn = math.sqrt(Tkeydiff.t[0] * Tkeydiff.t[0] + Tkeydiff.t[1] * Tkeydiff.t[1])
            rot = abs(math.atan2(Tkeydiff.l[2], Tkeydiff.l[3]))
            fuse = (tn > p.min_keyframe_dist) or (rot > p.min_keyframe_rot_deg * math.pi / 180.0)
        if fuse:
            self._add_to_reference(cur, Tcurrent)  # :234-247
        self.T_prev = Tcurrent  # :257
        return Tcurrent.xyt()

    def counts(self):
        """(outer iterations, inner iterations of the first eight, residuals, keyframes, cells) as the device tests compare them"""
        S = self.summary
        if S is None:
            return (0, [], 0, self.num_keyframes, self.n_cells)
        no = max(int(S.outer_iterations), 0)
        return (int(S.outer_iterations), [int(v) for v in S.inner_iterations[:min(no, 8)]], int(S.num_residuals), self.num_keyframes, self.n_cells)


def run(oracle, kw, frames, soft_constraint=0, use_guess=1, cfar=None, cov_sampling=None, keep=None):
    """one recording through a Fuser under oracle.default_params(**kw) -> [sweep] (counts, pose); keep(t, fuser) is called after every
    sweep (to copy out what a test wants of the fuser's state)"""
    fu = Fuser(oracle, oracle.default_params(**kw), soft_constraint, use_guess, cfar)
    if cov_sampling:
        fu.set_cov_sampling(True, **cov_sampling)
    out = []
    for t, img in enumerate(frames):
        pose = fu.process_polar(img)
        out.append((fu.counts(), np.array(pose)))
        if keep:
            keep(t, fu)
    return out


# ---- the drives and parameter sets the fuser-option tests share (tests/test_fuser_options_cpu.py checks on the reference alone that the
# switches change these trajectories by more than ten times the pose bar; tests/test_fuser_options_gpu.py compares the device on them) ----
A, R, RR = 400, 3360, np.float32(0.0595238)
P2P, P2L, P2D = 0, 1, 2
T_SWEEPS = 12
# (kind, world seed, seed) of synth.drive_chunks: drives on which the reference's trajectory moves by more than ten times the pose bar under
# either switch for every cost (on most drives the converged P2L registration barely depends on where it starts)
SEQS = [("canyon", 13, 23), ("blocks", 15, 25), ("canyon", 29, 39), ("blocks", 14, 24)]
BASE = dict(range_res=RR, k_strongest=12, z_min=60.0, res=3.0, weight_intensity=1, weight_opt=0, compensate=1, radar_ccw=0, cost=P2L, loss=1,
            loss_limit=0.1, covar_scale=1.0, regularization=1.0, submap_scan_size=4)
COSTS = {"P2L": dict(BASE, cost=P2L, loss=1), "P2D": dict(BASE, cost=P2D, loss=0), "P2P": dict(BASE, cost=P2P, loss=0, weight_opt=4)}
OPTIONS = [(0, 1), (1, 1), (0, 0), (1, 0)]  # (soft_constraint, use_guess)
_DRIVES, _RUNS = {}, {}


def drive(kind, world_seed, seed, T=T_SWEEPS):
    from cfear_radarodometry_code_public_amd import synth
    key = (kind, world_seed, seed, T)
    if key not in _DRIVES:
        fr = np.empty((T, A, R), dtype=np.uint8)
        for t0, chunk in synth.drive_chunks(T, kind, world_seed, seed, A, R, RR, ccw=False, procs=4):
            fr[t0:t0 + len(chunk)] = chunk
        _DRIVES[key] = fr
    return _DRIVES[key]


def frames_of(seqs=SEQS, T=T_SWEEPS):
    """[T, len(seqs), A, R]"""
    return np.ascontiguousarray(np.stack([drive(*s, T=T) for s in seqs], axis=1))


def reference(oracle, name, kw, seq, soft_constraint, use_guess, T=T_SWEEPS):
    """run() of one shared drive under one parameter set and option pair, computed once per process"""
    key = (name, tuple(seq), int(soft_constraint), int(use_guess), T)
    if key not in _RUNS:
        _RUNS[key] = run(oracle, kw, drive(*seq, T=T), soft_constraint, use_guess)
    return _RUNS[key]
