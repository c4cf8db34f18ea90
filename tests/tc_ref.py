"""numpy restatement of n_scan_normal_reg::RegisterTimeContinuous (n_scan_normal.cpp:67-80) for the time-continuous tests: Register
(:82-187) with the time_continuous_ branch of AddScanPairCost (:215-326), built from oracle primitives only - Scan.cells(),
Scan.closest() and loss_eval. associate / build / evaluate / solve / register follow the LM transcription of
test_oracle_lm_transcription_cpu.py, extended by what the device summary reports: every loss, the soft prior
(mahalanobisDistanceError, n_scan_normal.h:259-290), the termination types, the covariance (:392-433) and the failure returns.

The time-continuous part, in the reference's order of operations: for source cell j
    ts_j     = GetRelTimeStamp(u_j, ccw)                          (utils.h:28-32)
    Tcomp_j  = vectorToAffine2d(ts_j vx, ts_j vy, ts_j vtheta)    (:235)
    T_j      = (Ttar^-1 Tsrc) Tcomp_j                             (:236) - composed first, then applied
    query    = float(T_j u_j), gate / similarity with T_j.linear() n_j
    residual = P2P: the corrected mean Tcomp_j u_j (P2PEfficientContinuousCost, n_scan_normal.h:363-404)
               P2L, P2D: the UNCORRECTED mean u_j (:279-300) - quirk q19; corrected_residual=True is the variant a reader
               would expect (the corrected mean everywhere), which the device must NOT agree with."""
import math
from types import SimpleNamespace

import numpy as np

P2P, P2L, P2D = 0, 1, 2
DBL_MAX = np.finfo(np.float64).max
STAMP_EDGE = 1e-5  # GetRelTimeStamp's discontinuity: a > 0.00001 ? a : 2 pi + a


def aff(x, y, th):
    """vectorToAffine3d (registration.cpp:130-136) as a homogeneous 3 x 3"""
    c, s = math.cos(th), math.sin(th)
    return np.array([[c, -s, x], [s, c, y], [0.0, 0.0, 1.0]])


def aff_inv(T):
    """Eigen's Affine inverse: general linear inverse, t' = -L^-1 t"""
    L = T[:2, :2]
    det = L[0, 0] * L[1, 1] - L[0, 1] * L[1, 0]
    Li = np.array([[L[1, 1], -L[0, 1]], [-L[1, 0], L[0, 0]]]) * (1.0 / det)
    out = np.eye(3)
    out[:2, :2] = Li
    out[:2, 2] = -(Li @ T[:2, 2])
    return out


def round_trip(pose):
    """Affine3dToVectorXYeZ(vectorToAffine3d(pose)) (utils.cpp:115-122)"""
    return np.array([pose[0], pose[1], math.atan2(math.sin(pose[2]), math.cos(pose[2]))])


def rel_stamp(x, y, ccw):
    a = math.atan2(y, x)
    d = (a if a > 0.00001 else (2 * math.pi + a)) / (2 * math.pi)
    return -(d - 0.5) if ccw else (d - 0.5)


def stamp_margin(cells):
    """smallest |atan2(u_y, u_x) - 1e-5| over the cells: every test asserts it is not within 1e-9 of the stamp's discontinuity"""
    a = np.arctan2(cells["mean"][:, 1], cells["mean"][:, 0])
    return float(np.min(np.abs(a - STAMP_EDGE))) if len(a) else np.inf


def tcomp(mean, vel, ccw):
    ts = rel_stamp(mean[0], mean[1], ccw)
    return aff(ts * vel[0], ts * vel[1], ts * vel[2])


def compensate_cells(cells, vel, ccw):
    """the cells with mean <- Tcomp_j mean, normal <- Tcomp_j.linear() normal (everything else as it is): what a P2P
    time-continuous registration is the plain registration of"""
    out = cells.copy()
    for j in range(len(out)):
        T = tcomp(cells["mean"][j], vel, ccw)
        out["mean"][j] = T[:2, :2] @ cells["mean"][j] + T[:2, 2]
        out["normal"][j] = T[:2, :2] @ cells["normal"][j]
    return out


def _sim(a, b):
    return 2 * min(a, b) / (a + b)


def weight(opt, cs, ct, sim):
    n1, n2, p1, p2 = float(cs["nsamples"]), float(ct["nsamples"]), float(cs["scale"]), float(ct["scale"])
    return {0: 1.0, 1: _sim(n1, n2), 2: sim, 3: _sim(p1, p2), 4: _sim(n1, n2) + sim + _sim(p1, p2)}.get(opt, 1.0)


def build(targets, tcells, src, par, p, itr, vel=None, ccw=False, corrected_residual=False):
    """AddScanPairCost for every keyframe (:215-326, :359-367): the residual blocks in (keyframe, source cell) order as arrays
    tm (M, 2), ex (M, 3) = (tn_x, tn_y, 0) or the P2D factor (l00, l10, l11), s (M, 2), w (M)"""
    radius = 2 * p.assoc_radius if itr == 1 else p.assoc_radius  # :222
    Tsrc = aff(*par[-1])
    cos30 = math.cos(math.pi / 6)
    tm, ex, sm, w = [], [], [], []
    for i, tar in enumerate(targets):
        Ttar = aff(*par[i])
        Trel = aff_inv(Ttar) @ Tsrc  # :224
        ct_all = tcells[i]
        for j in range(len(src)):
            cs = src[j]
            u = cs["mean"]
            T, s_res = Trel, u
            if vel is not None:
                Tc = tcomp(u, vel, ccw)
                T = Trel @ Tc  # :236
                if p.cost == P2P or corrected_residual:
                    s_res = Tc[:2, :2] @ u + Tc[:2, 2]
            q = T[:2, :2] @ u + T[:2, 2]
            ti = tar.closest(q[0], q[1], radius)
            if ti < 0:
                continue
            ct = ct_all[ti]
            n = T[:2, :2] @ cs["normal"]
            sim = max(float(n @ ct["normal"]), 0.0)
            if not sim > cos30:  # :247
                continue
            Rt, tt = Ttar[:2, :2], Ttar[:2, 2]
            tm.append(Rt @ ct["mean"] + tt)
            if p.cost == P2D:  # :290-299
                C = np.array([[ct["cov"][0], ct["cov"][1]], [ct["cov"][1], ct["cov"][2]]])
                Cw = (Rt @ C @ Rt.T + p.regularization * np.eye(2)) * p.covar_scale
                det = Cw[0, 0] * Cw[1, 1] - Cw[0, 1] * Cw[1, 0]
                i00, i10, i11 = Cw[1, 1] / det, -Cw[1, 0] / det, Cw[0, 0] / det
                l00 = math.sqrt(i00)
                l10 = i10 / l00
                ex.append([l00, l10, math.sqrt(i11 - l10 * l10)])
            else:
                tn = Rt @ ct["normal"]
                ex.append([tn[0], tn[1], 0.0])
            sm.append(np.array(s_res, dtype=np.float64))
            w.append(weight(p.weight_opt, cs, ct, sim))
    return SimpleNamespace(tm=np.array(tm).reshape(-1, 2), ex=np.array(ex).reshape(-1, 3), s=np.array(sm).reshape(-1, 2), w=np.array(w), n=len(w))


def prior_terms(prior_cov6, guess, n_src):
    """:373-376: guess_inf_sqrt = Cov6to3(cov).inverse().llt().matrixL(), alpha = sqrt(#source cells)"""
    C = np.asarray(prior_cov6, dtype=np.float64).reshape(6, 6)[np.ix_([0, 1, 5], [0, 1, 5])]
    return np.linalg.cholesky(np.linalg.inv(C)), np.array(guess, dtype=np.float64), math.sqrt(n_src)


def evaluate(oracle, B, p, x, prior=None, grad=True):
    """cost 1/2 sum w rho(s) (+ prior), gradient J~^T r~ and Gauss-Newton matrix J~^T J~ with the corrector sqrt(w rho')"""
    c, s = math.cos(x[2]), math.sin(x[2])
    px = (c * B.s[:, 0] - s * B.s[:, 1]) + x[0]
    py = (s * B.s[:, 0] + c * B.s[:, 1]) + x[1]
    dtx = -s * B.s[:, 0] - c * B.s[:, 1]
    dty = c * B.s[:, 0] - s * B.s[:, 1]
    one, zero = np.ones(B.n), np.zeros(B.n)
    if p.cost == P2L:
        r = [(px - B.tm[:, 0]) * B.ex[:, 0] + (py - B.tm[:, 1]) * B.ex[:, 1]]
        J = [[B.ex[:, 0], B.ex[:, 1], dtx * B.ex[:, 0] + dty * B.ex[:, 1]]]
    elif p.cost == P2D:
        dx, dy = px - B.tm[:, 0], py - B.tm[:, 1]
        r = [B.ex[:, 0] * dx, B.ex[:, 1] * dx + B.ex[:, 2] * dy]
        J = [[B.ex[:, 0], zero, B.ex[:, 0] * dtx], [B.ex[:, 1], B.ex[:, 2], B.ex[:, 1] * dtx + B.ex[:, 2] * dty]]
    else:
        r = [B.tm[:, 0] - px, B.tm[:, 1] - py]
        J = [[-one, zero, -dtx], [zero, -one, -dty]]
    sq = sum(rk * rk for rk in r)
    rho = np.array([oracle.loss_eval(p.loss, p.loss_limit, float(v))[:2] for v in sq]).reshape(-1, 2) * B.w[:, None]  # ScaledLoss (:277)
    f = 0.5 * float(np.sum(rho[:, 0]))
    g, H = np.zeros(3), np.zeros((3, 3))
    if grad:
        sr = np.sqrt(rho[:, 1])
        for rk, Jk in zip(r, J):
            Jt = np.stack([sr * Jk[0], sr * Jk[1], sr * Jk[2]], axis=1)
            g += Jt.T @ (sr * rk)
            H += Jt.T @ Jt
    if prior is not None:  # r = L (alpha (guess - x)), J = -alpha L, no loss
        L, guess, alpha = prior
        rp = L @ (alpha * (guess - np.asarray(x, dtype=np.float64)))
        f += 0.5 * float(rp @ rp)
        if grad:
            Jp = -alpha * L
            g += Jp.T @ rp
            H += Jp.T @ Jp
    return f, g, H


def _chol_solve(A, b):
    try:
        np.linalg.cholesky(A)
        y = np.linalg.solve(A, b)
    except np.linalg.LinAlgError:
        return None
    return y if np.all(np.isfinite(y)) else None


def solve(oracle, B, p, x0, prior=None):
    """Ceres trust-region LM with default options -> (x, iterations incl. the initial evaluation, final_cost,
    last relative decrease, termination 0 CONVERGENCE / 1 NO_CONVERGENCE / 2 FAILURE)"""
    x = np.array(x0, dtype=np.float64)
    f, g, H = evaluate(oracle, B, p, x, prior)
    iters, final_cost, last_rho = 1, f, 0.0
    if np.max(np.abs(g)) <= 1e-10:
        return x, iters, final_cost, last_rho, 0
    sc = 1.0 / (1.0 + np.sqrt(np.diag(H)))  # Jacobi scaling, once
    radius, dec, reuse, invalid, it = 1e4, 2.0, False, 0, 0
    dg = np.zeros(3)
    max_inner = p.max_solver_iterations
    while True:
        if it >= max_inner:
            return x, iters, final_cost, last_rho, 1
        if radius < 1e-32:
            return x, iters, final_cost, last_rho, 0
        it += 1
        Hs, gs = H * np.outer(sc, sc), g * sc
        if not reuse:
            dg = np.clip(np.diag(Hs), 1e-6, 1e32)
        reuse = True
        y = _chol_solve(Hs + np.diag(dg / radius), -gs)
        mcc = 0.0
        if y is not None:
            mcc = -(y @ gs + 0.5 * y @ Hs @ y)
            if not mcc > 0:
                y = None
        if y is None:  # HandleInvalidStep
            invalid += 1
            if invalid >= 5:
                return x, iters, final_cost, last_rho, 2
            radius /= dec
            dec *= 2
            iters += 1
            last_rho = 0.0
            final_cost = min(final_cost, f)
            continue
        invalid = 0
        xc = x + y * sc
        fc, _, _ = evaluate(oracle, B, p, xc, prior, grad=False)
        if np.linalg.norm(x - xc) <= 1e-8 * (np.linalg.norm(x) + 1e-8):
            return x, iters, final_cost, last_rho, 0
        change = f - fc
        if abs(change) <= 1e-6 * f:
            return x, iters, final_cost, last_rho, 0
        rho = change / mcc
        iters += 1
        last_rho = rho
        if rho > 1e-3:  # HandleSuccessfulStep
            x = xc
            f, g, H = evaluate(oracle, B, p, x, prior)
            t = 2.0 * rho - 1.0
            radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - t * t * t))
            dec, reuse = 2.0, False
            final_cost = min(final_cost, f)
            if it >= max_inner:
                return x, iters, final_cost, last_rho, 1
            if np.max(np.abs(g)) <= 1e-10:
                return x, iters, final_cost, last_rho, 0
        else:  # HandleUnsuccessfulStep
            radius /= dec
            dec *= 2
            reuse = True
            final_cost = min(final_cost, fc)


def register(oracle, scans, poses, p, vel=None, ccw=False, prior_cov6=None, src_cells=None, corrected_residual=False):
    """Register / RegisterTimeContinuous (vel = (vx, vy, vtheta), None: the plain Register). scans: oracle Scans (the keyframes
    are searched through Scan.closest); src_cells: the cells to use for the last scan instead of its own.
    -> (ret, poses, cov6 or None where the caller's covariance is left alone, summary) with the fields of cfear_reg_summary"""
    n = len(scans)
    poses_in = np.asarray(poses, dtype=np.float64).reshape(n, 3)
    par = np.array([round_trip(q) for q in poses_in])
    targets = scans[:-1]
    tcells = [s.cells() for s in targets]
    src = scans[-1].cells() if src_cells is None else src_cells
    prior = prior_terms(prior_cov6, par[-1], len(src)) if prior_cov6 is not None else None
    S = SimpleNamespace(success=0, usable=0, outer_iterations=0, num_residuals=0, num_residual_blocks=0, final_cost=0.0, score=0.0,
                        inner_iterations=[], termination=[], outer_cost=[])
    tsrc_last = poses_in[-1].copy()
    prev_par, prev_score = par[-1].copy(), DBL_MAX
    success, nres, B = True, 0, None
    final_cost, last_rho, iters = 0.0, 0.0, 0
    use_prior = None
    itr = 1
    while itr <= p.max_itr_association and success:  # :102
        B = build(targets, tcells, src, par, p, itr, vel, ccw, corrected_residual)
        nres = B.n * (1 if p.cost == P2L else 2)
        if nres <= 1:  # :370-371, :114-115
            success = False
            break
        use_prior = prior
        if prior is not None:
            nres += 3  # the prior block joins after the residual-count check (:370-377)
        x, iters, final_cost, last_rho, term = solve(oracle, B, p, par[-1], use_prior)
        par[-1] = x
        success = term != 2  # IsSolutionUsable
        if success:
            tsrc_last = par[-1].copy()
        S.inner_iterations.append(iters); S.termination.append(term); S.outer_cost.append(final_cost)
        if itr > p.min_itr:  # :134-149
            if prev_score < final_cost:
                par[-1] = prev_par
                break
            if (prev_score - final_cost) / prev_score < 0.00001:
                break
            if last_rho < 0.00001 or iters == 1:
                break
        prev_score, prev_par = final_cost, par[-1].copy()
        itr += 1
    S.outer_iterations = itr
    S.usable = int(success)
    S.num_residuals, S.num_residual_blocks, S.final_cost = nres, (B.n if B is not None else 0), final_cost
    out = poses_in.copy()
    cov, ret = None, 0
    if success:
        S.score = final_cost / nres  # :166
        out = par.copy()
        cov = np.zeros((6, 6)); cov[0, 0] = cov[1, 1] = 0.1 * 0.1; cov[5, 5] = 0.01 * 0.01  # :173
        _, _, H = evaluate(oracle, B, p, par[-1], use_prior)  # GetCovariance (:392-433)
        a, b, c, d, e, f = H[0, 0], H[0, 1], H[0, 2], H[1, 1], H[1, 2], H[2, 2]
        C00, C01, C02 = d * f - e * e, c * e - b * f, b * e - c * d
        det = a * C00 + b * C01 + c * C02
        dof = nres - 3
        if det > 0 and math.isfinite(det) and dof != 0:
            sc = 30 * (final_cost / dof) / det
            cov = np.eye(6)
            cov[0, 0], cov[0, 1], cov[1, 0], cov[1, 1] = sc * C00, sc * C01, sc * C01, sc * (a * f - c * c)
            cov[5, 5], cov[0, 5], cov[5, 0] = sc * (a * d - b * b), sc * C02, sc * C02  # (1,5)/(5,1) left 0: :426-430
            ret = 1
    else:
        out[-1] = tsrc_last
    S.success = ret
    return ret, out, cov, S


def decisions(S):
    """what has to be EQUAL between two runs of the same problem"""
    return (S.success, S.usable, S.outer_iterations, list(S.inner_iterations), list(S.termination), S.num_residuals, S.num_residual_blocks)


def on_decision_boundary(oracle, scans, poses, p, vel, ccw=False, prior_cov6=None):
    """an input sits on a decision boundary when this restatement changes its own counts after the velocity is perturbed by 1e-12"""
    base = decisions(register(oracle, scans, poses, p, vel, ccw, prior_cov6)[3])
    for sgn in (1.0, -1.0):
        v = np.asarray(vel, dtype=np.float64) + sgn * 1e-12
        if decisions(register(oracle, scans, poses, p, v, ccw, prior_cov6)[3]) != base:
            return True
    return False
