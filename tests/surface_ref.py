"""numpy restatement of n_scan_normal_reg::GetSurface (n_scan_normal.cpp:29-65) for the surface tests, built from oracle
primitives only: Scan.cells(), Scan.closest() and loss_eval. The problem is AddScanPairCost (:215-326) with Weights::GetWeight
(registration.cpp:67-76) built once at the round-tripped poses, the soft prior mahalanobisDistanceError (n_scan_normal.h:259-290)
when asked for and the problem has more than one residual (:370-377); a pixel is ceres::Problem::Evaluate at (x, y, yaw of the
estimate)."""
import math

import numpy as np

P2P, P2L, P2D = 0, 1, 2


def aff(x, y, th):
    c, s = math.cos(th), math.sin(th)
    return np.array([[c, -s], [s, c]]), np.array([x, y], dtype=np.float64)


def round_trip(pose):
    """Affine3dToVectorXYeZ(vectorToAffine3d(pose)) (utils.cpp:115-122)"""
    R, t = aff(*pose)
    return np.array([t[0], t[1], math.atan2(R[1, 0], R[1, 1])])


def _sim(a, b):
    return 2 * min(a, b) / (a + b)


def weight(opt, cs, ct, sim):
    n1, n2, p1, p2 = float(cs["nsamples"]), float(ct["nsamples"]), cs["scale"], ct["scale"]
    return {0: 1.0, 1: _sim(n1, n2), 2: sim, 3: _sim(p1, p2), 4: _sim(n1, n2) + sim + _sim(p1, p2)}.get(opt, 1.0)


def build_blocks(scans, poses, p, itr):
    """the residual blocks in residual-block order: (tm[2], tn[2] or L[3], source mean, weight)"""
    par = np.array([round_trip(q) for q in np.asarray(poses, dtype=np.float64)])
    radius = 2 * p.assoc_radius if itr == 1 else p.assoc_radius  # :222
    Rs, ts = aff(*par[-1])
    src = scans[-1].cells()
    blocks = []
    for i in range(len(scans) - 1):
        Rt, tt = aff(*par[i])
        Ri = np.linalg.inv(Rt)
        T = Ri @ Rs
        tr = Ri @ ts - Ri @ tt
        tar = scans[i].cells()
        for j in range(len(src)):
            cs = src[j]
            q = T @ cs["mean"] + tr
            ti = scans[i].closest(q[0], q[1], radius)
            if ti < 0:
                continue
            ct = tar[ti]
            n = T @ cs["normal"]
            sim = max(float(n @ ct["normal"]), 0.0)
            if not sim > math.cos(math.pi / 6):  # :247
                continue
            tm = Rt @ ct["mean"] + tt
            extra = Rt @ ct["normal"]
            if p.cost == P2D:  # :290-299
                C = np.array([[ct["cov"][0], ct["cov"][1]], [ct["cov"][1], ct["cov"][2]]])
                Cw = (Rt @ C @ Rt.T + p.regularization * np.eye(2)) * p.covar_scale
                Linf = np.linalg.cholesky(np.linalg.inv(Cw))
                extra = np.array([Linf[0, 0], Linf[1, 0], Linf[1, 1]])
            blocks.append((tm, extra, cs["mean"].copy(), weight(p.weight_opt, cs, ct, sim)))
    return par, blocks


def prior_terms(scans, par, prior_cov6):
    C = np.asarray(prior_cov6, dtype=np.float64).reshape(6, 6)[np.ix_([0, 1, 5], [0, 1, 5])]
    return np.linalg.cholesky(np.linalg.inv(C)), par[-1].copy(), math.sqrt(len(scans[-1].cells()))


def evaluate(oracle, blocks, p, x, prior=None):
    """ceres::Problem::Evaluate at x = (x, y, theta) -> (cost, robustified residuals)"""
    R, t = aff(*x)
    cost, res = 0.0, []
    for tm, extra, sm, w in blocks:
        pp = R @ sm + t
        if p.cost == P2L:
            r = np.array([(pp - tm) @ extra])
        elif p.cost == P2D:
            d = pp - tm
            r = np.array([extra[0] * d[0], extra[1] * d[0] + extra[2] * d[1]])
        else:
            r = tm - pp
        rho = oracle.loss_eval(p.loss, p.loss_limit, float(r @ r))
        cost += 0.5 * w * rho[0]
        res.extend(math.sqrt(w * rho[1]) * r)
    if prior is not None:
        L, guess, alpha = prior
        r = L @ (alpha * (guess - np.asarray(x)))
        cost += 0.5 * float(r @ r)
        res.extend(r)
    return cost, np.array(res)


def axis(v0, res, width, pixels):
    """the values `for (v = v0 - width; v <= v0 + width; v = v + res)` visits (n_scan_normal.cpp:52-54), at most pixels"""
    out, v = [], v0 - width
    while v <= v0 + width and len(out) < pixels:
        out.append(v)
        v = v + res
    return out


def surface(oracle, scans, poses, p, itr, res, width, prior_cov6=None):
    """GetSurface: (pixels, pixels), row i = x, column j = y, NaN where the loops never reach"""
    par, blocks = build_blocks(scans, poses, p, itr)
    nres = len(blocks) * (1 if p.cost == P2L else 2)
    prior = prior_terms(scans, par, prior_cov6) if (prior_cov6 is not None and nres > 1) else None
    pixels = int(math.ceil(2.0 * width / res)) + 1
    xs, ys = axis(par[-1][0], res, width, pixels), axis(par[-1][1], res, width, pixels)
    out = np.full((pixels, pixels), np.nan)
    for i, x in enumerate(xs):
        for j, y in enumerate(ys):
            out[i, j] = evaluate(oracle, blocks, p, (x, y, par[-1][2]), prior)[0]
    return out


def loss_rho(loss, a, s):
    """rho(s) of the registration's losses (registration.cpp:78-97) on an array of squared norms: the Ceres 2.0 closed forms that
    test_oracle_cpu.py pins for oracle.loss_eval, operation for operation (0 none, 1 Huber, 2 Cauchy, 3 SoftLOne, 4 Huber(1) of
    Cauchy(1), 5 Tukey)"""
    s = np.asarray(s, dtype=np.float64)
    b = a * a
    if loss == 1:
        return np.where(s > b, 2.0 * a * np.sqrt(s) - b, s)
    if loss == 2:
        return b * np.log(1.0 + s * (1.0 / b))
    if loss == 3:
        return 2.0 * b * (np.sqrt(1.0 + s * (1.0 / b)) - 1.0)
    if loss == 5:
        v = 1.0 - s / b
        return np.where(s <= b, b / 3.0 * (1.0 - (v * v) * v), b / 3.0)
    if loss == 4:
        return loss_rho(1, 1.0, loss_rho(2, 1.0, s))
    return s.copy()


def evaluate_grid(blocks, p, xs, ys, yaw, prior=None):
    """evaluate()'s cost at every (x, y) of xs x ys, yaw fixed: vectorised over the pixels, the blocks summed one after the other in
    residual-block order (the summation order of every pixel is evaluate()'s)"""
    X = np.asarray(xs, dtype=np.float64)[:, None]
    Y = np.asarray(ys, dtype=np.float64)[None, :]
    R, _ = aff(0.0, 0.0, yaw)
    cost = np.zeros((X.shape[0], Y.shape[1]))
    for tm, extra, sm, w in blocks:
        rs = R @ sm
        px, py = rs[0] + X, rs[1] + Y
        if p.cost == P2L:
            r0 = (px - tm[0]) * extra[0] + (py - tm[1]) * extra[1]
            sq = r0 * r0
        elif p.cost == P2D:
            dx, dy = px - tm[0], py - tm[1]
            r0, r1 = extra[0] * dx, extra[1] * dx + extra[2] * dy
            sq = r0 * r0 + r1 * r1
        else:
            r0, r1 = tm[0] - px, tm[1] - py
            sq = r0 * r0 + r1 * r1
        cost += 0.5 * w * loss_rho(p.loss, p.loss_limit, sq)
    if prior is not None:
        L, guess, alpha = prior
        d0, d1, d2 = alpha * (guess[0] - X), alpha * (guess[1] - Y), alpha * (guess[2] - yaw)
        acc = 0.0
        for i in range(3):
            r = (L[i, 0] * d0 + L[i, 1] * d1) + L[i, 2] * d2
            acc = acc + r * r
        cost += 0.5 * acc
    return cost


def surface_grid(oracle, scans, poses, p, itr, res, width, prior_cov6=None, with_blocks=False):
    """surface() for large grids: the same problem, the same result, the pixels vectorised (evaluate_grid). with_blocks: also the
    number of residual blocks, for tests that assert which regime they are in"""
    par, blocks = build_blocks(scans, poses, p, itr)
    nres = len(blocks) * (1 if p.cost == P2L else 2)
    prior = prior_terms(scans, par, prior_cov6) if (prior_cov6 is not None and nres > 1) else None
    pixels = int(math.ceil(2.0 * width / res)) + 1
    xs, ys = axis(par[-1][0], res, width, pixels), axis(par[-1][1], res, width, pixels)
    out = np.full((pixels, pixels), np.nan)
    out[:len(xs), :len(ys)] = evaluate_grid(blocks, p, xs, ys, par[-1][2], prior)
    return (out, len(blocks)) if with_blocks else out
