"""Planar pose graphs on the host: the numpy / scipy side of the batched optimiser of pose_graph.hip (include/cfear_hip.h states the problem).
No device anywhere in this module.

  problem(nodes, edges)        KEYFRAME_NODE_DTYPE / KEYFRAME_EDGE_DTYPE arrays (a log's, or replay.read_g2o / read_g2o_edges of any g2o file
                               this project wrote) -> (poses [n, 3], edges as capi.PG_EDGE_DTYPE), the input of Context.pose_graph_optimize
  cost(poses, edges, ...)      F = 1/2 sum rho(e^T Omega e)
  optimize(poses, edges, ...)  the twin of the device algorithm, step for step in float64: Levenberg-Marquardt with Marquardt damping,
                               conjugate gradients under the block-Jacobi preconditioner, the same tolerances and step rule. Its sums run
                               in numpy's order, not the kernel's: it agrees with the device to rounding, not to the bit.
  optimize_direct(...)         an independent checker: Gauss-Newton with a sparse direct solve (scipy.sparse.linalg.spsolve) to a step below
                               1e-13. It shares neither the damping nor CG with the twin. No loss.

The error of an edge (a, b, z, Omega) is expressed in the frame of a:  e_xy = R(theta_a)^T (t_b - t_a) - z_xy,  e_th = wrap(theta_b - theta_a -
z_th) to [-pi, pi)."""
import numpy as np

from . import capi

TERMINATION = capi.PG_TERMINATION
DIAG_MIN, LAMBDA_MIN, LAMBDA_MAX = 1e-6, 1e-12, 1e8
G2O_INFO = (0, 1, 5)  # rows / columns of a 6x6 information (x, y, z, roll, pitch, yaw) that a planar edge carries (replay.G2O_INFO)
_TRI = [(i, j) for i in range(3) for j in range(i, 3)]


def wrap_pi(a):
    return a - 2.0 * np.pi * np.floor((a + np.pi) / (2.0 * np.pi))


def _tri6(information):
    info = np.asarray(information, dtype=np.float64).reshape(6, 6)
    return [info[G2O_INFO[i], G2O_INFO[j]] for i, j in _TRI]


def problem(nodes, edges=None):
    """nodes (KEYFRAME_NODE_DTYPE) and edges (KEYFRAME_EDGE_DTYPE, or None) of ONE sequence -> (poses [n, 3], PG_EDGE_DTYPE edges): every node
    with a `prev` gives its own edge (a = the node, b = prev, z = t_be, the (x, y, yaw) block of its information; flag bit 0 clear), then the
    edges with success != 0 and status == 0 follow in their order as (a = to, b = from) with flag bit 0 set - the lines of replay.g2o_text.
    Nodes are addressed by their position in `nodes` (their `index` field names them in the edges)."""
    nodes = np.asarray(nodes)
    pos = {int(nd["index"]): k for k, nd in enumerate(nodes)}
    rows = []
    for k, nd in enumerate(nodes):
        if int(nd["prev"]) >= 0:
            rows.append((k, pos[int(nd["prev"])], 0, nd["t_be"], _tri6(nd["information"])))
    for e in (edges if edges is not None else ()):
        if int(e["success"]) and int(e["status"]) == 0:
            rows.append((pos[int(e["to"])], pos[int(e["from"])], 1, e["t_be"], _tri6(e["information"])))
    out = np.zeros(len(rows), dtype=capi.PG_EDGE_DTYPE)
    for k, (a, b, fl, z, tri) in enumerate(rows):
        out[k]["a"], out[k]["b"], out[k]["flags"], out[k]["z"], out[k]["info"] = a, b, fl, z, tri
    return np.array(nodes["pose"], dtype=np.float64).reshape(-1, 3), out


def make_edges(a, b, z, info, flags=0):
    """arrays -> PG_EDGE_DTYPE: a, b [m], z [m, 3], info [m, 3, 3] (symmetric) or [m, 6] (upper triangle), flags a scalar or [m]"""
    a = np.asarray(a, dtype=np.int32).reshape(-1)
    out = np.zeros(len(a), dtype=capi.PG_EDGE_DTYPE)
    out["a"], out["b"], out["flags"] = a, np.asarray(b, dtype=np.int32).reshape(-1), flags
    out["z"] = np.asarray(z, dtype=np.float64).reshape(-1, 3)
    info = np.asarray(info, dtype=np.float64)
    out["info"] = info.reshape(-1, 6) if info.shape[-1] == 6 else np.stack([info.reshape(-1, 3, 3)[:, i, j] for i, j in _TRI], axis=1)
    return out


def usable(edges):
    """the edges whose z and info are finite (the others are skipped and counted)"""
    E = np.asarray(edges)
    return np.isfinite(E["z"]).all(axis=1) & np.isfinite(E["info"]).all(axis=1)


def _omega(E):
    t = E["info"]
    return np.stack([np.stack([t[:, 0], t[:, 1], t[:, 2]], axis=1), np.stack([t[:, 1], t[:, 3], t[:, 4]], axis=1),
                     np.stack([t[:, 2], t[:, 4], t[:, 5]], axis=1)], axis=1)


def errors(poses, edges):
    """e [m, 3] of every edge at poses [n, 3]"""
    x, E = np.asarray(poses, dtype=np.float64).reshape(-1, 3), np.asarray(edges)
    pa, pb = x[E["a"]], x[E["b"]]
    c, s = np.cos(pa[:, 2]), np.sin(pa[:, 2])
    dx, dy = pb[:, 0] - pa[:, 0], pb[:, 1] - pa[:, 1]
    return np.stack([c * dx + s * dy - E["z"][:, 0], -s * dx + c * dy - E["z"][:, 1], wrap_pi(pb[:, 2] - pa[:, 2] - E["z"][:, 2])], axis=1)


def jacobians(poses, edges):
    """(A, B) [m, 3, 3] each: de / d(pose of a), de / d(pose of b), analytic"""
    x, E = np.asarray(poses, dtype=np.float64).reshape(-1, 3), np.asarray(edges)
    pa, pb = x[E["a"]], x[E["b"]]
    c, s = np.cos(pa[:, 2]), np.sin(pa[:, 2])
    dx, dy = pb[:, 0] - pa[:, 0], pb[:, 1] - pa[:, 1]
    rx, ry = c * dx + s * dy, -s * dx + c * dy
    m = len(E)
    A, B = np.zeros((m, 3, 3)), np.zeros((m, 3, 3))
    A[:, 0, 0], A[:, 0, 1], A[:, 0, 2] = -c, -s, ry
    A[:, 1, 0], A[:, 1, 1], A[:, 1, 2] = s, -c, -rx
    A[:, 2, 2] = -1.0
    B[:, 0, 0], B[:, 0, 1], B[:, 1, 0], B[:, 1, 1], B[:, 2, 2] = c, s, -s, c, 1.0
    return A, B


def loss_eval(loss, limit, s, flagged):
    """(rho(s), rho'(s)) per edge: Ceres' HuberLoss / CauchyLoss on the squared norm where `flagged`, the identity elsewhere"""
    s = np.asarray(s, dtype=np.float64)
    rho, w = s.copy(), np.ones_like(s)
    if loss == capi.LOSS_HUBER:
        b = limit * limit
        k = flagged & (s > b)
        r = np.sqrt(s[k])
        rho[k], w[k] = 2.0 * limit * r - b, limit / r
    elif loss == capi.LOSS_CAUCHY:
        b = limit * limit
        t = 1.0 + s[flagged] / b
        rho[flagged], w[flagged] = b * np.log(t), 1.0 / t
    elif loss != capi.LOSS_NONE:
        raise ValueError("posegraph: loss %r (LOSS_NONE, LOSS_HUBER or LOSS_CAUCHY)" % (loss,))
    return rho, w


def cost(poses, edges, loss=0, loss_limit=0.1):
    """F = 1/2 sum rho(e^T Omega e) over the usable edges"""
    E = np.asarray(edges)
    E = E[usable(E)]
    if len(E) == 0:
        return 0.0
    e = errors(poses, E)
    s = np.einsum("mi,mij,mj->m", e, _omega(E), e)
    rho, _ = loss_eval(int(loss), float(loss_limit), s, (E["flags"] & 1) != 0)
    return 0.5 * float(np.sum(rho))


def _check(n, E, fixed):
    if len(E) and (E["a"].min() < 0 or E["b"].min() < 0 or E["a"].max() >= n or E["b"].max() >= n or np.any(E["a"] == E["b"])):
        raise ValueError("posegraph: an edge names a node outside the graph, or a == b")
    if n and not 0 <= fixed < n:
        raise ValueError("posegraph: fixed = %d of %d nodes" % (fixed, n))


def _system(x, E, loss, limit):
    """the edges linearised at x: gradient [n, 3], H as a sparse matrix [3n, 3n], the diagonal blocks [n, 3, 3]"""
    from scipy import sparse
    n = len(x)
    e = errors(x, E)
    A, B = jacobians(x, E)
    Om = _omega(E)
    s = np.einsum("mi,mij,mj->m", e, Om, e)
    _, w = loss_eval(loss, limit, s, (E["flags"] & 1) != 0)
    W = w[:, None, None] * Om
    We = np.einsum("mij,mj->mi", W, e)
    g = np.zeros((n, 3))
    np.add.at(g, E["a"], np.einsum("mji,mj->mi", A, We))
    np.add.at(g, E["b"], np.einsum("mji,mj->mi", B, We))
    WA, WB = W @ A, W @ B
    blocks = [(E["a"], E["a"], np.einsum("mki,mkj->mij", A, WA)), (E["b"], E["b"], np.einsum("mki,mkj->mij", B, WB)),
              (E["a"], E["b"], np.einsum("mki,mkj->mij", A, WB)), (E["b"], E["a"], np.einsum("mki,mkj->mij", B, WA))]
    D = np.zeros((n, 3, 3))
    np.add.at(D, E["a"], blocks[0][2])
    np.add.at(D, E["b"], blocks[1][2])
    ii, jj, vv = [], [], []
    k3 = np.arange(3)
    for r, c, blk in blocks:
        ii.append((3 * r[:, None, None] + k3[None, :, None] + 0 * k3[None, None, :]).ravel())
        jj.append((3 * c[:, None, None] + 0 * k3[None, :, None] + k3[None, None, :]).ravel())
        vv.append(blk.ravel())
    H = sparse.csr_matrix((np.concatenate(vv), (np.concatenate(ii), np.concatenate(jj))), shape=(3 * n, 3 * n))
    return g, H, D


def optimize(poses, edges, fixed=0, max_iterations=50, max_linear_iterations=0, linear_tolerance=1e-8, function_tolerance=1e-12,
             parameter_tolerance=1e-10, initial_damping=1e-4, loss=0, loss_limit=0.1):
    """The device algorithm in numpy -> (poses [n, 3], summary: a dict with the fields of capi.PG_SUMMARY_DTYPE). See include/cfear_hip.h."""
    x = np.array(poses, dtype=np.float64).reshape(-1, 3)
    E = np.asarray(edges)
    n, fixed, loss, limit = len(x), int(fixed), int(loss), float(loss_limit)
    _check(n, E, fixed)
    ok = usable(E) if len(E) else np.zeros(0, dtype=bool)
    S = dict(initial_cost=0.0, final_cost=0.0, iterations=0, accepted=0, linear_iterations=0, edges_used=int(ok.sum()), edges_skipped=int(len(E) - ok.sum()),
             termination=capi.PG_NOTHING_TO_DO, status=0)
    if n == 0 or not ok.any():
        S["edges_used"], S["edges_skipped"] = 0, len(E)
        return x, S
    E = E[ok]
    free = np.ones(n, dtype=bool)
    free[fixed] = False
    fmask = np.repeat(free, 3)
    max_lin = int(max_linear_iterations) if max_linear_iterations > 0 else 30 * n
    F = cost(x, E, loss, limit)
    S["initial_cost"] = F
    lam = float(initial_damping)
    term = capi.PG_ITERATION_LIMIT
    it = accepted = lin_total = 0
    while it < max_iterations:
        it += 1
        g, H, D = _system(x, E, loss, limit)
        dg = np.maximum(np.stack([D[:, 0, 0], D[:, 1, 1], D[:, 2, 2]], axis=1), DIAG_MIN)  # [n, 3]
        Md = D.copy()
        for c in range(3):
            Md[:, c, c] += lam * dg[:, c]
        M = np.linalg.inv(Md)
        M[~free] = 0.0
        damp = (lam * dg).ravel()
        r = -g
        r[~free] = 0.0
        z = np.einsum("nij,nj->ni", M, r)
        d = z.copy()
        p = np.zeros_like(x)
        rz, rr = float(np.sum(r * z)), float(np.sum(r * r))
        gnorm = np.sqrt(rr)
        k = 0
        while k < max_lin and not np.sqrt(rr) <= linear_tolerance * gnorm:
            dv = d.ravel()
            q = ((H @ dv + damp * dv) * fmask).reshape(n, 3)
            dq = float(np.sum(d * q))
            if not dq > 0.0:
                break
            alpha = rz / dq
            p += alpha * d
            r -= alpha * q
            z = np.einsum("nij,nj->ni", M, r)
            rz_new, rr = float(np.sum(r * z)), float(np.sum(r * r))
            beta = rz_new / rz
            rz = rz_new
            d = z + beta * d
            k += 1
        lin_total += k
        if np.max(np.abs(p)) < parameter_tolerance:
            term = capi.PG_CONVERGED_STEP
            break
        xn = x + p
        Fn = cost(xn, E, loss, limit)
        if Fn < F:
            x[free] = xn[free]
            accepted += 1
            drop, Fold = F - Fn, F
            F = Fn
            lam = max(lam / 3.0, LAMBDA_MIN)
            if drop <= function_tolerance * Fold:
                term = capi.PG_CONVERGED_COST
                break
        else:
            if lam >= LAMBDA_MAX:
                term = capi.PG_DAMPING_LIMIT
                break
            lam = min(4.0 * lam, LAMBDA_MAX)
    S.update(final_cost=F, iterations=it, accepted=accepted, linear_iterations=lin_total, termination=term)
    return x, S


def optimize_direct(poses, edges, fixed=0, step_tolerance=1e-13, max_iterations=100):
    """Gauss-Newton with a sparse direct solve of the normal equations (the fixed node's rows and columns removed), no damping, no loss; a
    step that does not lower the cost is halved (at most 30 times); steps below 1e-6 are taken whole -> (poses, dict(cost, iterations,
    last_step)). It ends when max|step| < step_tolerance, or when the steps stop shrinking (the rounding floor of the solve: last_step says
    where that was). The graph must be connected to the fixed node (the system is singular otherwise)."""
    from scipy.sparse.linalg import spsolve
    x = np.array(poses, dtype=np.float64).reshape(-1, 3)
    E = np.asarray(edges)
    n, fixed = len(x), int(fixed)
    _check(n, E, fixed)
    E = E[usable(E)]
    keep = np.repeat(np.arange(n) != fixed, 3)
    F = cost(x, E)
    it, last = 0, np.inf
    while it < max_iterations:
        it += 1
        g, H, _ = _system(x, E, capi.LOSS_NONE, 0.0)
        Hs = H.tocsc()[keep][:, keep]
        dx = np.zeros(3 * n)
        dx[keep] = spsolve(Hs, -g.ravel()[keep])
        dx = dx.reshape(n, 3)
        prev, last = last, float(np.max(np.abs(dx)))
        if last < step_tolerance:
            break
        if last < 1e-6:  # Newton's last steps: the cost no longer resolves them - taken whole until they stop shrinking (the rounding floor)
            if last >= 0.5 * prev and prev < 1e-6:
                break
            x = x + dx
            F = cost(x, E)
            continue
        t, moved = 1.0, False
        for _ in range(30):
            Fn = cost(x + t * dx, E)
            if Fn < F:
                x, F, moved = x + t * dx, Fn, True
                break
            t *= 0.5
        if not moved:
            break
    return x, dict(cost=F, iterations=it, last_step=last)


def out_and_back(n, seed=0, spacing=1.5, heading=0.0, noise=(0.02, 0.02, 0.004), loop_noise=(0.02, 0.02, 0.003), min_index_gap=6, max_dist=3.0,
                 max_per_node=3, lateral=0.8, wrap=False):
    """A synthetic drive for tests and tools: n keyframes `spacing` apart, out along `heading` and back `lateral` metres beside the way out
    (two quarter turns), noisy chain edges integrated into the initial poses, and loop edges between the TRUE poses by the
    loop_candidates rule (min_index_gap, max_dist, max_per_node nearest) with noise of their own -> (initial poses [n, 3], PG_EDGE_DTYPE
    edges: the chain with flag 0, the loops with flag 1, true poses [n, 3]). wrap: the initial headings are wrapped to [-pi, pi) (a drive
    heading west then has neighbours on both sides of +-pi). Deterministic in `seed`."""
    rng = np.random.default_rng(seed)
    half = n // 2
    true = np.zeros((n, 3))
    x = y = 0.0
    th = float(heading)
    for i in range(n):
        true[i] = (x, y, th)
        if i == half - 1 or i == half:  # two quarter turns, `lateral` across: the way back runs beside the way out
            th += np.pi / 2.0
        step = lateral if i == half - 1 else spacing
        x, y = x + step * np.cos(th), y + step * np.sin(th)

    def rel(pa, pb):
        c, s = np.cos(pa[2]), np.sin(pa[2])
        dx, dy = pb[0] - pa[0], pb[1] - pa[1]
        return np.array([c * dx + s * dy, -s * dx + c * dy, wrap_pi(pb[2] - pa[2])])

    def info_of(sig):
        Lm = np.diag(1.0 / np.asarray(sig)) + 0.05 / max(sig) * np.triu(np.ones((3, 3)), 1)  # correlated: every entry of Omega is used
        return Lm.T @ Lm

    a, b, z, info, flags = [], [], [], [], []
    for i in range(1, n):
        a.append(i); b.append(i - 1); flags.append(0)
        z.append(rel(true[i], true[i - 1]) + rng.normal(0.0, noise))
        info.append(info_of(noise))
    init = np.zeros((n, 3))
    init[0] = true[0]
    for i in range(1, n):  # T_{i-1} = T_i * z  =>  T_i = T_{i-1} * z^-1
        zx, zy, zt = z[i - 1]
        ti = init[i - 1, 2] - zt
        c, s = np.cos(ti), np.sin(ti)
        init[i] = (init[i - 1, 0] - (c * zx - s * zy), init[i - 1, 1] - (s * zx + c * zy), ti)
    for to in range(n):
        last = to - min_index_gap
        if last < 0:
            continue
        dist = np.hypot(true[:last + 1, 0] - true[to, 0], true[:last + 1, 1] - true[to, 1])
        near = np.flatnonzero(dist <= max_dist)
        near = near[np.argsort(dist[near], kind="stable")][:max_per_node]
        for f in near:
            a.append(to); b.append(int(f)); flags.append(1)
            z.append(rel(true[to], true[int(f)]) + rng.normal(0.0, loop_noise))
            info.append(info_of(loop_noise))
    if wrap:
        init[:, 2] = wrap_pi(init[:, 2])
    return init, make_edges(a, b, np.array(z), np.array(info), np.array(flags, dtype=np.int32)), true
