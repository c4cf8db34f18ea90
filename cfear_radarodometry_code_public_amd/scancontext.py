"""Scan-Context descriptors and loop candidates by appearance on the host: the definition of include/cfear_hip.h (cfear_sc_params) in numpy,
the twin the device code (csrc/scan_context.hip) is tested against. Pure numpy; the layout table alone comes from the library
(cfear_scan_context_layout, host only: no device), because numpy's cosine and libm's differ in the last place and the bin of a point on a
sector boundary depends on it.

  layout(params)             the table: squared ring edges and sector directions
  describe(cloud, params)    bins uint32 [n_sectors, n_rings], ring_sums uint32 [n_rings], dropped - integers, exact
  key_distance(ra, rb)       stage 1: the ring-key distance, exact
  distance(a, b)             stage 2 in float64: (distance, shift, yaw, margin to the best other shift)
  candidates(bins, params)   the candidates of one set of descriptors, SC_CANDIDATE_DTYPE with `sequence` 0
"""
import math

import numpy as np

from . import capi


def params(p=None, **kw):
    """a capi.ScParams: p (None: the defaults), in a copy with the fields given replaced"""
    if p is None:
        return capi.sc_params(**kw)
    if not kw:
        return p
    q = capi.ScParams.from_buffer_copy(p)
    for k, v in kw.items():
        if k == "pad_" or not hasattr(q, k):
            raise AttributeError(k)
        setattr(q, k, v)
    return q


def layout(p=None, **kw):
    """-> (ring_edge2 [n_rings + 1], sector_dir [n_sectors, 2]) of the library's table"""
    return capi.scan_context_layout(params(p, **kw))


def bins_of_points(cloud, p=None, table=None, **kw):
    """The bin of every point of cloud [n, 3] (x, y, intensity; float32) -> (status [n]: 0 binned, 1 dropped (a field is not finite), 2 out
    of range; ring [n], sector [n], v [n]: -1 / 0 where status is not 0). The rule of the header: counts, no transcendental."""
    p = params(p, **kw)
    nr, ns = int(p.n_rings), int(p.n_sectors)
    edge2, sdir = table if table is not None else layout(p)
    c = np.ascontiguousarray(cloud, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    x, y, w = c[:, 0], c[:, 1], c[:, 2]
    finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(w)
    with np.errstate(invalid="ignore", over="ignore"):
        r2 = x * x + y * y
        inside = finite & (r2 < edge2[nr])
        ring = np.count_nonzero(r2[:, None] >= edge2[None, 1:nr], axis=1)
        cross = (sdir[None, :, 0] * y[:, None] - sdir[None, :, 1] * x[:, None]) >= 0.0  # [n, ns]
        j = np.arange(ns)
        up = (j >= 1) & (2 * j < ns)
        low = 2 * j > ns
        upper = (y > 0.0) | ((y == 0.0) & (x >= 0.0))
        sector = np.where(upper, np.count_nonzero(cross[:, up], axis=1), np.count_nonzero((j >= 1) & (2 * j <= ns)) + np.count_nonzero(cross[:, low], axis=1))
        sector = np.where((x == 0.0) & (y == 0.0), 0, sector)
        v = np.clip(np.trunc(np.where(finite, w, 0.0)), 0.0, 255.0).astype(np.int64)
    status = np.where(finite, np.where(inside, 0, 2), 1)
    ok = status == 0
    return status, np.where(ok, ring, -1), np.where(ok, sector, -1), np.where(ok, v, 0)


def describe(cloud, p=None, table=None, **kw):
    """The descriptor of one cloud -> (bins uint32 [n_sectors, n_rings], ring_sums uint32 [n_rings], dropped)"""
    p = params(p, **kw)
    nr, ns = int(p.n_rings), int(p.n_sectors)
    c = np.ascontiguousarray(cloud, dtype=np.float32).reshape(-1, 3)
    if len(c) > capi.SC_MAX_POINTS:
        raise ValueError("describe: a cloud of %d points, at most %d are described" % (len(c), capi.SC_MAX_POINTS))
    status, ring, sector, v = bins_of_points(c, p, table)
    ok = status == 0
    flat = sector[ok] * nr + ring[ok]
    bins = np.zeros(ns * nr, dtype=np.int64)
    if int(p.value) == capi.SC_MAX:
        np.maximum.at(bins, flat, v[ok])
    elif int(p.value) == capi.SC_SUM:
        np.add.at(bins, flat, v[ok])
    elif int(p.value) == capi.SC_COUNT:
        np.add.at(bins, flat, 1)
    else:
        raise ValueError("describe: value %d" % int(p.value))
    bins = bins.reshape(ns, nr).astype(np.uint32)
    return bins, bins.sum(axis=0, dtype=np.uint32), int(np.count_nonzero(status == 1))


def key_distance(ring_sum_a, ring_sum_b):
    """K(a, b) = sum over rings of (ring_sum_a - ring_sum_b)^2, exact (Python integers below 2^64)"""
    d = np.asarray(ring_sum_a, dtype=np.int64) - np.asarray(ring_sum_b, dtype=np.int64)
    return int(np.sum(d * d))


def shift_distances(a, b):
    """d(s) for every shift s, float64 [n_sectors]: a, b bins [n_sectors, n_rings]; a is `to`, b is `from`"""
    A, Bm = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ns = A.shape[0]
    na, nb = np.sqrt(np.sum(A * A, axis=1)), np.sqrt(np.sum(Bm * Bm, axis=1))
    both = (na[:, None] > 0.0) & (nb[None, :] > 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        cos = np.where(both, (A @ Bm.T) / (na[:, None] * nb[None, :]), 0.0)  # [j of a, column of b]
    j = np.arange(ns)
    k = (j[None, :] + j[:, None]) % ns  # [shift, j] -> the column of b
    n = np.count_nonzero(both[j[None, :], k], axis=1)
    return np.where(n > 0, 1.0 - np.sum(cos[j[None, :], k], axis=1) / np.maximum(n, 1), 1.0)


def shift_yaw(shift, n_sectors):
    """the yaw of a shift in (-pi, pi]: theta_to ~ theta_from + yaw"""
    m = shift - n_sectors if 2 * shift > n_sectors else shift
    return float(m) * (2.0 * math.pi) / float(n_sectors)


def distance(a, b):
    """-> (distance, shift, yaw, margin): the smallest d(s), the smallest s that reaches it, its yaw, and how far the best OTHER shift lies
    above it (inf with one sector) - where that is below the device's rounding bound the device may name another shift"""
    d = shift_distances(a, b)
    s = int(np.argmin(d))  # (the first of equal minima)
    rest = np.delete(d, s)
    return float(d[s]), s, shift_yaw(s, len(d)), (float(rest.min() - d[s]) if len(rest) else math.inf)


def rounding_bound(p=None, **kw):
    """B = (n_rings + n_sectors + 8) * 2^-24: the first-order rounding bound of the float32 distance (dot, two norms, a division, the column sum)"""
    p = params(p, **kw)
    return (int(p.n_rings) + int(p.n_sectors) + 8) * 2.0 ** -24


def stage1(ring_sums, to, p):
    """the `from` stage 1 hands to stage 2 for `to`: [(K, from)] - the n_keys smallest K (ties: the smaller index), or every eligible one"""
    last = to - int(p.min_index_gap)
    if last < 0:
        return []
    rs = np.asarray(ring_sums, dtype=np.int64)
    d = rs[:last + 1] - rs[to]
    K = np.sum(d * d, axis=1)  # (below 2^54: exact in int64)
    order = np.argsort(K, kind="stable")  # ties: the smaller index
    if int(p.n_keys) > 0 and len(order) > int(p.n_keys):
        order = order[:int(p.n_keys)]
    return [(int(K[f]), int(f)) for f in order]


def candidates(bins, p=None, details=False, **kw):
    """The candidates of one set: bins uint32 [N, n_sectors, n_rings] in log order -> SC_CANDIDATE_DTYPE, `to` ascending then distance,
    `sequence` 0. details=True: (candidates, per `to` the list of (distance, from, shift, margin, K) of everything stage 2 looked at,
    ordered by (distance, from)) - what a comparison within a rounding bound needs."""
    p = params(p, **kw)
    bins = np.asarray(bins, dtype=np.uint32).reshape(-1, int(p.n_sectors), int(p.n_rings))
    ring_sums = bins.sum(axis=1, dtype=np.uint32)
    out, looked = [], []
    for to in range(len(bins)):
        found = []
        for K, f in stage1(ring_sums, to, p):
            d, s, yaw, margin = distance(bins[to], bins[f])
            found.append((d, f, s, margin, K))
        found.sort(key=lambda e: (e[0], e[1]))
        looked.append(found)
        for d, f, s, margin, K in [e for e in found if e[0] <= float(p.max_distance)][:int(p.max_per_node)]:
            out.append((0, to, f, s, d, shift_yaw(s, int(p.n_sectors)), K))
    arr = np.array(out, dtype=capi.SC_CANDIDATE_DTYPE) if out else np.zeros(0, dtype=capi.SC_CANDIDATE_DTYPE)
    return (arr, looked) if details else arr
