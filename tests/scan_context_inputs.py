"""Seeded inputs of the Scan-Context tests (test_scan_context_cpu.py, test_scan_context_gpu.py) and the rule by which a device result is
compared with the numpy twin (cfear_radarodometry_code_public_amd/scancontext.py) where a float32 distance decides something.

The rule: B = (n_rings + n_sectors + 8) * 2^-24 bounds the device's distance error. A decision the twin takes with a margin above 2 B - which
shift is the best, which candidates are the max_per_node best, whether a distance is below max_distance - must come out the same on the
device; where the margin is smaller either answer is accepted. At most 5 % of the decisions of these inputs may be of the second kind:
test_scan_context_cpu.py asserts that on the twin alone."""
import math

import numpy as np

from cfear_radarodometry_code_public_amd import capi, scancontext as sc

SHAPES = [(1, 1), (20, 60), (20, 40), (40, 120), (3, 7), (20, 64), (20, 65)]  # (n_rings, n_sectors)
CLOUD_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 4800, 65536]
SET_SIZES = [0, 1, 2, 63, 64, 65, 257]
MAX_RANGE = 80.0
_C = {}


def random_cloud(n, seed, spread=90.0):
    """n points in a square that reaches past max_range, intensities past both ends of 0 .. 255 and fractional"""
    rng = np.random.default_rng(seed)
    c = np.empty((n, 3), dtype=np.float32)
    c[:, :2] = rng.uniform(-spread, spread, (n, 2))
    c[:, 2] = rng.uniform(-20.0, 300.0, n)
    return c


def special_cloud(n_rings, n_sectors):
    """the points a bin rule gets wrong first: the origin, negative zeros, exactly on max_range, on every sector boundary of the layout table
    at several radii (and one float32 step to either side), on the ring edges, NaN / inf fields, intensities below 0, above 255, fractional"""
    edge2, sdir = sc.layout(n_rings=n_rings, n_sectors=n_sectors, max_range=MAX_RANGE)
    pts = [(0.0, 0.0, 9.0), (-0.0, -0.0, 9.5), (0.0, -0.0, 3.0), (-0.0, 0.0, 3.0), (1.0, -0.0, 7.0), (-1.0, -0.0, 7.0), (-1.0, 0.0, 7.0),
           (MAX_RANGE, 0.0, 5.0), (0.0, -MAX_RANGE, 5.0), (-MAX_RANGE, 0.0, 5.0), (np.nextafter(np.float32(MAX_RANGE), np.float32(0)), 0.0, 5.0),
           (np.nan, 1.0, 5.0), (1.0, np.nan, 5.0), (1.0, 1.0, np.nan), (np.inf, 1.0, 5.0), (1.0, -np.inf, 5.0), (1.0, 1.0, np.inf), (1.0, 1.0, -np.inf),
           (2.0, 1.0, -5.0), (2.0, 1.0, -0.5), (2.0, 1.0, 0.99), (2.0, 1.0, 254.5), (2.0, 1.0, 255.0), (2.0, 1.0, 255.5), (2.0, 1.0, 1e9), (2.0, 1.0, 100.75)]
    for radius in (0.5, 3.999, 17.3, 40.0, 79.9):
        for c, s in sdir:
            x, y = np.float32(radius * c), np.float32(radius * s)
            pts.append((x, y, 50.0 + radius))
            pts.append((np.nextafter(x, np.float32(np.inf)), np.nextafter(y, np.float32(-np.inf)), 60.0))
            pts.append((np.nextafter(x, np.float32(-np.inf)), np.nextafter(y, np.float32(np.inf)), 70.0))
    for e2 in edge2:
        e = math.sqrt(e2)
        pts += [(e, 0.0, 11.0), (0.0, e, 12.0), (-e * 0.6, e * 0.8, 13.0), (np.nextafter(np.float32(e), np.float32(0)), 0.0, 14.0)]
    return np.array(pts, dtype=np.float32)


def grid_cloud(n_azimuths=400, range_res=0.0438, every=37):
    """points on the azimuth grid of a 400-row sweep (azimuth 2 pi k / 400, range a multiple of the range resolution), as float32: with 40
    or 60 sectors every 10th or 20th row lies on a sector boundary and the rounding of x, y decides its side"""
    k = np.repeat(np.arange(n_azimuths), 8)
    r = (np.tile(np.arange(8), n_azimuths) * every * 5 + 60 + k % 7) * range_res
    t = 2.0 * np.pi * k / n_azimuths
    return np.stack([(r * np.cos(t)).astype(np.float32), (r * np.sin(t)).astype(np.float32), np.full(len(k), 80.0, dtype=np.float32)], axis=1)


def random_descriptor(n_rings, n_sectors, rng, fill=0.3, top=256):
    return ((rng.random((n_sectors, n_rings)) < fill) * rng.integers(1, top, (n_sectors, n_rings))).astype(np.uint32)


def distance_pairs(n_rings, n_sectors, n_pairs=40):
    """pairs (a, b) for the distance test: random 30 %-filled descriptors, bins up to 255 (the max kind) and up to 2^24 (the sum kind), a
    third of the pairs related (b a shifted, perturbed copy of a: small distances, where a mean cosine near 1 is subtracted from 1)"""
    key = ("pairs", n_rings, n_sectors, n_pairs)
    if key not in _C:
        rng = np.random.default_rng(1000 * n_rings + n_sectors)
        fill = 0.3 if n_rings * n_sectors >= 100 else 0.7  # (a handful of bins: at 30 % whole columns are empty and shifts tie)
        out = []
        for i in range(n_pairs):
            top = 256 if i % 2 == 0 else 1 << 24
            a = random_descriptor(n_rings, n_sectors, rng, fill, top)
            if i % 3 == 0:
                b = np.roll(a, int(rng.integers(0, n_sectors)), axis=0).copy()
                flip = rng.random(b.shape) < 0.1
                b[flip] = random_descriptor(n_rings, n_sectors, rng, fill, top)[flip]
            else:
                b = random_descriptor(n_rings, n_sectors, rng, fill, top)
            out.append((a, b))
        _C[key] = out
    return _C[key]


def place_set(n, n_rings, n_sectors, seed, places=9, noise=0.08):
    """a set of n descriptors that revisits `places` places in turn: descriptor i is place i % places, seen under a random heading (its columns
    rolled) with a fraction `noise` of its bins replaced - so i matches i - places, i - 2 places, ... at distances that differ by the noise"""
    rng = np.random.default_rng(seed)
    base = [random_descriptor(n_rings, n_sectors, rng) for _ in range(places)]
    out = np.zeros((n, n_sectors, n_rings), dtype=np.uint32)
    for i in range(n):
        d = np.roll(base[i % places], int(rng.integers(0, n_sectors)), axis=0).copy()
        flip = rng.random(d.shape) < noise
        d[flip] = random_descriptor(n_rings, n_sectors, rng)[flip]
        out[i] = d
    return out


def sets_of(n_rings=20, n_sectors=60, sizes=SET_SIZES, seed=5):
    """one place_set per size"""
    key = ("sets", n_rings, n_sectors, tuple(sizes), seed)
    if key not in _C:
        _C[key] = [place_set(n, n_rings, n_sectors, seed * 100 + k) for k, n in enumerate(sizes)]
    return _C[key]


def twin_candidates(sets, p):
    """scancontext.candidates of every set, once per process -> [(candidates, looked)] ; p's fields are the key"""
    key = ("twin", tuple(id(s) for s in sets), bytes(p))
    if key not in _C:
        _C[key] = [sc.candidates(s, p, details=True) for s in sets]
    return _C[key]


def decisions(looked_to, p):
    """What the twin decided for one `to` - looked_to: scancontext.candidates' details, (distance, from, shift, margin, K) ordered by
    (distance, from) - and which of it stands above the rounding bound -> (chosen: the entries handed back, list_firm: the choice of these
    entries and their order holds on the device, shift_firm [len(chosen)]: so does every one's shift)"""
    B2 = 2.0 * sc.rounding_bound(p)
    mp, md = int(p.max_per_node), float(p.max_distance)
    chosen = [e for e in looked_to if e[0] <= md][:mp]
    firm = all(abs(e[0] - md) > B2 for e in looked_to)  # nobody sits on the threshold
    upto = min(len(chosen) + 1, len(looked_to))          # the order among the chosen, and against the first one left out
    firm = firm and all(looked_to[i + 1][0] - looked_to[i][0] > B2 for i in range(upto - 1))
    return chosen, firm, [e[3] > B2 for e in chosen]


def soft_fraction(results, p):
    """the share of the twin's decisions (a list per `to` with something eligible, a shift per candidate) that do not stand above 2 B"""
    total = soft = 0
    for cand, looked in results:
        for lt in looked:
            if not lt:
                continue
            chosen, firm, shifts = decisions(lt, p)
            total += 1 + len(shifts)
            soft += (0 if firm else 1) + sum(0 if s else 1 for s in shifts)
    return soft / max(total, 1), total


def compare_candidates(got, results, p, tag):
    """device candidates `got` (SC_CANDIDATE_DTYPE of the sets in `results`' order) against the twin under the rule above. Always: every
    record is a pair stage 1 handed on, its key distance exact, its distance within B of the twin's, its yaw its shift's; the records of a
    `to` ascend in (distance, from). Where the twin's decision is firm: the same `from` in the same order, the same shifts.
    -> (worst distance error / B, decisions, soft ones)"""
    B = sc.rounding_bound(p)
    worst, total, soft = 0.0, 0, 0
    assert list(got["sequence"]) == sorted(got["sequence"]), tag
    for g, (cand, looked) in enumerate(results):
        mine = got[got["sequence"] == g]
        assert list(mine["to"]) == sorted(mine["to"]), (tag, g)
        for to, lt in enumerate(looked):
            rows = mine[mine["to"] == to]
            by_from = {e[1]: e for e in lt}
            assert len(rows) <= int(p.max_per_node), (tag, g, to)
            for r in rows:
                assert int(r["from"]) in by_from, (tag, g, to, int(r["from"]), "not among the pairs stage 1 hands on")
                d, f, s, margin, K = by_from[int(r["from"])]
                assert int(r["key_distance"]) == K, (tag, g, to, f)
                err = abs(float(r["distance"]) - d)
                worst = max(worst, err / B)
                assert err <= B, (tag, g, to, f, float(r["distance"]), d, err / B)
                assert float(r["distance"]) <= float(p.max_distance), (tag, g, to, f)
                assert r["yaw"] == sc.shift_yaw(int(r["shift"]), int(p.n_sectors)), (tag, g, to, f)
            keys = [(float(r["distance"]), int(r["from"])) for r in rows]
            assert keys == sorted(keys), (tag, g, to)
            if not lt:
                continue
            chosen, firm, shifts = decisions(lt, p)
            total += 1 + len(shifts)
            soft += (0 if firm else 1) + sum(0 if s else 1 for s in shifts)
            if firm:
                assert [int(r["from"]) for r in rows] == [e[1] for e in chosen], (tag, g, to)
                for r, e, sf in zip(rows, chosen, shifts):
                    if sf:
                        assert int(r["shift"]) == e[2], (tag, g, to, e[1])
    return worst, total, soft


def ringed_cloud(n, n_rings, n_sectors, seed):
    """n points well inside their bins (no nearer than a tenth of a bin to any edge): a rotation by whole sector widths moves every point to
    the same ring and the sector that many further on, whatever the rounding -> (cloud float32 [n, 3], the sector and ring of every point)"""
    rng = np.random.default_rng(seed)
    sector, ring = rng.integers(0, n_sectors, n), rng.integers(0, n_rings, n)
    t = 2.0 * np.pi * (sector + rng.uniform(0.1, 0.9, n)) / n_sectors
    r = MAX_RANGE * (ring + rng.uniform(0.1, 0.9, n)) / n_rings
    c = np.stack([r * np.cos(t), r * np.sin(t), rng.integers(1, 256, n).astype(np.float64)], axis=1)
    return c.astype(np.float32), sector, ring


def rotated(cloud, angle):
    c, s = math.cos(angle), math.sin(angle)
    src = np.asarray(cloud, dtype=np.float64)
    out = src.copy()
    out[:, 0], out[:, 1] = c * src[:, 0] - s * src[:, 1], s * src[:, 0] + c * src[:, 1]
    return out.astype(np.float32)


# the candidate cases of the device tests: (name, n_rings, n_sectors, set sizes, ScParams fields). Every set is a place_set.
MATCH_CASES = [
    ("default", 20, 60, SET_SIZES, dict()),
    ("sixteen per node", 20, 60, [65, 12], dict(max_per_node=16, max_distance=1.0)),
    ("exhaustive", 20, 60, [64, 70, 2], dict(n_keys=0)),
    ("40 x 120", 40, 120, [0, 3, 70], dict(n_keys=5)),
    ("64 sectors", 20, 64, [40], dict()),
    ("65 sectors", 20, 65, [40], dict()),
    ("40 sectors, gap 1", 20, 40, [40], dict(min_index_gap=1)),
]


def match_case(name):
    """-> (sets, params, the twin's results) of a case, once per process"""
    key = ("case", name)
    if key not in _C:
        k = [c[0] for c in MATCH_CASES].index(name)
        _, nr, ns, sizes, kw = MATCH_CASES[k]
        sets = sets_of(nr, ns, sizes, seed=5 + k)
        p = capi.sc_params(n_rings=nr, n_sectors=ns, max_range=MAX_RANGE, **kw)
        _C[key] = (sets, p, twin_candidates(sets, p))
    return _C[key]
