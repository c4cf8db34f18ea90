"""Case tables and images of tests/test_cfar_layout_gpu.py, with the conditions tests/test_cfar_shape_cpu.py asserts on them: plain numpy and
host/cfar_shape_check (the launch plan of csrc/cfar_shape.h without a GPU). The owner-layout detector (cfar_detect_owner_kernel, csrc/cfar.hip) keeps
a transposed prefix array in LDS: row rho of column padl + t holds P'[TB t + rho] for rho = rmin .. TB + rmax - 1, and window bound c of bin
TB t + e is read at (row e + cr[c], column padl + t + cq[c]). Everything that shapes the array is chosen per launch on the host, so the cases
here are DERIVED from the plan - which (guard, window) read which cells, which take which neighbour-copy count, which integer scale - and the CPU
test asserts that the derivation reaches what it is meant to reach."""
import functools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cfear_radarodometry_code_public_amd", "host")
RR = np.float32(0.0595238)
FIELDS = ("TB", "NW", "RS", "full", "sh", "kopen", "rmin", "rmax", "cr0", "cr1", "cr2", "cr3", "cq0", "cq1", "cq2", "cq3", "padl", "fill", "lds_bytes",
          "per_cu", "workgroups")
SHAPES = ((28, 2), (20, 3), (16, 4), (32, 4))
_PLANS = {}


def _check(args):
    subprocess.check_call(["make", "-C", HOST, "cfar_shape_check"], stdout=subprocess.DEVNULL)
    return subprocess.run([os.path.join(HOST, "cfar_shape_check")] + args, capture_output=True, text=True, check=True).stdout.splitlines()


def rate_text(rate):
    return "%.9g" % float(np.float32(rate))  # (round-trips a float32: the program parses it back to the same value)


def plans(queries, cus=256):
    """queries: (R, window, guard, rate) -> the plan dicts of host/cfar_shape_check, one run for all of them (memoised). cr / cq come as tuples,
    `workgroups` is that of a batch with more rows than the device holds workgroups"""
    todo = [q for q in dict.fromkeys((int(R), int(w), int(g), rate_text(r), int(cus)) for R, w, g, r in queries) if q not in _PLANS]
    for i in range(0, len(todo), 2000):
        part = todo[i:i + 2000]
        lines = _check([str(v) for q in part for v in q])
        assert len(lines) == len(part)
        for q, line in zip(part, lines):
            tok = line.split()
            assert tok[0] == "kernel" and len(tok) == 2 + len(FIELDS)
            d = dict(zip(FIELDS, (int(v) for v in tok[2:])))
            d["kernel"] = tok[1]
            d["cr"] = tuple(d.pop("cr%d" % c) for c in range(4))
            d["cq"] = tuple(d.pop("cq%d" % c) for c in range(4))
            _PLANS[q] = d
    return [_PLANS[(int(R), int(w), int(g), rate_text(r), int(cus))] for R, w, g, r in queries]


def plan(R, window, guard, rate=0.01, cus=256):
    return plans([(R, window, guard, rate)], cus)[0]


def same_plan(got, exp, rows):
    """a context's cfear_cfar_launch_plan (capi.Context.cfar_launch_plan) against the check program's for `rows` azimuth rows"""
    exp = dict(exp, workgroups=min(exp["workgroups"], rows))
    return all(got[k] == exp[k] for k in exp), (got, exp)


@functools.lru_cache(maxsize=None)
def reach(TB):
    """[65, 1000, 2] (rmin, rmax) of guard 0 .. 64, window 1 .. 1000 for TB bins per thread"""
    a = np.array([[int(v) for v in l.split()] for l in _check(["reach", str(TB)])])
    assert a.shape == (65 * 1000, 4)
    return a[:, 2:].reshape(65, 1000, 2)


def scaling(window, rate):
    """CFARFilter::getCAScalingFactor (cfar.cpp:12-16)"""
    N = float(2 * window)
    return N * (float(np.float32(rate)) ** (-1.0 / N) - 1.0)


# ---- the detector's definition (cfar.cpp:45-60) on one row, in double: what the sensitive images are built from --------------------------------

def bounds(b, R, guard, window):
    """indices into the row's prefix sum of the four window bounds of bin b as the owner-layout detector reads them (a bin below 0 reads 0, a bin
    from R on the row total): A, B = trailing window, C, D = forward window"""
    return [min(max(b + o, 0), R) for o in (-guard - window, -guard, guard, guard + window)]


def threshold(P, b, R, guard, window, scal, replace=None):
    """scaling * mean of bin b off the prefix sum P (int64 [R + 1]); replace = c: bound c reads the row total instead (what a lost neighbour copy
    gives). None: an empty window (the reference's mean is NaN: no detection); inf: a forward sum that went negative (it wraps to a huge u32)"""
    ix = bounds(b, R, guard, window)
    v = [int(P[i]) for i in ix]
    if replace is not None:
        v[replace] = int(P[R])
    tn, fn = ix[1] - ix[0], ix[3] - ix[2]
    if tn <= 0 or fn <= 0:
        return None
    ts, fs = v[1] - v[0], v[3] - v[2]
    if ts < 0 or fs < 0:
        return float("inf")
    return scal * ((ts / float(tn) + fs / float(fn)) / 2.0)


def decides(row, b, guard, window, scal, replace=None):
    P = np.concatenate([[0], np.cumsum(row.astype(np.int64) ** 2)])
    thr = threshold(P, b, len(row), guard, window, scal, replace)
    return thr is not None and float(int(row[b]) ** 2) > thr


def detect_rows(img, guard, window, rate, zmin, mind, maxd=400.0):
    """the detector's definition on a whole image -> boolean [A, R] (vectorised; exact sums, double arithmetic like oracle.cfar(prefix=True))"""
    A, R = img.shape
    scal = scaling(window, rate)
    P = np.concatenate([np.zeros((A, 1), dtype=np.int64), np.cumsum(img.astype(np.int64) ** 2, axis=1)], axis=1)
    i = np.arange(R)
    t0, t1, f0, f1 = np.maximum(0, i - guard - window), i - guard, i + guard, np.minimum(R, i + guard + window)
    tn, fn = (t1 - t0).astype(float), (f1 - f0).astype(float)
    ok = (t1 > t0) & (f1 > f0)
    t0c, t1c, f0c, f1c = (np.clip(x, 0, R) for x in (t0, t1, f0, f1))
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = ((P[:, t1c] - P[:, t0c]) / tn + (P[:, f1c] - P[:, f0c]) / fn) / 2.0
        hit = (img.astype(np.float64) ** 2 > scal * mean) & ok
    rng = np.float64(np.float32(RR)) * i
    gate = (rng > float(np.float32(mind))) & (rng < maxd)
    return hit & gate & (img.astype(np.float64) > float(np.float32(zmin)))


# ---- B.1: rows that nearly fill the workgroup ------------------------------------------------------------------------------------------

def near_full_rows(TB, NW):
    NT = 64 * NW
    return (TB * NT - 4, TB * NT - 8, TB * (NT - 1) + 4)


REQUIRED_PAIRS = {(28, 2): [(20, 10), (20, 1), (10, 40), (5, 70), (37, 10), (37, 70)], (32, 4): [(20, 70), (10, 300), (0, 150)]}  # (guard, window)
PAIR_POOL = {2: [(g, w) for g in (0, 5, 10, 20, 37) for w in (1, 10, 40, 70)], 3: [(g, w) for g in (0, 5, 10, 20, 37) for w in (1, 10, 40, 70)],
             4: [(g, w) for g in (0, 5, 10, 20, 37) for w in (1, 40, 70, 150, 300)]}
MAX_DISTANCE = {(32, 4): 600.0}  # rows beyond 400 m / 0.0595 m = 6720 bins: the range gate must reach the row's end, on both sides of the comparison
NEAR_FULL_RATE = 0.01


def at_risk(p, R, guard, window):
    """[(bin, bound c)] whose bound is read from the contested cells - rows below 0 of column padl + NT, which thread NT - 1's neighbour copies and
    the fill loop both write - at a place where the two values differ: the cell of row rho < 0 holds P'[TB NT + rho], which is the row total only
    from bin R on"""
    if p["kernel"] != "owner" or not p["fill"]:
        return []
    TB, NT = p["TB"], 64 * p["NW"]
    off = (-guard - window, -guard, guard, guard + window)
    out = []
    for c in range(4):
        t = NT - p["cq"][c]
        for e in range(TB):
            b = TB * t + e
            if 0 <= t < NT and b < R and e + p["cr"][c] < 0 and b + off[c] < R:
                assert b + off[c] == TB * NT + e + p["cr"][c] and p["rmin"] <= e + p["cr"][c]
                out.append((b, c))
    return sorted(out)


def near_full_pairs(TB, NW):
    """{R: [(guard, window)]}: the required pairs of the shape and every pair of the pool whose plan at R reads the contested cells"""
    res = {}
    for R in near_full_rows(TB, NW):
        pool = REQUIRED_PAIRS.get((TB, NW), []) + [q for q in PAIR_POOL[NW] if q not in REQUIRED_PAIRS.get((TB, NW), [])]
        ps = plans([(R, w, g, NEAR_FULL_RATE) for g, w in pool])
        res[R] = [q for q, p in zip(pool, ps) if (p["TB"], p["NW"]) == (TB, NW) and (q in REQUIRED_PAIRS.get((TB, NW), []) or at_risk(p, R, *q))]
    return res


def random_hot_tail(R, TB, A, seed):
    """random bytes whose last 2 TB bins are >= 200: the even rows over the whole byte range (next to no detections outside the tail), the odd
    rows a low floor under a comb (detections everywhere)"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(A, R), dtype=np.uint8)
    img[1::2] = rng.integers(0, 48, size=img[1::2].shape, dtype=np.uint8)
    img[1::2, ::9] += rng.integers(90, 200, size=img[1::2, ::9].shape, dtype=np.uint8)
    img[:, -2 * TB:] = np.maximum(img[:, -2 * TB:], 200)
    return img


NEAR_FULL_GATE = dict(zmin=5.0, mind=2.5)


def sensitive_image(p, R, guard, window, direction, A=64, rate=NEAR_FULL_RATE):
    """An image that tells the two store orders apart, built from the detector's definition: row a carries one at-risk (bin, bound) - they take
    turns - over a flat floor, hot bytes from the bound's bin to the row's end (so that the prefix value there is not the row total), and at the
    bin a byte strictly between the true threshold and the threshold with that one bound replaced by the row total. direction "false": the
    forward sum is lost (a detection the reference does not make); "missed": it is inflated (a detection that goes missing).
    -> (image [A, R], [(bin, bound)] per row) or None when no at-risk bin of the case can be driven that way"""
    scal = scaling(window, rate)
    off = (-guard - window, -guard, guard, guard + window)
    rows = []
    for b, c in at_risk(p, R, guard, window):
        found = None
        for floor in (30, 10, 60, 3):
            for hot in (250, 120, 60, 20):
                row = np.full(R, floor, dtype=np.uint8)
                row[b + off[c]:] = hot
                row[b] = 0
                P0 = np.concatenate([[0], np.cumsum(row.astype(np.int64) ** 2)])
                vs = np.arange(8, 256, dtype=np.int64)
                ix = bounds(b, R, guard, window)
                tn, fn = ix[1] - ix[0], ix[3] - ix[2]
                if tn <= 0 or fn <= 0:
                    continue
                val = [P0[i] + (vs * vs if i > b else 0) for i in ix]   # the four bounds' prefix values with byte v at the bin, per v
                tot = P0[R] + vs * vs

                def thr(v4):
                    ts, fs = v4[1] - v4[0], v4[3] - v4[2]
                    return np.where((ts < 0) | (fs < 0), np.inf, scal * ((ts / float(tn) + fs / float(fn)) / 2.0))
                true = (vs * vs).astype(np.float64) > thr(val)
                wrong = (vs * vs).astype(np.float64) > thr([tot if k == c else val[k] for k in range(4)])
                ok = [int(v) for v in vs[(wrong & ~true) if direction == "false" else (true & ~wrong)]]
                if ok:
                    row[b] = ok[len(ok) // 2]
                    found = row.copy()
                    break
            if found is not None:
                break
        if found is not None:
            rows.append((found, (b, c)))
    if not rows:
        return None
    img = np.stack([rows[a % len(rows)][0] for a in range(A)])
    return img, [rows[a % len(rows)][1] for a in range(A)]


def sensitive_row_differs(row, guard, window, rate, risks):
    """the CPU condition: some at-risk (bin, bound) of the row is decided differently by the two thresholds"""
    scal = scaling(window, rate)
    return any(decides(row, b, guard, window, scal) != decides(row, b, guard, window, scal, c) for b, c in risks)


def edge_rows(TB, NW):
    """R = TB (NT - 1): FULL with thread NT - 1 holding no bytes; R = TB NT: the next shape"""
    return TB * (64 * NW - 1), TB * 64 * NW


# ---- B.2: every neighbour-copy count ---------------------------------------------------------------------------------------------------

COPY_ROWS = {28: (3360, 3364), 20: (3600, 3768), 16: (3904, 3900), 32: (6016, 6000)}  # (FULL, not FULL) row length per bins-per-thread


def copy_reachable(TB):
    """(rmax values, -rmin values, {(guard, window): (rmin, rmax)}) the owner-layout detector can take with TB bins per thread at COPY_ROWS[TB][0], over
    guard 0 .. 64 and window 1 .. 1000: the configurations whose plan there is that shape"""
    R = COPY_ROWS[TB][0]
    tab = reach(TB)
    q = [(g, w) for g in range(65) for w in range(1, 1001)]
    ps = plans([(R, w, g, 0.01) for g, w in q])
    ok = {k: (int(tab[k[0], k[1] - 1, 0]), int(tab[k[0], k[1] - 1, 1])) for k, p in zip(q, ps) if p["kernel"] == "owner" and p["TB"] == TB}
    for k, p in zip(q, ps):
        if k in ok:
            assert (p["rmin"], p["rmax"]) == ok[k]
    return sorted({v[1] for v in ok.values()}), sorted({-v[0] for v in ok.values()}), ok


@functools.lru_cache(maxsize=None)
def copy_pairs(TB):
    """a (guard, window) set that takes every rmax and every -rmin the shape can (greedy cover off the offsets' table, short reaches first, a
    pair kept only if its plan at COPY_ROWS[TB] is that shape; deterministic) -> [(guard, window, rmin, rmax)]"""
    tab = reach(TB)
    seen, chosen = set(), []
    for g, w in sorted(((g, w) for g in range(65) for w in range(1, 1001)), key=lambda k: (k[0] + k[1], k)):
        rmin, rmax = int(tab[g, w - 1, 0]), int(tab[g, w - 1, 1])
        new = {("hi", rmax), ("lo", -rmin)} - seen
        if new and all(p["kernel"] == "owner" and p["TB"] == TB for p in plans([(R, w, g, 0.01) for R in COPY_ROWS[TB]])):
            chosen.append((g, w, rmin, rmax))
            seen |= new
    return chosen


def comb_image(R, TB, A, seed):
    """random bytes (a low floor) with a comb: the bins either side of every thread boundary raised, so that they are candidates"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 64, size=(A, R), dtype=np.uint8)
    e = np.arange(R) % TB
    for a in range(A):
        sel = (e == (0, 1, TB - 1, TB - 2)[a % 4]) & ((np.arange(R) // TB) % 2 == (a // 4) % 2)
        img[a, sel] = np.minimum(img[a, sel].astype(int) + 130, 255).astype(np.uint8)
    return img


# ---- B.3: every integer scale -----------------------------------------------------------------------------------------------------------

SCALE_R, SCALE_GUARD = 3360, 2
SCALE_WINDOWS = (1, 2, 3, 5, 10, 20, 40, 70, 100, 150, 250, 300, 500, 700, 900, 1000)
SCALE_RATES = (0.99, 0.9, 0.7, 0.5, 0.3, 0.1, 0.03, 0.01, 0.001, 3e-4, 2.4e-4, 1e-4, 1e-6, 1e-9)
NO_SCALE_DETECTOR = (1, 1e-4)  # (window, rate): no usable integer scale - the round-5 kernels run


@functools.lru_cache(maxsize=None)
def scale_detectors():
    """[(window, rate, sh, kopen)]: per integer scale the search finds one detector (the shortest window), and the detectors with the smallest
    and the largest kopen - all at SCALE_R bins and SCALE_GUARD guard cells, where the owner-layout detector takes them"""
    q = [(w, r) for w in SCALE_WINDOWS for r in SCALE_RATES]
    ps = plans([(SCALE_R, w, SCALE_GUARD, r) for w, r in q])
    own = [(w, r, p["sh"], p["kopen"]) for (w, r), p in zip(q, ps) if p["kernel"] == "owner"]
    out = []
    for sh in sorted({d[2] for d in own}):
        out.append(min((d for d in own if d[2] == sh), key=lambda d: (d[0], -d[1])))
    for d in (min(own, key=lambda d: (d[3], d[0])), max(own, key=lambda d: (d[3], -d[0]))):
        if d not in out:
            out.append(d)
    return out


def near_ties(window, rate, keep=3):
    """Byte v over a two-level floor (n_a bins of a, window - n_a of b, in both windows): the combinations whose v^2 / (scaling * mean) is closest
    to 1 from above (a detection) and from below or at 1 (none), evaluated with the reference's expressions in double.
    -> ([(ratio - 1, v, a, b, n_a)] above, [...] below), nearest first"""
    scal = scaling(window, rate)
    v = np.arange(1, 256, dtype=np.int64)[:, None, None]
    a = np.arange(0, 256, dtype=np.int64)[None, :, None]
    b = a + np.arange(1, 9, dtype=np.int64)[None, None, :]
    target = v * v * window / scal                      # the window sum at which v^2 equals the threshold
    with np.errstate(divide="ignore", invalid="ignore"):
        na0 = np.floor((target - window * b * b) / (a * a - b * b))
    cands = []
    for d in (0, 1):
        na = np.clip(na0 + d, 0, window).astype(np.int64)
        S = na * a * a + (window - na) * b * b
        S = np.where(b <= 255, S, 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = (v * v).astype(np.float64) / (scal * ((S / float(window) + S / float(window)) / 2.0))
        cands.append((ratio, na))
    above, below = [], []
    for ratio, na in cands:
        r = np.where(np.isfinite(ratio), ratio, 0.0)
        for lst, mask, key in ((above, r > 1.0, r), (below, (r <= 1.0) & (r > 0.5), -r)):
            flat = np.where(mask.ravel(), key.ravel(), np.inf)
            for i in np.argsort(flat, kind="stable")[:keep]:
                if np.isfinite(flat[i]):
                    vi, ai, bi = np.unravel_index(i, mask.shape)
                    lst.append((float(r[vi, ai, bi]) - 1.0, int(vi) + 1, int(ai), int(ai) + int(bi) + 1, int(na[vi, ai, bi])))
    key = lambda t: (abs(t[0]), t[1:])
    return sorted(set(above), key=key)[:keep], sorted(set(below), key=key)[:keep]


def tie_image(R, window, guard, rate, A=8):
    """rows of near ties, above and below taking turns, each with whole trailing and forward windows
    -> (image, closest distance above, closest distance below (<= 0), sites per row)"""
    above, below = near_ties(window, rate)
    span = 2 * (guard + window) + 1
    sites = max(1, min(8, (R - 64) // span))
    assert span <= R - 64
    img = np.zeros((A, R), dtype=np.uint8)
    for r in range(A):
        for s in range(sites):
            lst = above if (r + s) % 2 == 0 else below
            _, v, a, b, na = lst[(r // 2 + s // 2) % len(lst)]
            i = 60 + s * span + guard + window   # the bin: past the range gate's start, its trailing window whole
            lo = i - guard - window
            img[r, lo:lo + span] = b
            img[r, lo:lo + na] = a
            img[r, i + guard:i + guard + na] = a
            img[r, i] = v
        img[r, 60 + sites * span:] = img[r, 60 + sites * span - 1]
    return img, (above[0][0] if above else None), (below[0][0] if below else None), sites


# ---- B.4: the widest arrays and the way out -----------------------------------------------------------------------------------------------

WIDEST = [(4092, 10, 500, 1e-4), (4080, 10, 500, 1e-4), (8000, 64, 1000, 0.01), (8004, 64, 1000, 0.01)]  # (R, guard, window, rate): RS = 64 NW + 128
BIG_LDS = [(6016, 43, 982, 0.01), (6020, 43, 982, 0.01), (8188, 38, 999, 0.01)]  # LDS above 64 KB, the attribute path: only the {32,4} shape gets there


def just_past_columns(R, guard=64, rate=0.01):
    """the shortest window (guard 64) whose columns no instantiation holds at R bins -> (window, its plan, the plan of window - 1)"""
    ws = list(range(200, 2001))
    ps = plans([(R, w, guard, rate) for w in ws])
    for w, p, prev in zip(ws[1:], ps[1:], ps[:-1]):
        if p["kernel"] != "owner":
            return w, p, prev
    raise AssertionError("every window fits")


# ---- B.5: candidate and record counts -----------------------------------------------------------------------------------------------------

SPIKE_COUNTS = (7, 8, 9, 60, 61, 62, 63, 64, 65, 66, 67, 68)
SPIKE_CASES = [(3360, 0), (3768, 1), (6000, 2)]  # (R, the wave whose bins carry the spikes)
SPIKE_DETECTOR = dict(window=10, guard=2, pfa=0.01, zmin=20.0, mind=2.5)  # (short reach: a spike stays out of its neighbours' windows)


def spike_image(R, TB, wave, seed):
    """per count n a row of n isolated spikes over a flat non-zero floor, all in `wave`'s bins, the other waves quiet; between them empty rows and
    rows of clutter -> (image, {row: n})"""
    rng = np.random.default_rng(seed)
    lo = max(wave * 64 * TB, 100)
    step = (min(R, (wave + 1) * 64 * TB) - lo - 20) // max(SPIKE_COUNTS)
    assert step > SPIKE_DETECTOR["window"] + SPIKE_DETECTOR["guard"] and lo + step * max(SPIKE_COUNTS) < min(R, (wave + 1) * 64 * TB)
    rows, counts = [], {}
    for k, n in enumerate(SPIKE_COUNTS):
        row = np.full(R, 12, dtype=np.uint8)
        row[lo + step * np.arange(n)] = 200 + (rng.integers(0, 50, size=n)).astype(np.uint8)
        counts[len(rows)] = n
        rows.append(row)
        if k % 2 == 0:
            rows.append(np.zeros(R, dtype=np.uint8))
        else:
            clutter = rng.integers(0, 12, size=R, dtype=np.uint8)
            clutter[::8] = 255
            rows.append(clutter)
    return np.stack(rows), counts


# ---- B.6: trips of the persistent workgroups --------------------------------------------------------------------------------------------------

TRIP_R, TRIP_K = 776, (1, 3, 4, 6)


def trip_rows(W):
    return [k * W + d for k in TRIP_K for d in (-1, 0, 1)]


def trip_pool(n_rows, seed=776):
    """n_rows distinct random rows of TRIP_R bins (one-row images), a comb on top so that every row has detections"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 64, size=(n_rows, TRIP_R), dtype=np.uint8)
    img[:, 50::37] += rng.integers(60, 190, size=img[:, 50::37].shape, dtype=np.uint8)
    return img
