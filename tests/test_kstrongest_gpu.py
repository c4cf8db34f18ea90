"""GPU parity: HIP k-strongest + peaks (through the C ABI) vs the CPU oracle, bit-exact.

Reference behaviour: radar_filters.cpp:209-298."""
import numpy as np
import pytest

from cfear_radarodometry_code_public_amd import capi, synth

pytestmark = pytest.mark.gpu


def run_case(oracle, img, k, z_min):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    if img.ndim == 2:
        img = img[None]
    n, A, R = img.shape
    p = capi.default_params(k_strongest=k, z_min=float(z_min))
    ctx = capi.Context(p, A, R)
    got = ctx.kstrongest_host(img)
    ctx.close()
    for s in range(n):
        exp = oracle.filter_polar(img[s], z_min, k)
        if not np.array_equal(got[s], exp):
            bad = np.argwhere(got[s] != exp)
            b = bad[0][0]
            raise AssertionError("scan %d row %d differs (A=%d R=%d k=%d zmin=%d)\n got %s\n exp %s" % (
                s, b, A, R, k, z_min, [hex(x) for x in got[s][b]], [hex(x) for x in exp[b]]))


@pytest.mark.parametrize("A,R", [(400, 3360), (400, 3768), (8, 64), (5, 37), (16, 100), (3, 4000), (7, 1)])
@pytest.mark.parametrize("k", [12, 1, 40])
def test_uniform_random(oracle, A, R, k):
    rng = np.random.default_rng(A * 7919 + R * 13 + k)
    run_case(oracle, rng.integers(0, 256, size=(A, R), dtype=np.uint8), k, 60)


@pytest.mark.parametrize("R", [3360, 3768, 333])
def test_heavy_ties(oracle, R):
    run_case(oracle, synth.ties_scan(64, R, seed=3), 12, 60)
    run_case(oracle, synth.ties_scan(64, R, seed=4, levels=(60, 61)), 12, 60)
    run_case(oracle, synth.ties_scan(64, R, seed=5, levels=(10, 200), p=[0.999, 0.001]), 12, 60)
    run_case(oracle, synth.ties_scan(64, R, seed=6, levels=(10, 200), p=[0.97, 0.03]), 40, 60)


@pytest.mark.parametrize("val", [0, 59, 60, 255])
@pytest.mark.parametrize("z_min", [0, 60, 255])
def test_constant_rows(oracle, val, z_min):
    run_case(oracle, np.full((6, 3360), val, dtype=np.uint8), 12, z_min)
    run_case(oracle, np.full((6, 3768), val, dtype=np.uint8), 64, z_min)


def test_zmin_zero_sparse(oracle):
    rng = np.random.default_rng(5)
    img = np.zeros((32, 3360), dtype=np.uint8)
    for b in range(32):
        n = b % 15  # fewer than k non-zero bins on some rows -> zero-valued bins must fill up
        img[b, rng.integers(0, 3360, n)] = rng.integers(1, 256, n)
    run_case(oracle, img, 12, 0)
    run_case(oracle, img, 12, 1)
    run_case(oracle, img[:, :9], 12, 0)  # R < k


def test_world_scan(oracle):
    w = synth.World(1234)
    run_case(oracle, synth.world_scan(w, 3, seed=1), 12, 60)
    run_case(oracle, synth.world_scan(w, 4, R=3768, range_res=np.float32(0.0438), seed=2), 40, 55)


def test_batch_isolation_and_halo(oracle):
    """Peaks windows read across row boundaries inside a scan but never across scans."""
    rng = np.random.default_rng(11)
    imgs = rng.integers(0, 256, size=(5, 24, 3360), dtype=np.uint8)
    # strong returns at both ends of every row: exercises the m<3 / m>=R-3 map-default branch
    imgs[:, :, :7] = rng.integers(200, 256, size=(5, 24, 7))
    imgs[:, :, -7:] = rng.integers(200, 256, size=(5, 24, 7))
    run_case(oracle, imgs, 12, 60)
    run_case(oracle, imgs[:, :, :3000], 40, 60)


@pytest.mark.parametrize("R", [5000, 8100, 9000, 16000])
def test_long_rows(oracle, R):
    rng = np.random.default_rng(R)
    run_case(oracle, rng.integers(0, 256, size=(9, R), dtype=np.uint8), 12, 60)
    run_case(oracle, synth.ties_scan(9, R, seed=R), 12, 60)


def test_k64_and_threshold_edges(oracle):
    rng = np.random.default_rng(64)
    img = rng.integers(0, 256, size=(40, 3360), dtype=np.uint8)
    run_case(oracle, img, 64, 60)
    run_case(oracle, img, 12, 255)
    run_case(oracle, img, 12, 254)
    run_case(oracle, img, 12, 128)
    run_case(oracle, img, 12, 127)
    run_case(oracle, np.minimum(img, 130), 12, 60)


def test_unsupported_sizes_fail_loudly(hip_lib):
    with pytest.raises(capi.CfearError):
        capi.Context(capi.default_params(k_strongest=65), 4, 100)
    with pytest.raises(capi.CfearError):
        capi.Context(capi.default_params(), 4, 20000)


def row_end_image(rng, A, R):
    """Rows whose strongest returns sit in the first / last nine bins, in every mix of edge and interior positions"""
    img = rng.integers(0, 50, size=(A, R), dtype=np.uint8)
    for a in range(A):
        ends = []
        if a % 3 != 1:
            ends.append(0)
        if a % 3 != 0:
            ends.append(R - 9)
        for e0 in ends:
            span = min(9, R - e0) if e0 else min(9, R)
            n = int(rng.integers(1, span + 1))
            pos = e0 + rng.choice(span, size=n, replace=False)
            pos = pos[(pos >= 0) & (pos < R)]
            img[a, pos] = rng.integers(120, 256, size=len(pos)) if a % 2 else 200  # distinct intensities / ties
    return img


@pytest.mark.parametrize("R", [3360, 333, 40, 25, 24, 23, 16, 13])
@pytest.mark.parametrize("k", [12, 3])
def test_kept_points_at_the_row_ends(oracle, R, k):
    """AxialNonMaxSupress at the ends of a row (radar_filters.cpp:251-276): a kept point within three bins of an end only sees the
    scores that interior kept points within six bins of that end put into the map; everything else reads as 0. Rows whose strongest
    returns sit in the first / last nine bins in every mix of edge and interior positions (R >= 24: the marked-bits path of the
    kernel, shorter rows: its plain loop)."""
    rng = np.random.default_rng(R * 31 + k)
    img = row_end_image(rng, 96, R)
    run_case(oracle, img, k, 60)


# ---- waves that walk several rows ----------------------------------------------------------------------------------------------------------
# cfear_launch_kstrongest gives a wave r = min(cap, ceil(n_rows / (1024 * occupancy))) consecutive rows (include/cfear_hip.h at
# cfear_kstrongest_launch_shape); the wave carries the selection threshold (Tprev) and its place in the scan from row to row. Every case above
# has at most 2000 rows: one row per wave, a fresh threshold, no scan boundary inside a wave. The cases below reach r rows with many tiny
# scans (n_rows > (r - 1) * 1024 * occupancy), assert the r they meant through the read-back and then compare bit for bit with the oracle.

# (n_scans, occupancy knob, rows knob, rows per wave) at A = 7 (and any R up to 4069): n_rows = 7 n in ((r - 1) * 1024 * occ, r * 1024 * occ],
# and no multiple of 4 r: the last wave and the last workgroup are partial. 7 against 5 or 8 rows puts the scan wrap at every phase of a wave.
A7_OCC5 = [(733, 5, 8, 2), (1465, 5, 8, 3), (2927, 5, 8, 5), (5123, 5, 8, 8)]
A7_OCC67 = [(879, 6, 8, 2), (1757, 6, 8, 3), (3511, 6, 8, 5), (1025, 7, 8, 2), (2049, 7, 8, 3), (4097, 7, 8, 5)]
A7 = A7_OCC5 + A7_OCC67
# (At R = 37 a row never has more than 40 candidates, so the carried threshold never leaves the floor: 7 x 37 is about the scan wrap alone. 7 x 127
# under the same settings adds the carried threshold - a uniform row has 97 +- 5 bins >= 60 - at every phase of the wrap.)
A3 = [(16727, None, 8, 8)]   # 3 x R, default occupancy 7: 50181 rows > 7 * 7168; a wave of 8 rows spans three scans
N7, N3 = 5123, 16727


def run_rows(oracle, img, k, z_min, settings, partial=True):
    """img [n, A, R]; settings: (n_scans, occupancy knob or None, rows knob or None, rows per wave the launch must have). One oracle pass over all
    scans, then for every setting the first n_scans scans through the kernel under these knobs."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    n_all, A, R = img.shape
    exp = np.stack([oracle.filter_polar(img[s], z_min, k) for s in range(max(st[0] for st in settings))])
    ctx = capi.Context(capi.default_params(k_strongest=k, z_min=float(z_min)), A, R)
    try:
        for n, occ, cap, rows in settings:
            ctx.tune(capi.TUNE_FILTER_OCCUPANCY, 7 if occ is None else occ)
            ctx.tune(capi.TUNE_FILTER_ROWS_PER_WAVE, 0 if cap is None else cap)
            got_rows, wgs, got_occ = ctx.kstrongest_launch_shape(n)
            assert got_rows == rows, "meant %d rows per wave, the launch has %d (A=%d R=%d n=%d occ=%s cap=%s)" % (rows, got_rows, A, R, n, occ, cap)
            assert wgs == ceil_div(ceil_div(n * A, rows), 4)
            assert got_occ == ((7 if occ is None else occ) if R + 27 <= 4096 else (3 if R + 27 <= 8192 else 2))
            if partial:
                assert (n * A) % (rows * 4) != 0
            got = ctx.kstrongest_host(img[:n])
            if not np.array_equal(got, exp[:n]):
                s_, b = np.argwhere((got != exp[:n]).any(axis=2))[0]
                g = s_ * A + b
                raise AssertionError("scan %d row %d (row %d of its wave of %d) differs (A=%d R=%d k=%d zmin=%d occ=%s n=%d)\n got %s\n exp %s" % (
                    s_, b, g % rows, rows, A, R, k, z_min, occ, n, [hex(x) for x in got[s_][b]], [hex(x) for x in exp[s_][b]]))
    finally:
        ctx.close()
    return exp


def ceil_div(a, b):
    return -(-a // b)


def kept(slots):
    return ((slots >> 24) & 1).sum(axis=-1)


def kth_strongest(rows, k):
    """[N] k-th largest byte of every row"""
    R = rows.shape[1]
    return np.partition(rows, R - k, axis=1)[:, R - k].astype(int)


def count_ge(rows, t):
    return (rows.astype(int) >= np.asarray(t)[:, None]).sum(axis=1)


def scatter(rng, N, R):
    """[N, R] a permutation of the bins per row (a random start and a random stride coprime to R): column j says where the j-th value goes"""
    steps = np.array([t for t in range(1, max(R, 2)) if np.gcd(t, R) == 1])
    return (rng.integers(0, R, size=N)[:, None] + np.arange(R)[None, :] * rng.choice(steps, size=N)[:, None]) % R


def runs_of_1_to_3(rng, N):
    """[N] bool: False and True in turn, in runs of 1 to 3"""
    runs = rng.integers(1, 4, size=N)
    return (np.repeat(np.arange(N) % 2 == 1, runs))[:N]


def quiet_cluttered_rows(rng, N, R, k, z_min):
    """Runs of 1 to 3 cluttered rows (uniform bytes; k of the bins lifted to >= z_min where they fell short) and of 1 to 3 quiet rows (q < k bins
    >= z_min, everything else below) in turn. Returns the rows and which are quiet."""
    quiet = runs_of_1_to_3(rng, N)
    pos = scatter(rng, N, R)
    strong = rng.integers(z_min, 256, size=(N, R), dtype=np.uint8)
    nlift = np.where(quiet, rng.integers(0, k, size=N), k)
    lift = np.arange(R)[None, :] < nlift[:, None]
    base = np.where(quiet[:, None], rng.integers(0, z_min, size=(N, R), dtype=np.uint8), rng.integers(0, 256, size=(N, R), dtype=np.uint8))
    rows = np.empty((N, R), dtype=np.uint8)
    np.put_along_axis(rows, pos, np.where(lift, np.maximum(strong, np.take_along_axis(base, pos, axis=1)), np.take_along_axis(base, pos, axis=1)), axis=1)
    return rows, quiet


def ramp_rows(rng, N, R, k, up):
    """Periods of rows whose bytes are uniform in 0 .. top. Down (5 rows): top = 255, then 30 less each row and below the k-th strongest of the row
    before. Up (3 rows): top = 75, 165, 255."""
    P = 3 if up else 5
    n_per = ceil_div(N, P)
    out = np.empty((n_per, P, R), dtype=np.uint8)
    top = np.full(n_per, 75 if up else 255)
    for i in range(P):
        out[:, i] = (rng.random((n_per, R)) * (top[:, None] + 1)).astype(np.uint8)
        top = top + 90 if up else np.maximum(np.minimum(kth_strongest(out[:, i], k) - 1, top - 30), 0)
    return out.reshape(-1, R)[:N], P


@pytest.mark.parametrize("A,R,settings", [(7, 37, A7), (7, 127, A7_OCC5), (3, 333, A3)])
def test_rows_quiet_and_cluttered_in_turn(oracle, A, R, settings):
    """The restart from the floor (a quiet row behind a cluttered one: the carried threshold finds fewer than k) and, from R = 333, the jump
    (a cluttered row behind a quiet one: the floor finds more than 64)."""
    k, z_min, n = 12, 60, max(st[0] for st in settings)
    rows, quiet = quiet_cluttered_rows(np.random.default_rng(A * 1000 + R), n * A, R, k, z_min)
    assert 0.3 < quiet.mean() < 0.7 and (np.diff(quiet.astype(int)) != 0).mean() > 0.3
    exp = run_rows(oracle, rows.reshape(n, A, R), k, z_min, settings)
    kp = kept(exp).reshape(-1)
    assert np.all(kp[quiet] < k) and np.all(kp[~quiet] == k)
    if R > 100:
        assert np.all(count_ge(rows[~quiet], np.full((~quiet).sum(), z_min)) > 64)


@pytest.mark.parametrize("A,R,settings,up", [(7, 37, A7_OCC5, False), (7, 127, A7_OCC5, False), (3, 333, A3, False), (3, 333, A3, True)])
def test_rows_ramps(oracle, A, R, settings, up):
    """Down: row i of a period has all bytes <= 255 - 30 i and below the k-th strongest of the row before: the carried threshold is always too
    high (no bin reaches it). Up: all bytes <= 75 + 90 i: it is always too low, with more than 64 bins at or above it."""
    k, z_min, n = 12, 60, max(st[0] for st in settings)
    rows, P = ramp_rows(np.random.default_rng(R + up), n * A, R, k, up)
    i = np.arange(n * A) % P
    assert np.all(rows.max(axis=1) <= (75 + 90 * i if up else 255 - 30 * i))
    t = kth_strongest(rows, k)
    c = count_ge(rows[1:], t[:-1])[i[1:] != 0]  # row pairs inside a period
    assert np.all(c > 64) if up else np.all(c == 0) and np.all(t[:-1][i[1:] != 0] > 0)
    run_rows(oracle, rows.reshape(n, A, R), k, z_min, settings)


@pytest.mark.parametrize("k", [12, 40])
def test_rows_threshold_bumped_by_one(oracle, k):
    """Tprev = lo + 1 behind a row with more than 40 candidates. Even rows: c in 41..64 bins equal to v = their k-th strongest and more than 64 bins
    equal to v - 1, so the search can only end at lo = v with c candidates. Odd rows: fewer than k bins above v and plenty equal to v - the
    k-th strongest is exactly v, one below the first probe."""
    A, R, z_min = 3, 333, 60
    n = N3 + 1  # (an even number of rows; the launch takes the first N3 scans: the last pair stays whole in the reference and is cut by the launch)
    rng = np.random.default_rng(k)
    N = n * A
    v = np.repeat(rng.integers(z_min + 2, 255, size=N // 2), 2)
    pos = scatter(rng, N, R)
    rows = (rng.random((N, R)) * (v[:, None] - 1)).astype(np.uint8)  # < v - 1
    c = rng.integers(41, 65, size=N)
    j = rng.integers(0, k, size=N)  # odd rows: bins above v
    idx = np.arange(R)[None, :]
    even = (np.arange(N) % 2 == 0)[:, None]
    fill = np.where(idx < c[:, None], v[:, None], np.where(idx < c[:, None] + 70, v[:, None] - 1, -1))
    above = v[:, None] + 1 + (rng.random((N, R)) * (255 - v[:, None])).astype(int)
    fill_odd = np.where(idx < j[:, None], above, np.where(idx < j[:, None] + 80, v[:, None], -1))
    fill = np.where(even, fill, fill_odd)
    cur = np.take_along_axis(rows, pos, axis=1).astype(int)
    np.put_along_axis(rows, pos, np.where(fill >= 0, fill, cur).astype(np.uint8), axis=1)
    t = kth_strongest(rows, k)
    a, b = rows[0::2], rows[1::2]
    ca = count_ge(a, t[0::2])
    assert np.all(t[0::2] == v[0::2]) and np.all((ca >= 41) & (ca <= 64)) and np.all(count_ge(a, t[0::2] - 1) > 64)
    assert np.all(t[1::2] == t[0::2]) and np.all(count_ge(b, t[0::2] + 1) < k)
    run_rows(oracle, rows.reshape(n, A, R), k, z_min, A3)


@pytest.mark.parametrize("A,R,settings", [(7, 37, A7), (3, 333, A3)])
def test_rows_ties(oracle, A, R, settings):
    n = max(st[0] for st in settings)
    run_rows(oracle, synth.ties_scan(n * A, R, seed=3).reshape(n, A, R), 12, 60, settings)
    run_rows(oracle, synth.ties_scan(n * A, R, seed=4, levels=(60, 61)).reshape(n, A, R), 12, 60, settings)
    run_rows(oracle, synth.ties_scan(n * A, R, seed=5, levels=(10, 200), p=[0.999, 0.001]).reshape(n, A, R), 12, 60, settings)
    run_rows(oracle, synth.ties_scan(n * A, R, seed=6, levels=(10, 200), p=[0.97, 0.03]).reshape(n, A, R), 40, 60, settings)


@pytest.mark.parametrize("k", [12, 40])
def test_rows_many_ties_behind_a_higher_threshold(oracle, k):
    """More than 64 bytes equal to the row's threshold (the positional tie scan), in a row that follows one whose threshold was higher (the carried
    probe finds fewer than k first)."""
    A, R, z_min, n = 3, 333, 60, N3
    rng = np.random.default_rng(100 + k)
    N = n * A
    tb = rng.integers(z_min, 200, size=N)      # tie level of a tied row
    rows = rng.integers(0, 256, size=(N, R), dtype=np.uint8)  # the rows before: uniform, threshold ~ 245
    tied = np.arange(N) % 3 != 0               # one uniform row, two tied rows in turn
    pos = scatter(rng, N, R)
    j = rng.integers(0, k, size=N)
    nt = rng.integers(65, 200, size=N)
    idx = np.arange(R)[None, :]
    low = (rng.random((N, R)) * tb[:, None]).astype(int)  # < tb
    above = tb[:, None] + 1 + (rng.random((N, R)) * (255 - tb[:, None])).astype(int)
    val = np.where(idx < j[:, None], above, np.where(idx < (j + nt)[:, None], tb[:, None], low))
    trow = np.empty((N, R), dtype=np.uint8)
    np.put_along_axis(trow, pos, val.astype(np.uint8), axis=1)
    rows[tied] = trow[tied]
    t = kth_strongest(rows, k)
    first_tied = tied & ~np.roll(tied, 1)
    assert np.all(t[tied] == tb[tied]) and np.all((rows[tied] == tb[tied][:, None]).sum(axis=1) > 64)
    assert np.mean(t[np.flatnonzero(first_tied) - 1] > t[first_tied]) > 0.95 and np.mean(t[1:][tied[1:]] != t[:-1][tied[1:]]) > 0.9
    run_rows(oracle, rows.reshape(n, A, R), k, z_min, A3)


def test_rows_zmin_zero_sparse_between_bright(oracle):
    """z_min = 0: zero-valued bins fill up a sparse row - also when the wave comes from a bright row, with a carried threshold above 1."""
    k = 12
    for A, R, settings, n in ((7, 37, A7_OCC5, N7), (7, 9, A7_OCC5, N7), (7, 127, A7_OCC5, N7), (3, 333, A3, N3)):
        rng = np.random.default_rng(R)
        N = n * A
        rows = rng.integers(100, 256, size=(N, R), dtype=np.uint8)  # bright
        sparse = runs_of_1_to_3(rng, N)
        nz = rng.integers(0, 15, size=N)  # non-zero bins of a sparse row: fewer than k on most
        pos = scatter(rng, N, R)
        srow = np.zeros((N, R), dtype=np.uint8)
        np.put_along_axis(srow, pos, np.where(np.arange(R)[None, :] < nz[:, None], rng.integers(1, 256, size=(N, R)), 0).astype(np.uint8), axis=1)
        rows[sparse] = srow[sparse]
        few = sparse & ((rows > 0).sum(axis=1) < min(k, R))
        assert few.mean() > 0.25 and (few[1:] & ~sparse[:-1]).mean() > 0.1  # ... many of them right behind a bright row
        exp = run_rows(oracle, rows.reshape(n, A, R), k, 0, settings)
        assert np.all(kept(exp).reshape(-1) == min(k, R))  # the zeros filled every row up
        exp1 = run_rows(oracle, rows.reshape(n, A, R), k, 1, settings)
        assert np.all(kept(exp1).reshape(-1)[few] < min(k, R))


@pytest.mark.parametrize("z_min", [255, 254])
def test_rows_zmin_at_the_top(oracle, z_min):
    """Tprev sits at 255 (the lo < 255 guards): rows with no, a few, about k and far more than 64 bytes of 255 in turn"""
    k = 12
    for A, R, settings, n in ((7, 37, A7_OCC5, N7), (3, 333, A3, N3)):
        rng = np.random.default_rng(R + z_min)
        N = n * A
        frac = np.array([0.0, 0.01, k / R, 0.3, 0.9])[rng.integers(0, 5, size=N)]
        rows = rng.integers(0, 256, size=(N, R), dtype=np.uint8)
        rows[rng.random((N, R)) < frac[:, None]] = 255
        c = (rows == 255).sum(axis=1)
        assert (c == 0).mean() > 0.05 and ((c > 0) & (c < k)).mean() > 0.1 and (c >= k).mean() > 0.3 and (R < 100 or (c > 64).mean() > 0.3)
        run_rows(oracle, rows.reshape(n, A, R), k, z_min, settings)


@pytest.mark.parametrize("z_min", [0, 60, 255])
def test_rows_constant_between_random(oracle, z_min):
    for A, R, settings, n, k in ((7, 37, A7_OCC5, N7, 12), (3, 333, A3, N3, 12), (3, 333, A3, N3, 64)):
        rng = np.random.default_rng(R + z_min + k)
        N = n * A
        rows = rng.integers(0, 256, size=(N, R), dtype=np.uint8)
        what = rng.integers(0, 8, size=N)  # 0..3: a constant row of 0 / 59 / 60 / 255; 4..7: random
        for w, val in enumerate((0, 59, 60, 255)):
            rows[what == w] = val
        run_rows(oracle, rows.reshape(n, A, R), k, z_min, settings)


@pytest.mark.parametrize("R", [37, 23])
@pytest.mark.parametrize("k", [12, 3])
def test_rows_kept_points_at_the_row_ends(oracle, R, k):
    """test_kept_points_at_the_row_ends with several rows per wave at A = 7: the suppression halo stays masked by the scan the ROW belongs to
    when the wave came from another scan."""
    A, n = 7, 2927
    block = row_end_image(np.random.default_rng(R * 31 + k), 200 * A, R).reshape(200, A, R)
    img = np.tile(block, (n // 200 + 1, 1, 1))[:n]
    run_rows(oracle, img, k, 60, A7_OCC5[:3] + [(1757, 6, 8, 3), (2049, 7, 8, 3)])


def mixed_rows(rng, N, R, k, z_min):
    """Blocks of 16 rows of the families above (those with z_min = 60) in turn"""
    out = np.empty((N, R), dtype=np.uint8)
    fam = (np.arange(N) // 16) % 6
    for f in range(6):
        m = int((fam == f).sum())
        if f == 0:
            src = quiet_cluttered_rows(rng, m, R, k, z_min)[0]
        elif f in (1, 2):
            src = ramp_rows(rng, m, R, k, f == 2)[0]
        elif f == 3:
            src = synth.ties_scan(m, R, seed=int(rng.integers(1 << 30)))
        elif f == 4:
            src = synth.ties_scan(m, R, seed=int(rng.integers(1 << 30)), levels=(10, 200), p=[0.999, 0.001])
        else:
            src = rng.integers(0, 256, size=(m, R), dtype=np.uint8)
            what = rng.integers(0, 8, size=m)
            for w, val in enumerate((0, 59, 60, 255)):
                src[what == w] = val
        out[fam == f] = src
    return out


# 1 x 64: every row is the first and the last row of its scan; default knobs: 21507 rows in (3 * 7168, 4 * 7168]
# 17 x 64: the default cap turns from 4 to 6 at 1536 scans (5120 slots: 26112 rows would fill five, the cap of 1535 scans stops at four). 1536 x 17
# is a multiple of 24 - every wave full -, 1537 x 17 is not.
@pytest.mark.parametrize("A,R,settings,partial", [
    (1, 64, [(21507, None, None, 4)], True),
    (17, 64, [(1535, 5, None, 4), (1537, 5, None, 6)], True),
    (17, 64, [(1536, 5, None, 6)], False),
    (9, 5000, [(401, None, None, 2)], True),   # NCH = 8, occupancy 3: 3609 rows > 3072
    (9, 9000, [(301, None, None, 2)], True),   # NCH = 16, occupancy 2: 2709 rows > 2048
])
def test_rows_other_shapes(oracle, A, R, settings, partial):
    k, z_min, n = 12, 60, max(st[0] for st in settings)
    rows = mixed_rows(np.random.default_rng(A * R), n * A, R, k, z_min)
    run_rows(oracle, rows.reshape(n, A, R), k, z_min, settings, partial=partial)


# (400 x 16 r rows is a multiple of 4 r for r = 4 whatever the scan count: at 54 scans every wave is full; 65 x 400 is no multiple of 24)
@pytest.mark.parametrize("n,occ,cap,rows_per_wave,partial", [(54, None, None, 4, False), (65, 5, 6, 6, True)])
def test_rows_production_shape(oracle, n, occ, cap, rows_per_wave, partial):
    A, R, k, z_min = 400, 3360, 12, 60
    rows = mixed_rows(np.random.default_rng(n), n * A, R, k, z_min)
    run_rows(oracle, rows.reshape(n, A, R), k, z_min, [(n, occ, cap, rows_per_wave)], partial=partial)


def test_launch_shape_read_back(hip_lib):
    """cfear_kstrongest_launch_shape on a context, against the shapes include/cfear_hip.h states (tests/test_filter_shape_cpu.py: the same
    arithmetic without a GPU)"""
    ctx = capi.Context(capi.default_params(), 400, 3360)
    assert [ctx.kstrongest_launch_shape(n)[:2] for n in (4608, 1535, 1536, 5)] == [(6, 76800), (4, 38375), (6, 25600), (1, 500)]
    for cap, rows in ((1, 1), (3, 3), (8, 8), (300, 258)):
        ctx.tune(capi.TUNE_FILTER_ROWS_PER_WAVE, cap)
        assert ctx.kstrongest_launch_shape(4608)[0] == rows and ctx.kstrongest_launch_shape(5)[0] == 1
    ctx.tune(capi.TUNE_FILTER_ROWS_PER_WAVE, 0)
    for knob, occ in ((4, 5), (5, 5), (6, 6), (7, 7), (9, 7)):
        ctx.tune(capi.TUNE_FILTER_OCCUPANCY, knob)
        assert ctx.kstrongest_launch_shape(64)[2] == occ
    with pytest.raises(capi.CfearError):
        ctx.kstrongest_launch_shape(0)
    ctx.close()
    for R, occ in ((5000, 3), (9000, 2)):
        ctx = capi.Context(capi.default_params(), 9, R)
        assert ctx.kstrongest_launch_shape(9) == (1, ceil_div(81, 4), occ)
        ctx.close()

