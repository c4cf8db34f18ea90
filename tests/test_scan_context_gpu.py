"""Loop candidates by appearance on the device (scan_context.hip): the Scan-Context descriptor bit for bit against the numpy twin
(scancontext.py), the float32 distance against the twin's float64 within B = (n_rings + n_sectors + 8) * 2^-24, the candidate lists under
the rule of scan_context_inputs (a decision the twin takes with a margin above 2 B comes out the same; elsewhere either answer), the exact
rules (key distance, stage 1, ties), batch independence, rotations, and the routes that read the keyframe log.

The drive of the log test: sweeps 0 .. 15 of test_keyframes_gpu's images out, 14 .. 0 back, compensation off - a return keyframe whose sweep
shows the image of an outbound keyframe has recorded the very same cloud. The oracle's fuser (on the CPU) fuses every second sweep of this
drive both ways, keyframes 8 .. 14 on the images of keyframes 6 .. 0."""
import ctypes as C
import math

import numpy as np
import pytest

from cfear_radarodometry_code_public_amd import capi, replay, scancontext as sc
import scan_context_inputs as si
import test_keyframes_gpu as kg
import test_keyframe_clouds_gpu as kcg

pytestmark = pytest.mark.gpu
A, R = 400, 3360
TURN = 15  # the log test's drive: images 0 .. TURN, then TURN - 1 .. 0


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(capi.default_params(**kcg.KW), A, R)
    yield c
    c.close()


def params(n_rings, n_sectors, **kw):
    return capi.sc_params(n_rings=n_rings, n_sectors=n_sectors, max_range=si.MAX_RANGE, **kw)


# ---- the descriptor ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rings,n_sectors", si.SHAPES)
def test_descriptor_is_the_twins_bit_for_bit(ctx, n_rings, n_sectors):
    """clouds of every size at which the kernel's loops change their trip count, the special points and the azimuth grid, all three values"""
    clouds = [si.random_cloud(n, 100 + n) for n in si.CLOUD_SIZES] + [si.special_cloud(n_rings, n_sectors), si.grid_cloud()]
    table = sc.layout(n_rings=n_rings, n_sectors=n_sectors, max_range=si.MAX_RANGE)
    for value in (capi.SC_MAX, capi.SC_SUM, capi.SC_COUNT):
        p = params(n_rings, n_sectors, value=value)
        bins, ring_sums, dropped = ctx.scan_context(clouds, p)
        assert bins.shape == (len(clouds), n_sectors, n_rings) and bins.dtype == np.uint32
        for k, c in enumerate(clouds):
            eb, er, ed = sc.describe(c, p, table)
            assert bins[k].tobytes() == eb.tobytes(), (value, k, len(c), int(np.count_nonzero(bins[k] != eb)))
            assert ring_sums[k].tobytes() == er.tobytes() and int(dropped[k]) == ed, (value, k, len(c))
        assert int(dropped[-2]) == 7 and not dropped[:len(si.CLOUD_SIZES)].any() and not bins[0].any()
        if value == capi.SC_COUNT and n_rings * n_sectors > 1:
            assert int(ring_sums[len(si.CLOUD_SIZES) - 1].sum()) > 35000  # (the 65 536-point cloud: most of it in range)
    one = ctx.scan_context(clouds[4], params(n_rings, n_sectors))  # a single array: no leading axis
    assert one[0].tobytes() == ctx.scan_context(clouds, params(n_rings, n_sectors))[0][4].tobytes()


def test_descriptor_refusals(ctx):
    with pytest.raises(capi.CfearError, match="rc=-1.*cloud 1 has 65537 points"):
        ctx.scan_context([si.random_cloud(10, 1), np.zeros((capi.SC_MAX_POINTS + 1, 3), dtype=np.float32)])
    for kw, field in ((dict(n_rings=41), "n_rings"), (dict(n_sectors=0), "n_sectors"), (dict(max_range=float("nan")), "max_range"), (dict(value=5), "value")):
        with pytest.raises(capi.CfearError, match="rc=-1.*params.%s" % field):
            ctx.scan_context([si.random_cloud(10, 1)], capi.sc_params(**kw))
    bins, ring_sums, dropped = ctx.scan_context([])
    assert bins.shape == (0, 60, 20) and len(dropped) == 0


# ---- the distance -----------------------------------------------------------------------------------------------------------------------
def pair_match(ctx, pairs, p):
    """the device's (distance, shift) of every (a = to, b = from): a set of two per pair, all sets in one call"""
    q = sc.params(p, min_index_gap=1, n_keys=0, max_per_node=1, max_distance=1.0)
    got = ctx.scan_context_match([np.stack([b, a]) for a, b in pairs], q)
    assert len(got) == len(pairs) and list(got["sequence"]) == list(range(len(pairs))) and np.all(got["to"] == 1) and np.all(got["from"] == 0)
    return got


@pytest.mark.parametrize("n_rings,n_sectors", si.SHAPES)
def test_distance_is_within_the_rounding_bound_of_the_twins(ctx, n_rings, n_sectors):
    p = params(n_rings, n_sectors)
    B = sc.rounding_bound(p)
    assert abs(B - {(20, 60): 5.2e-6, (40, 120): 1.0e-5}.get((n_rings, n_sectors), B)) <= 0.05e-5
    pairs = si.distance_pairs(n_rings, n_sectors)
    got = pair_match(ctx, pairs, p)
    worst, compared = 0.0, 0
    for r, (a, b) in zip(got, pairs):
        d, shift, yaw, margin = sc.distance(a, b)
        worst = max(worst, abs(float(r["distance"]) - d) / B)
        assert int(r["key_distance"]) == sc.key_distance(a.sum(axis=0), b.sum(axis=0))
        if margin > 2.0 * B:
            compared += 1
            assert int(r["shift"]) == shift and r["yaw"] == yaw, (int(r["shift"]), shift, margin)
    print("distance %2d x %3d: worst |device - twin| / B = %.4f over %d pairs, %d shifts compared" % (n_rings, n_sectors, worst, len(pairs), compared))
    assert worst <= 1.0 and compared >= 0.95 * len(pairs)


# ---- the candidates ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in si.MATCH_CASES])
def test_candidates_are_the_twins(ctx, name):
    sets, p, results = si.match_case(name)
    got = ctx.scan_context_match(sets, p)
    worst, total, soft = si.compare_candidates(got, results, p, name)
    print("%-20s %4d candidates, %4d decisions, %d within 2 B; worst distance error / B = %.4f" % (name, len(got), total, soft, worst))
    assert soft <= 0.05 * total and len(got) >= 10
    assert got.tobytes() == ctx.scan_context_match(sets, p).tobytes()  # two calls in a row


def test_stage_one_selection_is_exact(ctx):
    """with room for every pair stage 1 hands on and no threshold, the `from` of a `to` are exactly the twin's n_keys smallest key distances"""
    sets, p0, _ = si.match_case("default")
    for n_keys in (1, 5, 16):
        p = sc.params(p0, n_keys=n_keys, max_per_node=16, max_distance=1.0)
        got = ctx.scan_context_match(sets, p)
        for g, s in enumerate(sets):
            ring_sums = s.sum(axis=1, dtype=np.uint32)
            mine = got[got["sequence"] == g]
            for to in range(len(s)):
                want = sc.stage1(ring_sums, to, p)
                rows = mine[mine["to"] == to]
                assert sorted(int(f) for f in rows["from"]) == sorted(f for _, f in want), (n_keys, g, to)
                assert {int(r["from"]): int(r["key_distance"]) for r in rows} == {f: K for K, f in want}, (n_keys, g, to)


def test_exact_rules_and_set_shapes(ctx):
    rng = np.random.default_rng(8)
    flat = np.tile(np.arange(1, 21, dtype=np.uint32), (60, 1))
    none = np.zeros((60, 20), dtype=np.uint32)
    some = si.random_descriptor(20, 60, rng)
    # ties: bit-identical descriptors in a set -> the smaller `from` first; all columns equal -> shift 0
    got = ctx.scan_context_match(np.stack([some, flat, some, none, some, flat]), min_index_gap=1, n_keys=0, max_per_node=16, max_distance=0.2)
    assert [(int(c["to"]), int(c["from"])) for c in got] == [(2, 0), (4, 0), (4, 2), (5, 1)]
    assert np.all(got["shift"] == 0) and np.all(np.abs(got["distance"]) <= sc.rounding_bound()) and np.all(got["key_distance"] == 0) and np.all(got["yaw"] == 0.0)
    assert got["distance"][1] == got["distance"][2]
    # two empty descriptors: distance 1 - a candidate only at max_distance 1
    empties = np.stack([none] * 9)
    assert len(ctx.scan_context_match(empties, min_index_gap=1, max_distance=0.999)) == 0
    at_one = ctx.scan_context_match(empties, min_index_gap=1, max_distance=1.0, max_per_node=2)
    assert len(at_one) == 1 + 2 * 7 and np.all(at_one["distance"] == 1.0) and np.all(at_one["shift"] == 0)
    assert [int(f) for f in at_one["from"][:5]] == [0, 0, 1, 0, 1]
    # min_index_gap larger than the set, sets of 0 and 1, n_keys larger than what is eligible
    sets, p0, results = si.match_case("default")
    assert len(ctx.scan_context_match(sets[3], sc.params(p0, min_index_gap=63))) == 0
    assert len(ctx.scan_context_match([sets[0], sets[1], sets[0]], p0)) == 0
    assert len(ctx.scan_context_match([], p0)) == 0
    few = ctx.scan_context_match(sets[3][:12], sc.params(p0, n_keys=64, max_per_node=16, max_distance=1.0))
    assert len(few) == sum(range(1, 7)) and [int(t) for t in few["to"][:3]] == [6, 7, 7]
    # n_keys = 0 is n_keys = 64 where no more than 64 are eligible: sets up to 64 + gap
    for n in (63, 64, 65, 70):
        s = si.place_set(n, 20, 60, 900 + n)
        for mp in (1, 16):
            a = ctx.scan_context_match(s, sc.params(p0, n_keys=0, max_per_node=mp))
            b = ctx.scan_context_match(s, sc.params(p0, n_keys=64, max_per_node=mp))
            assert a.tobytes() == b.tobytes() and len(a) >= n - 6 - 9, (n, mp)
    # a buffer too short: the project's error for it, the count, and nothing written
    p = sc.params(p0)
    s = np.ascontiguousarray(sets[3])
    off = np.array([0, len(s)], dtype=np.int32)
    full = ctx.scan_context_match(s, p)
    buf = np.full(len(full) * capi.SC_CANDIDATE_DTYPE.itemsize, 0x55, dtype=np.uint8)
    n = C.c_int(-1)
    rc = ctx._L.cfear_scan_context_match(ctx._h, C.byref(p), 1, off.ctypes.data, s.ctypes.data, buf.ctypes.data, len(full) - 1, C.byref(n))
    assert rc == -6 and n.value == len(full) and np.all(buf == 0x55)
    rc = ctx._L.cfear_scan_context_match(ctx._h, C.byref(p), 1, off.ctypes.data, s.ctypes.data, None, 0, C.byref(n))
    assert rc == -6 and n.value == len(full)
    rc = ctx._L.cfear_scan_context_match(ctx._h, C.byref(p), 1, off.ctypes.data, s.ctypes.data, buf.ctypes.data, len(full), C.byref(n))
    assert rc == 0 and buf.tobytes() == full.tobytes()
    for kw, field in ((dict(min_index_gap=0), "min_index_gap"), (dict(n_keys=65), "n_keys"), (dict(max_per_node=17), "max_per_node"), (dict(max_distance=0.0), "max_distance")):
        with pytest.raises(capi.CfearError, match="rc=-1.*params.%s" % field):
            ctx.scan_context_match(s, capi.sc_params(**kw))


def test_a_sets_candidates_do_not_depend_on_the_batch(ctx):
    """five sets in one call, the same five reversed, and each alone: the same bytes (but for the set's number)"""
    _, p, _ = si.match_case("default")
    five = [si.place_set(n, 20, 60, 700 + n) for n in (40, 7, 65, 0, 130)]
    p = sc.params(p, max_per_node=3)

    def per_set(got, order):
        out = {}
        for pos, g in enumerate(order):
            rows = got[got["sequence"] == pos].copy()
            rows["sequence"] = 0
            out[g] = rows.tobytes()
        return out

    fwd = per_set(ctx.scan_context_match(five, p), [0, 1, 2, 3, 4])
    rev = per_set(ctx.scan_context_match(five[::-1], p), [4, 3, 2, 1, 0])
    alone = {g: ctx.scan_context_match(five[g], p).tobytes() for g in range(5)}
    assert fwd == rev == alone and sum(len(v) for v in alone.values()) >= 40 * capi.SC_CANDIDATE_DTYPE.itemsize
    assert fwd == per_set(ctx.scan_context_match(five, p), [0, 1, 2, 3, 4])


@pytest.mark.parametrize("n_rings,n_sectors", [s for s in si.SHAPES if s[1] >= 3])
def test_a_rotated_cloud_is_found_at_its_shift(ctx, n_rings, n_sectors):
    p = params(n_rings, n_sectors)
    b_cloud, _, _ = si.ringed_cloud(max(8, (2 * n_rings * n_sectors) // 5), n_rings, n_sectors, 11)
    ms = (1, n_sectors // 2, n_sectors - 1)
    clouds = [b_cloud] + [si.rotated(b_cloud, -m * 2.0 * math.pi / n_sectors) for m in ms]
    bins = ctx.scan_context(clouds, p)[0]
    pairs = []
    for k, m in enumerate(ms):
        d, shift, yaw, margin = sc.distance(bins[k + 1], bins[0])  # asserted on the twin first
        assert shift == m and d < 1e-12 and margin > 2.0 * sc.rounding_bound(p), (m, d, shift, margin)
        pairs.append((bins[k + 1], bins[0]))
    got = pair_match(ctx, pairs, p)
    assert [int(s) for s in got["shift"]] == list(ms) and np.all(np.abs(got["distance"]) <= sc.rounding_bound(p))
    assert got["yaw"][0] > 0.0 > got["yaw"][2]


# ---- from the log -----------------------------------------------------------------------------------------------------------------------
def drive(B):
    """[2 TURN + 1, B, A, R]: out and back, sequence q sees the world rotated by q azimuths"""
    fr = kg.frames(B)
    return np.ascontiguousarray(np.concatenate([fr[:TURN + 1], fr[:TURN][::-1]]))


def image_of(t):
    return t if t <= TURN else 2 * TURN - t


def test_descriptors_and_candidates_from_the_log(ctx):
    B, T = 3, 2 * TURN + 1
    fr = drive(B)
    c0 = capi.Context(capi.default_params(**dict(kcg.KW, compensate=0)), A, R)
    p = capi.sc_params(min_index_gap=4)
    Bd = sc.rounding_bound(p)
    table = sc.layout(p)
    runs = []
    for call in (True, False):
        odo = c0.odometry(B)
        odo.record_keyframes(kcg.ALL, T, kg.MAX_CELLS, T * 2 * A * 12)
        first = odo.replay_host(fr[:28])
        if call:
            before = (kcg.log_bytes(odo), kg.log_of(odo))
            nodes = [odo.keyframes(q) for q in range(B)]
            desc = []
            for source in (0, 1):
                ps = sc.params(p, source=source)
                desc = []
                for q in range(B):
                    bins, ring_sums = odo.keyframe_descriptors(q, ps)
                    assert len(bins) == len(nodes[q]) >= 10
                    for i in range(len(bins)):  # bit-exact against the twin on the recorded cloud
                        eb, er, _ = sc.describe(odo.keyframe_cloud(q, i, peaks=bool(source)), ps, table)
                        assert bins[i].tobytes() == eb.tobytes() and ring_sums[i].tobytes() == er.tobytes(), (source, q, i)
                    desc.append(bins)
                cand = odo.keyframe_candidates(ps)
                assert cand.tobytes() == ctx.scan_context_match(desc, ps).tobytes(), source  # the caller-descriptor route, byte for byte
            # (source = 1 ran last: what follows is about the peaks clouds' candidates too, so take the filtered clouds' again)
            cand = odo.keyframe_candidates(p)
            pairs_seen = 0
            jobs = []
            for q in range(B):
                sweep = [int(s) for s in nodes[q]["sweep"]]
                out = {image_of(t): i for i, t in enumerate(sweep) if t <= TURN}
                mine = cand[cand["sequence"] == q]
                for i, t in enumerate(sweep):
                    if t > TURN and image_of(t) in out and i - out[image_of(t)] >= 4:  # a return keyframe on an outbound keyframe's image
                        row = mine[mine["to"] == i]
                        assert len(row) == 1 and int(row["from"][0]) == out[image_of(t)], (q, i, row)
                        assert abs(float(row["distance"][0])) <= Bd and int(row["shift"][0]) == 0 and int(row["key_distance"][0]) == 0, (q, i, row)
                        pairs_seen += 1
                        jobs.append(replay.appearance_jobs(q, row, nodes[q]))
            print("return keyframes on outbound images:", pairs_seen, "candidates in all:", len(cand), "loop_candidates by pose:",
                  [len(replay.loop_candidates(nd)) for nd in nodes])
            assert pairs_seen >= 3 * B
            jobs = np.concatenate(jobs)
            assert np.all(jobs["flags"] == 1)
            edges = odo.keyframe_edges(jobs)
            t_be = np.abs(edges["t_be"])
            print("edges of the appearance jobs: success", edges["success"].tolist(), "worst |t_be|", t_be.max(axis=0))
            assert np.all(edges["success"] == 1) and np.all(edges["status"] == 0)
            assert t_be[:, :2].max() <= 1e-4 and t_be[:, 2].max() <= 1e-5  # the project's parity bound: the same cloud registers onto itself
            after = (kcg.log_bytes(odo), kg.log_of(odo))
            assert before[0] == after[0]
            kg.logs_equal(before[1], after[1])
        rest = odo.replay_host(fr[28:])
        runs.append((first, rest, kcg.log_bytes(odo), odo.poses()))
        odo.release()
    (f0, r0, l0, p0), (f1, r1, l1, p1) = runs  # a replay continued after the calls is the replay without them, bit for bit
    assert f0.tobytes() == f1.tobytes() and r0.tobytes() == r1.tobytes() and l0 == l1 and p0.tobytes() == p1.tobytes()
    # refusals: a log without clouds, the peaks cloud of a log without peaks, recording off
    for what, kw, text in ((capi.KF_NODES | capi.KF_CELLS, {}, "CFEAR_KF_CLOUD"), (capi.KF_NODES | capi.KF_CLOUD, dict(source=1), "CFEAR_KF_PEAKS"), (0, {}, "recording is off")):
        odo = c0.odometry(1)
        if what:
            odo.record_keyframes(what, T, kg.MAX_CELLS, T * 2 * A * 12)
        odo.replay_host(np.ascontiguousarray(fr[:6, :1]))
        with pytest.raises(capi.CfearError, match="rc=-1.*" + text):
            odo.keyframe_descriptors(0, **kw)
        with pytest.raises(capi.CfearError, match="rc=-1.*" + text):
            odo.keyframe_candidates(**kw)
        if what & capi.KF_CLOUD:  # ... and what it does hold is described
            assert len(odo.keyframe_descriptors(0)[0]) == len(odo.keyframes(0)) >= 2 and len(odo.keyframe_candidates()) == 0
        odo.release()
    c0.close()


def test_replay_grid_and_the_command_line_close_loops_by_appearance(tmp_path):
    from cfear_radarodometry_code_public_amd import readers
    imgs = np.ascontiguousarray(drive(1)[:, 0])
    rows = [capi.default_params(**dict(kcg.KW, compensate=0)), capi.default_params(**dict(kcg.KW, compensate=0, min_keyframe_dist=3.0))]
    spec = dict(appearance=dict(min_index_gap=4, max_distance=0.3), n_side=1)
    out = replay.replay_grid(imgs, rows, keyframes="cells+clouds", edges=spec, optimise={})
    assert not out["keyframes_dropped"].any() and len(out["keyframe_candidates"]) == len(out["keyframe_edges"]) == 2
    for q in range(2):
        cand, e, nodes = out["keyframe_candidates"][q], out["keyframe_edges"][q], out["keyframes"][q]
        assert len(cand) == len(e) >= 2 and np.all(cand["sequence"] == q) and np.all(e["sequence"] == q)
        assert np.array_equal(e["to"], cand["to"]) and np.array_equal(e["from"], cand["from"]) and np.all(cand["to"] - cand["from"] >= 4)
        assert len(out["keyframe_cells"][q]) == len(out["keyframe_clouds"][q]) == len(out["keyframe_peaks"][q]) == len(nodes)
        assert out["keyframe_poses_optimised"][q].shape == (len(nodes), 3)
        one = replay.replay_grid(imgs, [rows[q]], keyframes="cells+clouds", edges=spec)  # a row's candidates do not depend on the grid
        for f in ("to", "from", "shift", "distance", "yaw", "key_distance"):
            assert one["keyframe_candidates"][0][f].tobytes() == cand[f].tobytes(), (q, f)
    assert e["success"].any() and out["poses_optimised"].shape == out["poses"].shape
    # existing spellings are what they were
    plain = replay.replay_grid(imgs[:8], rows, keyframes="cells", edges=dict(min_index_gap=2, max_dist=3.0))
    assert "keyframe_candidates" not in plain and "keyframe_clouds" not in plain and len(plain["keyframe_edges"]) == 2
    # the command line over the same sweeps as an Oxford PNG directory
    d = tmp_path / "radar"
    d.mkdir()
    for i in range(len(imgs)):
        ts = 1547131046353776 + i * 250000
        readers.write_png_gray8(d / ("%d.png" % ts), readers.oxford_png_rows(imgs[i], ts + np.arange(A) * 625), filter_type=2)
    g = tmp_path / "graph.g2o"
    res = replay.main(["--oxford_png_dir", str(d), "--est_directory", str(tmp_path / "est"), "--range-res", "0.0595238", "--z-min", "60", "--res", "3.0",
                       "--submap_scan_size", "4", "--weight_option", "4", "--min_distance", str(kcg.KW["min_distance"]), "--disable_compensate", "1",
                       "--store_graph", str(g), "--loop_edges_appearance", "4,0.3,1"])
    cand, e = out["keyframe_candidates"][0], out["keyframe_edges"][0]
    assert res["keyframes"] == len(out["keyframes"][0]) and res["appearance_candidates"] == len(cand) and res["loop_edges"] == int(e["success"].sum())
    back = replay.read_g2o_edges(g)
    ok = e[e["success"] != 0]
    assert back["to"].tobytes() == ok["to"].tobytes() and back["from"].tobytes() == ok["from"].tobytes() and back["t_be"].tobytes() == ok["t_be"].tobytes()
    nodes_back = replay.read_g2o(g)
    for f in ("index", "prev", "pose", "t_be"):
        assert nodes_back[f].tobytes() == out["keyframes"][0][f].tobytes(), f
