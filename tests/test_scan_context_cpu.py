"""Scan-Context descriptors and loop candidates by appearance, the parts that need no device: the C ABI (header, EXPORTS, record sizes, the
kernels in a library built for gfx950), the layout table, the numpy twin's bin rule (scancontext.py) against atan2 / hypot and against
the stand-alone host check (host/scan_context_check.cpp runs csrc/scan_context_dev.h, what the kernels run), the twin's distance on
rotated clouds, replay.appearance_jobs, and that the device tests' inputs leave the twin's decisions clear of the float32 rounding bound."""
import ctypes as C
import inspect
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from cfear_radarodometry_code_public_amd import capi, replay, scancontext as sc
import scan_context_inputs as si

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cfear_radarodometry_code_public_amd", "host")


def test_abi_header_exports_and_sizes(hip_lib):
    txt = open(os.path.join(ROOT, "include", "cfear_hip.h")).read()
    names = ("cfear_sc_default_params", "cfear_scan_context_layout", "cfear_scan_context_describe", "cfear_scan_context_match",
             "cfear_odometry_keyframe_descriptors", "cfear_odometry_keyframe_candidates")
    for name in names:
        assert re.search(r"\b(int|void) %s\(" % name, txt), name
        assert name in capi.EXPORTS and hasattr(hip_lib, name), name
    blob = open(capi.lib_path(), "rb").read()
    assert b"sc_describe_kernel" in blob and b"sc_match_kernel" in blob and b"gfx950" in blob
    assert capi.SC_CANDIDATE_DTYPE.itemsize == 40
    for cname, size, st in (("cfear_sc_params", 48, capi.ScParams), ("cfear_sc_candidate", 40, capi.ScCandidate)):
        assert C.sizeof(st) == size
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), txt, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        declared = [n.strip() for line in body.split(";") if line.strip() for n in line.strip().split(None, 1)[1].split(",")]
        assert declared == [f for f, _ in st._fields_], (cname, declared)  # the header's fields in the header's order
    p = capi.sc_params()
    assert (p.n_rings, p.n_sectors, p.value, p.source, p.min_index_gap, p.n_keys, p.max_per_node) == (20, 60, capi.SC_MAX, 0, 6, 10, 1)
    assert (p.max_range, p.max_distance) == (80.0, 0.4)
    for macro, value in (("CFEAR_SC_MAX", capi.SC_MAX), ("CFEAR_SC_SUM", capi.SC_SUM), ("CFEAR_SC_COUNT", capi.SC_COUNT), ("CFEAR_SC_MAX_RINGS", capi.SC_MAX_RINGS),
                         ("CFEAR_SC_MAX_SECTORS", capi.SC_MAX_SECTORS), ("CFEAR_SC_MAX_KEYS", capi.SC_MAX_KEYS), ("CFEAR_SC_MAX_PER_NODE", capi.SC_MAX_PER_NODE),
                         ("CFEAR_SC_MAX_POINTS", capi.SC_MAX_POINTS)):
        assert re.search(r"#define %s %d\b" % (macro, value), txt), macro
    for cls, name in ((capi.Context, "scan_context"), (capi.Context, "scan_context_match"), (capi.Odometry, "keyframe_descriptors"), (capi.Odometry, "keyframe_candidates")):
        assert hasattr(cls, name), name
    # the layout refuses what the header says it refuses, and names nothing it cannot
    for kw in (dict(n_rings=0), dict(n_rings=41), dict(n_sectors=0), dict(n_sectors=121), dict(max_range=0.0), dict(max_range=math.inf), dict(value=3), dict(source=2),
               dict(min_index_gap=0), dict(n_keys=65), dict(n_keys=-1), dict(max_per_node=0), dict(max_per_node=17), dict(max_distance=0.0), dict(max_distance=1.5)):
        with pytest.raises(capi.CfearError):
            capi.scan_context_layout(capi.sc_params(**kw))


@pytest.mark.parametrize("n_rings,n_sectors", si.SHAPES)
def test_layout_table(hip_lib, n_rings, n_sectors):
    edge2, sdir = sc.layout(n_rings=n_rings, n_sectors=n_sectors, max_range=si.MAX_RANGE)
    assert edge2.shape == (n_rings + 1,) and sdir.shape == (n_sectors, 2)
    assert np.array_equal(edge2, (np.arange(n_rings + 1) * si.MAX_RANGE / n_rings) ** 2) and edge2[-1] == si.MAX_RANGE ** 2
    t = 2.0 * np.pi * np.arange(n_sectors) / n_sectors
    assert np.max(np.abs(sdir[:, 0] - np.cos(t))) <= 1e-15 and np.max(np.abs(sdir[:, 1] - np.sin(t))) <= 1e-15
    axes = {0: (1.0, 0.0), 1: (0.0, 1.0), 2: (-1.0, 0.0), 3: (0.0, -1.0)}
    seen = 0
    for j in range(n_sectors):
        if (4 * j) % n_sectors == 0:
            assert tuple(sdir[j]) == axes[4 * j // n_sectors], j
            seen += 1
    assert seen == {1: 1, 60: 4, 40: 4, 120: 4, 7: 1, 64: 4, 65: 1}[n_sectors]


@pytest.mark.parametrize("n_sectors", [1, 2, 3, 40, 60, 64, 65, 120])
def test_twin_bin_rule_against_atan2_and_hypot(hip_lib, n_sectors):
    """the count rule is floor(atan2 / 2 pi * n_sectors) and floor(hypot / max_range * n_rings) on random float32 points"""
    n_rings = 20
    pts = si.random_cloud(200000, 77 + n_sectors, spread=85.0)
    status, ring, sector, v = sc.bins_of_points(pts, n_rings=n_rings, n_sectors=n_sectors, max_range=si.MAX_RANGE)
    x, y = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    ang = np.arctan2(y, x)
    ang[ang < 0.0] += 2.0 * np.pi
    inside = x * x + y * y < si.MAX_RANGE ** 2
    assert np.array_equal(status == 0, inside) and np.all(status[~inside] == 2) and 0.5 < inside.mean() < 0.95
    assert np.count_nonzero(sector[inside] != np.floor(ang[inside] / (2.0 * np.pi) * n_sectors).astype(int)) == 0
    assert np.count_nonzero(ring[inside] != np.floor(np.hypot(x, y)[inside] / si.MAX_RANGE * n_rings).astype(int)) == 0
    assert np.array_equal(v[inside], np.clip(np.trunc(pts[inside, 2].astype(np.float64)), 0, 255).astype(int))
    assert len(np.unique(sector[inside])) == n_sectors and len(np.unique(ring[inside])) == n_rings


def build_check(target="scan_context_check"):
    subprocess.check_call(["make", "-C", HOST, target], stdout=subprocess.DEVNULL)
    return os.path.join(HOST, target)


def check_bins(exe, cloud, n_rings, n_sectors, path):
    """the stand-alone program's bin of every point, on the library's table"""
    edge2, sdir = sc.layout(n_rings=n_rings, n_sectors=n_sectors, max_range=si.MAX_RANGE)
    with open(path, "wb") as f:
        f.write(struct.pack("<iii", n_rings, n_sectors, len(cloud)))
        f.write(np.ascontiguousarray(edge2, dtype="<f8").tobytes() + np.ascontiguousarray(sdir, dtype="<f8").tobytes() + np.ascontiguousarray(cloud, dtype="<f4").tobytes())
    out = subprocess.run([exe, "bins", str(path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return np.array([[int(w) for w in line.split()] for line in out.stdout.splitlines()], dtype=np.int64).reshape(-1, 4)


@pytest.mark.parametrize("n_rings,n_sectors", si.SHAPES)
def test_twin_and_host_check_give_the_same_bins(hip_lib, tmp_path, n_rings, n_sectors):
    """the points where rounding decides - the 400-row azimuth grid, whose rows lie on sector boundaries, and the special points - land in
    the same bin under the numpy twin and under the header the kernels are compiled from"""
    exe = build_check()
    grid = si.grid_cloud()
    cloud = np.concatenate([grid, si.special_cloud(n_rings, n_sectors), si.random_cloud(2000, 5)])
    got = check_bins(exe, cloud, n_rings, n_sectors, tmp_path / "points.bin")
    status, ring, sector, v = sc.bins_of_points(cloud, n_rings=n_rings, n_sectors=n_sectors, max_range=si.MAX_RANGE)
    assert np.array_equal(got[:, 0], status) and np.array_equal(got[:, 1], ring) and np.array_equal(got[:, 2], sector) and np.array_equal(got[:, 3], v)
    assert {0, 1, 2} <= set(status.tolist())
    if n_sectors in (40, 60):  # rows on a boundary go to either side: this is what an atan2 on the device could not reproduce
        k = np.repeat(np.arange(400), 8)
        on = (k * n_sectors) % 400 == 0
        nominal = (k * n_sectors) // 400
        below = np.count_nonzero(sector[:len(grid)][on] != nominal[on])
        print("n_sectors", n_sectors, "boundary points", int(on.sum()), "in the sector below", int(below))
        assert 0 < below < on.sum()
        assert np.array_equal(sector[:len(grid)][~on], nominal[~on])


def test_stand_alone_host_check_plain_and_under_the_sanitizers():
    """host/scan_context_check.cpp: the rules the kernels run, on the CPU with no library - and once more under ASan / UBSan"""
    plain = subprocess.run([build_check()], capture_output=True, text=True)
    assert plain.returncode == 0 and plain.stdout.splitlines()[-1] == "ok" and "FAILED" not in plain.stdout, plain.stdout + plain.stderr
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", os.devnull], input="int main() { return 0; }\n", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("no -fsanitize=address,undefined runtime for g++ here: the sanitized run does not happen")
    san = subprocess.run([build_check("scan_context_check_san")], capture_output=True, text=True)
    assert san.returncode == 0 and san.stdout == plain.stdout, san.stdout + san.stderr  # (-O2 and no contraction in both: the same figures)


def test_twin_descriptor_and_distances(hip_lib):
    """the twin on inputs whose answer is known: a descriptor from its points' bins, the key distance, rotations, constant and empty descriptors"""
    cloud, sector, ring = si.ringed_cloud(3000, 20, 60, 3)
    for value in (capi.SC_MAX, capi.SC_SUM, capi.SC_COUNT):
        bins, ring_sums, dropped = sc.describe(cloud, n_rings=20, n_sectors=60, max_range=si.MAX_RANGE, value=value)
        want = np.zeros((60, 20), dtype=np.int64)
        v = cloud[:, 2].astype(np.int64)
        {capi.SC_MAX: np.maximum.at, capi.SC_SUM: np.add.at, capi.SC_COUNT: np.add.at}[value](want, (sector, ring), 1 if value == capi.SC_COUNT else v)
        assert np.array_equal(bins, want) and np.array_equal(ring_sums, want.sum(axis=0)) and dropped == 0
    with pytest.raises(ValueError):
        sc.describe(np.zeros((capi.SC_MAX_POINTS + 1, 3), dtype=np.float32))
    assert sc.key_distance([0, 16711680, 5], [16711680, 0, 9]) == 2 * 16711680 ** 2 + 16
    for n_rings, n_sectors in si.SHAPES:
        if n_sectors < 3:
            continue
        b_cloud, _, _ = si.ringed_cloud(max(8, (2 * n_rings * n_sectors) // 5), n_rings, n_sectors, 11)
        b = sc.describe(b_cloud, n_rings=n_rings, n_sectors=n_sectors, max_range=si.MAX_RANGE)[0]
        for m in (1, n_sectors // 2, n_sectors - 1):
            # `to` has turned by +m sector widths against `from`: what it sees stands rotated by -m widths in its frame
            a = sc.describe(si.rotated(b_cloud, -m * 2.0 * math.pi / n_sectors), n_rings=n_rings, n_sectors=n_sectors, max_range=si.MAX_RANGE)[0]
            assert np.array_equal(a, np.roll(b, -m, axis=0)), (n_rings, n_sectors, m)
            d, shift, yaw, margin = sc.distance(a, b)
            assert shift == m and d < 1e-12 and margin > 1e-3, (n_rings, n_sectors, m, d, shift, margin)
            assert abs(yaw - (m if 2 * m <= n_sectors else m - n_sectors) * 2.0 * math.pi / n_sectors) < 1e-12 and -math.pi - 1e-15 < yaw <= math.pi + 1e-15
    flat = np.tile(np.arange(1, 21, dtype=np.uint32), (60, 1))
    assert sc.distance(flat, flat)[:2] == (0.0, 0) or (abs(sc.distance(flat, flat)[0]) < 1e-15 and sc.distance(flat, flat)[1] == 0)
    none = np.zeros((60, 20), dtype=np.uint32)
    assert sc.distance(none, none)[:2] == (1.0, 0) and sc.distance(none, flat)[0] == 1.0
    assert len(sc.candidates(np.stack([none] * 10), max_distance=0.999)) == 0
    same = sc.candidates(np.stack([flat, none, flat, none, flat]), min_index_gap=1, n_keys=0, max_per_node=16)
    assert [(int(c["to"]), int(c["from"])) for c in same] == [(2, 0), (4, 0), (4, 2)]  # ties: the smaller `from` first


def test_device_test_inputs_leave_the_twins_decisions_clear_of_rounding(hip_lib):
    """at most 5 % of what the device tests compare - a candidate list per `to`, a shift per candidate - may rest on a margin below 2 B"""
    total = soft = 0
    for name, nr, ns, sizes, kw in si.MATCH_CASES:
        sets, p, results = si.match_case(name)
        frac, n = si.soft_fraction(results, p)
        print("%-20s %4d decisions, %.4f of them within 2 B, %d candidates" % (name, n, frac, sum(len(r[0]) for r in results)))
        assert n > 0 and frac <= 0.05, name
        assert sum(len(r[0]) for r in results) >= 10, name  # the sets do hold loops
        total, soft = total + n, soft + frac * n
    assert soft / total <= 0.05
    soft = total = 0
    for nr, ns in si.SHAPES:  # ... and of the shifts of the distance pairs
        margins = [sc.distance(a, b)[3] for a, b in si.distance_pairs(nr, ns)]
        total += len(margins)
        soft += sum(m <= 2.0 * sc.rounding_bound(n_rings=nr, n_sectors=ns) for m in margins)
    print("distance pairs: %d shifts, %d within 2 B" % (total, soft))
    assert soft / total <= 0.05


def test_appearance_jobs():
    """`to` is placed on the candidate: the recorded pose of `from`, its angle turned by the match's yaw; otherwise edge_jobs' jobs"""
    rng = np.random.default_rng(4)
    nodes = np.zeros(30, dtype=capi.KEYFRAME_NODE_DTYPE)
    nodes["index"], nodes["pose"] = np.arange(30), rng.normal(size=(30, 3)) * [20.0, 20.0, 1.0]
    cand = np.zeros(5, dtype=capi.SC_CANDIDATE_DTYPE)
    cand["sequence"] = [0, 2, 2, 1, 2]
    cand["to"], cand["from"] = [20, 21, 25, 9, 29], [3, 0, 11, 1, 28]
    cand["shift"] = [0, 5, 59, 30, 31]
    cand["yaw"] = [sc.shift_yaw(int(s), 60) for s in cand["shift"]]
    jobs = replay.appearance_jobs(2, cand, nodes, n_side=1)
    assert jobs.dtype == capi.KEYFRAME_EDGE_JOB_DTYPE and len(jobs) == 3
    plain = replay.edge_jobs(2, [(0, 21), (11, 25), (28, 29)], 1, len(nodes))
    for f in ("sequence", "to", "n_from", "ref", "from"):
        assert jobs[f].tobytes() == plain[f].tobytes(), f
    assert jobs["n_from"].tolist() == [2, 3, 2] and jobs["from"][0][:2].tolist() == [0, 1] and jobs["from"][2][:2].tolist() == [28, 27]  # clipped to the log, never `to`
    assert np.all(jobs["flags"] == 1) and np.all(plain["flags"] == 0)
    for j, c in zip(jobs, cand[[1, 2, 4]]):
        want = nodes["pose"][int(c["from"])] + [0.0, 0.0, float(c["yaw"])]
        assert j["guess_xyt"].tobytes() == want.tobytes()
    assert cand["yaw"][2] < 0.0 < cand["yaw"][1] and abs(cand["yaw"][3] - math.pi) < 1e-15  # (59 of 60 sectors is one sector back)
    assert len(replay.appearance_jobs(3, cand, nodes)) == 0
    # replay_grid: the new spellings are refused or accepted before any device is touched; the existing ones are what they were
    sig = inspect.signature(replay.replay_grid)
    assert list(sig.parameters)[-1] == "optimise" and sig.parameters["edges"].default is None
    frames = np.zeros((1, 4, 8), dtype=np.uint8)
    with pytest.raises(ValueError, match="cells\\+clouds"):
        replay.replay_grid(frames, [capi.Params()], keyframes="cells", edges=dict(appearance={}))
    with pytest.raises(ValueError, match="n_side"):
        replay.replay_grid(frames, [capi.Params()], keyframes="cells+clouds", edges=dict(appearance={}, max_dist=3.0))
    with pytest.raises(ValueError):
        replay.replay_grid(frames, [capi.Params()], keyframes="clouds", edges=dict(min_index_gap=4))
