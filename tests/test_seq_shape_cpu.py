"""Per-sequence cost and submap_scan_size (cfear_odometry_set_sequence_shapes), the host-only part: the grid helpers of replay, the two
exports, and the launch-group classification of csrc/seq_groups.h through host/seq_groups_check.

The classification is the one place of the feature that decides which sequences run register_step_kernel, whose per-scan LDS arrays hold
CFEAR_STEP_SMALL_SCANS = 8 scans (the keyframes and the current one): a sequence with submap_scan_size + 1 > 8 must never be in a small
group, whatever the context's submap_scan_size is."""
import os
import re
import subprocess

from cfear_radarodometry_code_public_amd import capi, replay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cfear_radarodometry_code_public_amd", "host")
P2P, P2L, P2D = 0, 1, 2


def small_scans():
    txt = open(os.path.join(ROOT, "cfear_radarodometry_code_public_amd", "csrc", "common.h")).read()
    return int(re.search(r"#define\s+CFEAR_STEP_SMALL_SCANS\s+(\d+)", txt).group(1))


def groups(shapes, small=None):
    """shapes: [(cost, submap_scan_size)] -> dict(launches, large, max_large_submap, groups: [6] dict(cost, small, offset, count), list) or None
    (a shape the header refuses)"""
    subprocess.check_call(["make", "-C", HOST, "seq_groups_check"], stdout=subprocess.DEVNULL)
    args = [str(small_scans() if small is None else small)] + [str(int(v)) for s in shapes for v in s]
    out = subprocess.run([os.path.join(HOST, "seq_groups_check")] + args, capture_output=True, text=True)
    if out.returncode == 1 and out.stdout.strip() == "invalid":
        return None
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    head = lines[0].split()
    res = {"launches": int(head[1]), "large": int(head[3]), "max_large_submap": int(head[5]), "groups": [], "list": [int(v) for v in lines[7].split()[1:]]}
    for g, line in enumerate(lines[1:7]):
        w = line.split()
        assert int(w[1]) == g
        res["groups"].append({"cost": int(w[3]), "small": int(w[5]) == 1, "offset": int(w[7]), "count": int(w[9])})
    return res


def check_partition(shapes, G):
    B = len(shapes)
    assert sorted(G["list"]) == list(range(B))  # every sequence once
    at = 0
    for g in G["groups"]:
        assert g["offset"] == at  # the segments lie back to back, in group order
        seg = G["list"][at:at + g["count"]]
        assert seg == sorted(seg)  # ascending inside a group
        for q in seg:
            cost, s = shapes[q]
            assert cost == g["cost"]
            assert g["small"] == (s + 1 <= 8), (q, s, g)  # stated in numbers: the small kernels hold 8 scans
        at += g["count"]
    assert at == B
    assert G["launches"] == sum(1 for g in G["groups"] if g["count"] > 0)
    large = [s for _, s in shapes if s + 1 > 8]
    assert G["large"] == len(large) and G["max_large_submap"] == (max(large) if large else 0)


def test_no_sequence_of_more_than_seven_keyframes_is_ever_in_a_small_group():
    # the 8 of check_partition is what the small kernels are compiled for, and what the classification is asked with
    assert small_scans() == 8
    txt = open(os.path.join(ROOT, "cfear_radarodometry_code_public_amd", "csrc", "register_step.hip")).read()
    assert re.search(r"#define\s+CFEAR_REG_MAX_SCANS\s+8\b", txt)
    for S in (8, 10, 63):
        for s in (7, 8):
            for cost in (P2P, P2L, P2D):
                # the sequence under test among neighbours of every other kind, at the first, a middle and the last position
                others = [(P2L, 1), (P2D, min(S, 9)), (P2P, 7), (cost, S), (P2L, min(S, 8))]
                for at in (0, 2, len(others)):
                    shapes = others[:at] + [(cost, s)] + others[at:]
                    G = groups(shapes)
                    check_partition(shapes, G)
                    g = [i for i, grp in enumerate(G["groups"]) if at in G["list"][grp["offset"]:grp["offset"] + grp["count"]]]
                    assert len(g) == 1
                    assert G["groups"][g[0]]["small"] == (s == 7), (S, s, cost, at)
                    assert G["groups"][g[0]]["cost"] == cost
    # every s of a 63-keyframe context, one sequence each
    shapes = [(q % 3, s) for q, s in enumerate(range(1, 64))]
    G = groups(shapes)
    check_partition(shapes, G)
    for g in G["groups"]:
        for q in G["list"][g["offset"]:g["offset"] + g["count"]]:
            assert g["small"] == (shapes[q][1] <= 7)
    assert G["large"] == 56 and G["max_large_submap"] == 63


def test_empty_groups_produce_no_launch_and_the_segments_partition_the_batch():
    shapes = [(P2L, 3)] * 5
    G = groups(shapes)
    check_partition(shapes, G)
    assert G["launches"] == 1 and G["list"] == [0, 1, 2, 3, 4] and G["large"] == 0
    # 13 sequences in groups of 1, 5 and 7 with one cost absent (tests/test_seq_shape_gpu.py's fourth test)
    shapes = [(P2D, 7)] + [(P2L, 8)] * 5 + [(P2L, 2)] * 7
    shapes = [shapes[i] for i in (3, 7, 0, 8, 1, 9, 10, 2, 11, 4, 12, 5, 6)]
    G = groups(shapes)
    check_partition(shapes, G)
    assert G["launches"] == 3
    assert sorted(g["count"] for g in G["groups"]) == [0, 0, 0, 1, 5, 7]
    assert all(g["count"] == 0 for g in G["groups"] if g["cost"] == P2P)
    # all six groups
    shapes = [(c, s) for s in (9, 2) for c in (P2D, P2P, P2L)] * 2
    G = groups(shapes)
    check_partition(shapes, G)
    assert G["launches"] == 6 and [g["count"] for g in G["groups"]] == [2] * 6
    G = groups([])
    assert G["launches"] == 0 and G["list"] == []
    # what is no shape is refused, never classified
    assert groups([(P2L, 3), (3, 3)]) is None and groups([(-1, 3)]) is None and groups([(P2L, 0)]) is None


def test_grid_context_params_takes_the_largest_submap_scan_size(hip_lib):
    base = capi.default_params(k_strongest=12, z_min=60.0, res=3.0, submap_scan_size=4, cost=P2D)
    rows = replay.param_grid(base, submap_scan_size=[3, 10, 1], cost=[P2L, P2P], k_strongest=[5, 12])
    before = [bytes(r) for r in rows]
    p = replay.grid_context_params(rows)
    assert (p.submap_scan_size, p.k_strongest, p.cost) == (10, 12, P2L)  # the largest s and k; the cost is rows[0]'s
    assert [bytes(r) for r in rows] == before and p is not rows[0]
    q = capi.Params.from_buffer_copy(rows[0])
    q.submap_scan_size, q.k_strongest = 10, 12
    assert bytes(p) == bytes(q)  # every other field is rows[0]'s


def test_grid_shapes(hip_lib):
    base = capi.default_params(k_strongest=12, res=3.0, submap_scan_size=4, cost=P2L)
    same = replay.param_grid(base, res=[2.5, 3.5], loss=[1, 2])
    assert replay.grid_shapes(same, replay.grid_context_params(same)) is None  # uniform rows: no shapes
    assert replay.grid_shapes(iter(same), base) is None  # (any iterable)
    other = capi.Params.from_buffer_copy(base)
    other.submap_scan_size = 5
    assert [(s.cost, s.submap_scan_size) for s in replay.grid_shapes(same, other)] == [(P2L, 4)] * 4  # uniform, but not the context's
    # param_grid's order: cost outside submap_scan_size outside res (utils/worker:49-58), whatever order the axes are given in
    rows = replay.param_grid(base, res=[2.5, 3.5], submap_scan_size=[1, 2, 3], cost=[P2P, P2L, P2D])
    ctxp = replay.grid_context_params(rows)
    assert (ctxp.cost, ctxp.submap_scan_size) == (P2P, 3)
    shapes = replay.grid_shapes(rows, ctxp)
    assert all(isinstance(s, capi.SeqShape) for s in shapes)
    assert [(s.cost, s.submap_scan_size) for s in shapes] == [(c, s) for c in (P2P, P2L, P2D) for s in (1, 2, 3) for _ in (2.5, 3.5)]
    assert [r.res for r in rows[:4]] == [2.5, 3.5, 2.5, 3.5]
    # the reference's params/submap_keyframes/submap_keyframe_cfear-3: 30 jobs
    rows = replay.param_grid(base, cost=[P2P, P2L, P2D], submap_scan_size=range(1, 11))
    shapes = replay.grid_shapes(rows, replay.grid_context_params(rows))
    assert len(shapes) == 30 and (shapes[0].cost, shapes[0].submap_scan_size) == (P2P, 1) and (shapes[29].cost, shapes[29].submap_scan_size) == (P2D, 10)
    assert replay.grid_context_params(rows).submap_scan_size == 10


def test_both_symbols_are_declared_and_exported(hip_lib):
    txt = open(os.path.join(ROOT, "include", "cfear_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"typedef\s+struct\s+cfear_seq_shape\s*\{\s*int32_t\s+cost;\s*int32_t\s+submap_scan_size;\s*\}\s*cfear_seq_shape;", code)
    assert re.search(r"int\s+cfear_odometry_set_sequence_shapes\s*\(\s*cfear_ctx\*[^,]*,\s*cfear_odometry\*[^,]*,\s*const\s+cfear_seq_shape\*[^,]*,\s*int\s+n_rows\s*\)\s*;", code)
    assert re.search(r"int\s+cfear_odometry_sequence_shape\s*\(\s*cfear_ctx\*[^,]*,\s*cfear_odometry\*[^,]*,\s*int\s+sequence\s*,\s*cfear_seq_shape\*[^,]*\)\s*;", code)
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path()]).decode()
    exported = [l.split()[-1] for l in out.splitlines() if " T " in l]
    for name in ("cfear_odometry_set_sequence_shapes", "cfear_odometry_sequence_shape"):
        assert name in exported and name in capi.EXPORTS and hasattr(hip_lib, name)
    import ctypes as C
    assert C.sizeof(capi.SeqShape) == 8 and capi.SeqShape.submap_scan_size.offset == 4
