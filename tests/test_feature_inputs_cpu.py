"""The clouds of feature_inputs.py have the properties they are named after (no GPU): what test_feature_seams_gpu.py feeds the feature
build sits AT the limits of features_compact_dev.h, by the numpy twin of its bookkeeping (plan) and, where it can speak, by the oracle.
Without this file the GPU tests could pass on clouds that never reach the branch they mean."""
import os
import re

import numpy as np
import pytest

import feature_inputs as fi

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cfear_radarodometry_code_public_amd", "csrc")
NAMES = list(fi.CASES)


def _define(text, name):
    m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, text, re.M)
    assert m, name
    return int(m.group(1))


def _eval(expr, env):
    """a constant expression of the headers (names, integers, + - * /, sizeof of a scalar type) as an integer"""
    expr = re.sub(r"sizeof\((\w+)\)", lambda m: str({"int": 4, "float": 4, "double": 8}[m.group(1)]), expr)
    expr = re.sub(r"\(\s*(?:int|size_t)\s*\)", "", expr)
    expr = re.sub(r"(?:FeatLdsC::)?([A-Za-z_]\w*)", lambda m: str(env[m.group(1)]), expr)
    assert re.fullmatch(r"[\d\s+\-*/()]+", expr), expr
    return int(eval(expr.replace("/", "//")))


def test_the_limits_are_the_headers():
    """the numbers feature_inputs.py works with, recomputed from the headers: the #define values, the constexpr offsets of FeatLdsC evaluated in
    order, and the constant expressions of the four places that derive a limit from them. A later change of a limit fails here instead of
    leaving the cases at the old value"""
    compact = open(os.path.join(CSRC, "features_compact_dev.h")).read()
    general = open(os.path.join(CSRC, "features_dev.h")).read()
    step = open(os.path.join(CSRC, "odometry_step_dev.h")).read()
    env = {"CFEAR_CPT_CAP": _define(compact, "CFEAR_CPT_CAP"), "CFEAR_CPT_VOXELS": _define(compact, "CFEAR_CPT_VOXELS"),
           "CFEAR_FEAT_BLOCK": _define(general, "CFEAR_FEAT_BLOCK"), "CFEAR_PT": _define(general, "CFEAR_PT")}
    assert (env["CFEAR_CPT_CAP"], env["CFEAR_CPT_VOXELS"], env["CFEAR_FEAT_BLOCK"], env["CFEAR_PT"]) == (fi.CPT_CAP, fi.CPT_VOXELS, fi.FEAT_BLOCK, fi.PT) == (4864, 32768, 512, 10)
    body = re.search(r"struct FeatLdsC \{(.*?)\n\};", compact, re.S).group(1)
    for name, expr in re.findall(r"static constexpr size_t (\w+) = ([^;]+);", body):
        env[name] = _eval(expr, env)
    assert env["total"] <= 80384
    lm = re.search(r"constexpr int LM_CAP = ([^;]+);", compact).group(1)
    assert fi.LM_CAP == _eval(lm, env) == 772
    sets = re.search(r"8 \* VS <= (\(int\)\([^)]*\))", compact).group(1)
    assert fi.CW_HALVES == _eval(sets, env) == 19456
    tab = re.search(r"tab_voxels = ([^;]+);", compact).group(1)
    div = re.search(r"G \+ 1 <= W\.tab_voxels / (\d+)", general).group(1)
    assert fi.GRID_LDS == _eval(tab, env) // int(div) == 9728
    bearings = re.search(r"\(int\)\((CFEAR_CPT_CAP \* \d+ / \(\d+ \* sizeof\(double\)\))\)", step).group(1)
    assert fi.BEARINGS == _eval(bearings, env) == 810
    assert fi.REG_POINTS == env["CFEAR_FEAT_BLOCK"] * env["CFEAR_PT"] == 5120


def test_every_case_of_the_list_is_there():
    want = ["n=%d" % n for n in (4863, 4864, 4865, 512, 513, 4608, 4609, 5120, 5121)]
    want += ["G=32768=256x128", "G=32768=128x256", "G=32768=32768x1", "G=32896=257x128", "G=32896=128x257"] + ["G=%d" % g for g in (31, 32, 33, 63, 64, 65)]
    want += ["nv=%d" % v for v in (2430, 2431, 2432, 2433)] + ["nv=n", "nv=1", "dark-nv=2431", "rows=4and5"]
    want += ["chunks-%s-%s" % (k, c) for c in ("4864", "own") for k in ("listed", "unlisted", "c32", "c64")]
    want += ["runs", "cells=771", "cells=772", "cells=773", "buckets+1=9728", "buckets+1=9729"]
    assert sorted(want) == sorted(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_the_case_is_what_its_name_says(oracle, name):
    c = fi.case(name)
    P = c.check()  # every claimed value, exactly, by the twin
    assert fi.pinned(c) == fi.PINNED[name], (name, fi.pinned(c))  # n, G, nv, C, NC, NA, listed against the case's ccap; C, listed against n points
    print("[plan] %s: n %d, grid %d x %d = %d, nv %d, %d counter set(s), rows %s, C %d, NC %d, NA %d, listed %s, %s path, %d cells"
          % (name, P.n, P.div0, P.div1, P.G, P.nv, P.sets, sorted(set(P.rows.tolist())), P.C, P.NC, P.NA, P.listed, P.path, c.cells))
    key, _, val = name.partition("=")
    if key == "n":
        assert P.n == int(val) and P.path == ("compact" if P.n <= fi.CPT_CAP else "general") and P.rounds == (-(-P.n // 512) if P.n <= fi.REG_POINTS else 0)
    if key == "G":
        g = int(val.split("=")[0])
        assert P.G == g and P.path == ("compact" if g <= fi.CPT_VOXELS else "general")
        if "x" in val:
            assert "%dx%d" % (P.div0, P.div1) == val.split("=")[1]
        assert P.extra_word == (g % 32 == 0)
        assert P.voxel[-1] == P.G - 1  # the highest voxel is occupied
    if key in ("nv", "dark-nv") and val.isdigit():
        assert P.nv == int(val) and P.sets == (8 if P.nv <= 2431 else 1) and P.odd_nv == bool(int(val) & 1) and P.path == "compact"
    if name == "nv=n":
        assert P.nv == P.n and (P.count == 1).all()
    if name.startswith("chunks"):
        kind, cap = name.split("-")[1:]
        assert c.ccap == (fi.CPT_CAP if cap == "4864" else c.n) and P.n <= c.ccap
        c16 = int((-(-np.where(P.tot >= 6, P.tot, 0) // 16)).sum())
        c32 = int((-(-np.where(P.tot >= 6, P.tot, 0) // 32)).sum())
        if kind == "listed":
            assert P.listed and P.C == 16 and P.NC + P.NA == c.ccap
        elif kind == "unlisted":
            assert not P.listed and P.C == 16 and P.NC + P.NA == c.ccap + 1 and P.NC <= c.ccap
        elif kind == "c32":
            assert not P.listed and P.C == 32 and c16 == c.ccap + 1
        else:
            assert not P.listed and P.C == 64 and c32 > c.ccap >= P.NC
        assert not P.any_big
    if name == "runs":
        for kind, mk in fi.run_kinds(P).items():
            assert mk.any(), kind
        assert set(fi.run_kinds(P)) == set(fi.RUN_KINDS)
    # the oracle: as many samples as occupied voxels, the centroids bit for bit
    scan = fi.oracle_scan(c.xyi, c.res, c.df)
    samples = scan.samples()
    assert len(samples) == P.nv
    assert np.array_equal(samples.view(np.uint32), P.cen.view(np.uint32))
    cells = scan.cells()
    assert scan.size == c.cells == len(cells)
    if key == "cells":
        assert scan.size == int(val)
        assert (scan.size <= fi.LM_CAP) == (int(val) <= 772)
    if key == "buckets+1":
        gw, gh = fi.cell_grid_shape(cells)[:2]
        assert gw * gh + 1 == int(val) == c.buckets + 1 and (gw * gh + 1 <= fi.GRID_LDS) == (int(val) == 9728)
    if c.min_cells is None:
        assert scan.size == 1  # the degenerate case: one voxel, one cell
    else:
        assert scan.size >= 30
    # at least one cell is made at the seam (all of them where the case says so)
    made = np.zeros(P.nv, dtype=bool)
    made[fi.cell_samples(P, cells, c.res)] = True
    seam = c.seam(P)
    assert seam.any() and (made & seam).any(), name
    if c.seam_all:
        assert made[seam].all(), name
    if name == "rows=4and5":
        assert (made & P.stored & (P.rows == 4)).any() and (made & ~P.stored & (P.rows == 5)).any()
    if key == "G" and P.extra_word:
        assert (made & (P.gx1 == P.div0 - 1) & (P.gy1 == P.div1 - 1)).any()  # a cell whose candidates include the last voxel: rank(G) reads the extra word


def test_zero_weights_do_not_change_the_bookkeeping():
    a, b = fi.case("nv=2431"), fi.case("dark-nv=2431")
    assert np.array_equal(a.xyi[:, :2], b.xyi[:, :2]) and (b.xyi[:, 2] <= 60).sum() > 1000 and (a.xyi[:, 2] > 60).all()
    Pa, Pb = a.plan(), b.plan()
    for k in ("n", "G", "nv", "sets", "C", "NC", "NA", "listed", "path"):
        assert getattr(Pa, k) == getattr(Pb, k), k
    for k in ("tot", "m", "rows", "run_start", "run_len"):
        assert np.array_equal(getattr(Pa, k), getattr(Pb, k)), k


def test_the_twin_counts_the_neighbours_the_oracle_counts():
    """plan's m (float32 distances, strict <) is the oracle's nsamples for every cell of a dense cloud"""
    c = fi.case("rows=4and5")
    P = c.plan()
    cells = fi.oracle_scan(c.xyi, c.res, c.df).cells()
    v = fi.cell_samples(P, cells, c.res)
    assert len(v) == len(cells) > 1000 and np.array_equal(P.m[v], cells["nsamples"])


def test_the_batched_objects_capacity_moves_the_chunk_list_switch():
    """the same cloud against 4864 and against its own size: the own-size cases are at the switch only for a caller sized for exactly n points"""
    c = fi.case("chunks-listed-own")
    assert c.plan(fi.CPT_CAP).listed and c.plan(c.n).listed and not c.plan(c.n - 1).listed
    c = fi.case("chunks-unlisted-own")
    assert c.plan(fi.CPT_CAP).listed and not c.plan(c.n).listed and c.plan(c.n + 1).listed


@pytest.mark.parametrize("name", list(fi.SLOT_CASES))
def test_the_sweeps_keep_the_slots_their_name_says(oracle, name):
    """the polar sweeps of the slot route, by the oracle's filter and the twin on the filtered cloud, sweep by sweep: every slot kept (A * k points, on
    either side of 4864 and of 5120; 810 and 811 bearings; a register round that fills exactly and one bearing more), an exact n of 4872 slots,
    an exact nv, or the world's own ragged bearings and a second z_min that drops more"""
    c = fi.SLOT_CASES[name]
    A, k = c.A, c.k
    imgs = fi.slot_sweeps(name)
    assert imgs.shape == (fi.SLOT_T, A, fi.SLOT_R)
    key, _, val = name.partition("=")
    if key == "A":
        assert A == int(val) and A * k <= fi.CPT_CAP and (A <= fi.BEARINGS) == (int(val) == 810)
    if key == "slots":
        assert A * k == int(val) == c.n
    if key == "n":
        assert c.n == int(val.split("of")[0]) and A * k == int(val.split("of")[1]) == 4872 and -(-A * k // 512) == fi.PT
    for t in range(fi.SLOT_T):
        cl = fi.slot_cloud(imgs[t], k)
        P = fi.plan(cl, 3.0, 1.0, A * k)
        per_bearing = (fi.oracle.unpack_slots(fi.oracle.filter_polar(imgs[t], 60, k))["valid"]).sum(axis=1)
        assert per_bearing.sum() == len(cl)  # a point per kept slot
        if c.full:
            assert len(cl) == c.n == A * k - c.drop
            assert (per_bearing == k - 1).sum() == c.drop and (per_bearing >= k - 1).all()  # ragged ballots in exactly `drop` bearings
            assert P.path == ("compact" if c.n <= fi.CPT_CAP else "general")
            if c.nv:
                assert P.nv == c.nv and P.sets == (8 if c.nv <= 2431 else 1) and P.n == fi.CPT_CAP
        else:
            assert (per_bearing < k).sum() > A // 4 and (per_bearing == k).any()  # full and partly empty bearings
            high = fi.slot_cloud(imgs[t], k, fi.HOLES_Z[1])
            assert 30 * k < len(high) < len(cl) - 100 and len(cl) < A * k - 100 and P.path == "compact"
        assert fi.oracle_scan(cl, 3.0, 1.0).size >= 30


def test_the_slot_cases_cover_what_a_polar_image_can_produce():
    want = ["A=810", "A=811", "slots=4864", "slots=4872", "slots=5120", "slots=5128", "holes"]  # h
    want += ["n=4863of4872", "n=4864of4872", "n=4865of4872", "slots=512", "slots=520", "slots=4608", "slots=4616"]  # a
    want += ["slots-nv=2431", "slots-nv=2432"]  # c
    assert sorted(want) == sorted(fi.SLOT_CASES)
