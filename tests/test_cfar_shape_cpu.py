"""Launch plan of the CA-CFAR detector (csrc/cfar_shape.h: the arithmetic the launcher launches with and cfear_cfar_launch_plan reads back) against
the plans the documents state - include/cfear_hip.h at the declaration, the comment above cfar_detect_owner_kernel - and the conditions on the
case tables and images of tests/test_cfar_layout_gpu.py (tests/cfar_inputs.py): that they reach every launch-dependent feature of the owner-layout
detector the older CA-CFAR tests do not, and that the sensitive images really tell a lost neighbour copy from a kept one. A context needs a GPU,
so here the header is driven by host/cfar_shape_check; the GPU tests assert the same plans through the export before they compare."""
import numpy as np
import pytest

import cfar_inputs as ci


def test_documented_plans():
    p = ci.plan(3360, 40, 10)  # the comment above the kernel: guard 10 / window 40 at 28 bins per thread - r = 6, -10, 10, -6: 48 rows instead of 56
    assert (p["kernel"], p["TB"], p["NW"], p["RS"], p["full"]) == ("owner", 28, 2, 128, 1)
    assert p["cr"] == (6, -10, 10, -6) and p["cq"] == (-2, 0, 0, 2) and p["TB"] + p["rmax"] - p["rmin"] == 48
    assert all(28 * q + r == o for q, r, o in zip(p["cq"], p["cr"], (-50, -10, 10, 50)))
    assert p["lds_bytes"] == 4 * (48 * 128 + 64 * 2 + 2 * 64 + 16) and p["per_cu"] == 6 and p["workgroups"] == 6 * 256 and not p["fill"]
    assert ci.plan(3360, 40, 10, cus=8)["workgroups"] == 48
    # a reach above 128 gives four waves
    assert [(q["TB"], q["NW"]) for q in ci.plans([(3360, 120, 8, 0.01), (3360, 120, 9, 0.01), (3360, 500, 10, 1e-4)])] == [(28, 2), (16, 4), (16, 4)]
    assert [(q["TB"], q["NW"]) for q in ci.plans([(3700, 120, 8, 0.01), (3700, 120, 9, 0.01)])] == [(20, 3), (16, 4)]
    # the four shapes' row lengths: threads x bins per thread just above R
    edges = [(4, (28, 2)), (3580, (28, 2)), (3584, (20, 3)), (3836, (20, 3)), (3840, (16, 4)), (4092, (16, 4)), (4096, (32, 4)), (8188, (32, 4))]
    assert [(q["kernel"], (q["TB"], q["NW"])) for q in ci.plans([(R, 10, 20, 0.01) for R, _ in edges])] == [("owner", s) for _, s in edges]
    # and the way out: rows of 8192 bins and more, rows that are no whole dwords, no integer scale
    assert [q["kernel"] for q in ci.plans([(8192, 10, 20, 0.01), (8196, 10, 20, 0.01), (3361, 10, 20, 0.01), (3362, 10, 20, 0.01), (4097, 10, 20, 0.01)])] == \
        ["fast32", "general", "general", "general", "general"]
    q = ci.plan(3360, ci.NO_SCALE_DETECTOR[0], ci.SCALE_GUARD, ci.NO_SCALE_DETECTOR[1])
    assert q["sh"] < 0 and q["kernel"] == "fast16" and q["workgroups"] > 1 << 20  # (one workgroup per row)
    # the driver's default detector (radar_driver.h:43) at 3580 bins
    d = ci.plan(3580, 10, 20)
    assert (d["TB"], d["NW"], d["RS"], d["padl"], d["rmin"], d["full"], d["fill"]) == (28, 2, 192, 32, -8, 0, 1)
    assert ci.at_risk(d, 3580, 20, 10) == [(3556, 2), (3557, 2), (3558, 2), (3559, 2)]  # the start of the forward window, row e - 8 of column t + 1


def test_the_integer_scale():
    """sh = the largest scale at which the window sums stay below 2^31 and kopen = ceil((1 + 4e-6) 2^sh / (scaling / 2w)) lies in 64 .. 33025"""
    for w, r, sh, kopen in ci.scale_detectors():
        kf = ci.scaling(w, r) * 0.5 / w
        assert kopen == int(np.ceil((1.0 + 4e-6) * 2.0 ** sh / kf)) and 64 <= kopen <= 33025
        assert 2.0 * w * 65025.0 * 2.0 ** sh < 2.0 ** 31
        if sh < 12:
            assert 2.0 * w * 65025.0 * 2.0 ** (sh + 1) >= 2.0 ** 31 or np.ceil((1.0 + 4e-6) * 2.0 ** (sh + 1) / kf) > 33025


def test_case_tables_reach_what_the_older_tests_do_not():
    """every launch-dependent feature of the owner-layout detector, reached by a case of tests/test_cfar_layout_gpu.py - from the check program's output"""
    # every RS = 64 NW + 128 instantiation: {16,4} and {32,4}, FULL and not
    ps = ci.plans([(R, w, g, r) for R, g, w, r in ci.WIDEST])
    assert sorted((p["TB"], p["NW"], p["RS"], p["full"]) for p in ps) == [(16, 4, 384, 0), (16, 4, 384, 1), (32, 4, 384, 0), (32, 4, 384, 1)]
    assert all(p["kernel"] == "owner" for p in ps)
    # LDS above 64 KB (the attribute path): of the row lengths and detectors of the copy-count cases only the {32,4} shape gets there
    assert all(p["kernel"] == "owner" and p["lds_bytes"] > 64 * 1024 and (p["TB"], p["NW"]) == (32, 4) for p in ci.plans([(R, w, g, r) for R, g, w, r in ci.BIG_LDS]))
    assert {p["full"] for p in ci.plans([(R, w, g, r) for R, g, w, r in ci.BIG_LDS])} == {0, 1}
    # too many columns at a dword row length: the round-5 kernels, one window past the widest instantiation
    for R, kernel in ((4092, "fast16"), (8188, "fast32")):
        w, p, prev = ci.just_past_columns(R)
        assert p["kernel"] == kernel and p["sh"] >= 0 and prev["kernel"] == "owner" and prev["RS"] == 64 * 4 + 128
    # every integer scale, sh = 1 among them; no scale at all at a dword row length
    shs = {d[2] for d in ci.scale_detectors()}
    assert shs >= {1} | set(range(3, 13)) and shs == set(range(0, 13))
    assert all(p["kernel"] == "owner" and (p["sh"], p["kopen"]) == d[2:] for d, p in
               zip(ci.scale_detectors(), ci.plans([(ci.SCALE_R, d[0], ci.SCALE_GUARD, d[1]) for d in ci.scale_detectors()])))
    ks = [d[3] for d in ci.scale_detectors()]
    assert min(ks) < 70 and max(ks) > 32000  # (the bounds are 64 and 33025)
    # every neighbour-copy count a shape can take, at a FULL and a not FULL row length
    lo_hi = {28: (22, 10), 20: (16, 7), 16: (12, 6), 32: (25, 12)}
    for TB, (hi, lo) in lo_hi.items():
        his, los, ok = ci.copy_reachable(TB)
        assert (min(his), max(his), min(los), max(los)) == (0, hi, 0, lo) and los == list(range(lo + 1))
        # (rmax takes no value in (TB - rmax_max + ..): the combination with the fewest rows never needs them - e.g. 11 .. 13 at 28 bins per thread)
        assert set(range(hi + 1)) - set(his) == {28: {11, 12, 13}, 20: {8, 9}, 16: {7}, 32: {13, 14, 15}}[TB]
        pairs = ci.copy_pairs(TB)
        assert {c[3] for c in pairs} == set(his) and {-c[2] for c in pairs} == set(los) and len(pairs) <= len(his) + len(los)
        full, part = ci.COPY_ROWS[TB]
        assert full % TB == 0 and part % TB != 0 and part % 4 == 0
        for R in (full, part):
            assert all(p["kernel"] == "owner" and p["TB"] == TB and p["full"] == (R == full) and (p["rmin"], p["rmax"]) == c[2:]
                       for c, p in zip(pairs, ci.plans([(R, c[1], c[0], 0.01) for c in pairs])))
    # the fill loop, on every shape, while thread NT - 1 holds real bytes
    for TB, NW in ci.SHAPES:
        NT = 64 * NW
        table = ci.near_full_pairs(TB, NW)
        assert sorted(table) == sorted(ci.near_full_rows(TB, NW)) and all(TB * (NT - 1) < R < TB * NT for R in table)
        for R, pairs in table.items():
            assert set(ci.REQUIRED_PAIRS.get((TB, NW), [])) <= set(pairs)
            for (g, w), p in zip(pairs, ci.plans([(R, w, g, ci.NEAR_FULL_RATE) for g, w in pairs])):
                assert p["kernel"] == "owner" and (p["TB"], p["NW"]) == (TB, NW) and p["fill"] == 1 and p["full"] == 0
                if R == TB * NT - 4 and (g, w) in ci.REQUIRED_PAIRS.get((TB, NW), []):
                    assert ci.at_risk(p, R, g, w), (R, g, w)
        assert any(ci.at_risk(ci.plan(R, w, g, ci.NEAR_FULL_RATE), R, g, w) for R, pairs in table.items() for g, w in pairs), (TB, NW)
        # R = TB (NT - 1): FULL, thread NT - 1 without bytes, the loop still runs; R = TB NT: the next shape (none beyond 8188 bins)
        e0, e1 = ci.edge_rows(TB, NW)
        p0, p1 = ci.plans([(e0, 10, 20, 0.01), (e1, 10, 20, 0.01)])
        assert (p0["kernel"], p0["TB"], p0["NW"], p0["full"], p0["fill"]) == ("owner", TB, NW, 1, 1)
        assert (p1["kernel"], p1["TB"], p1["NW"]) == {(28, 2): ("owner", 20, 3), (20, 3): ("owner", 16, 4), (16, 4): ("owner", 32, 4), (32, 4): ("fast32", 0, 0)}[(TB, NW)]
    assert [ci.near_full_rows(*s) for s in ci.SHAPES] == [(3580, 3576, 3560), (3836, 3832, 3824), (4092, 4088, 4084), (8188, 8184, 8164)]
    # the loop runs when thread R / TB + ceil(reach / TB) + 1 is the workgroup's last or beyond: the default detector (reach 30: 3 columns) from 124 x 28 bins on
    assert all(ci.plan(R, 10, 20)["fill"] for R in range(3472, 3584, 4)) and not any(ci.plan(R, 10, 20)["fill"] for R in range(3300, 3472, 4))


@pytest.mark.parametrize("TB,NW", ci.SHAPES)
def test_sensitive_images_tell_the_store_orders_apart(TB, NW):
    """in every row of every sensitive image at least one at-risk bin is decided differently by the true threshold and by the threshold with the
    contested bound replaced by the row total; both directions occur; the default detector at 3580 bins is one of the cases"""
    directions, cases = set(), 0
    for R, pairs in ci.near_full_pairs(TB, NW).items():
        for g, w in pairs:
            p = ci.plan(R, w, g, ci.NEAR_FULL_RATE)
            risks = ci.at_risk(p, R, g, w)
            if not risks:
                continue
            built = 0
            for direction in ("false", "missed"):
                s = ci.sensitive_image(p, R, g, w, direction)
                if s is None:
                    continue
                img, targets = s
                assert img.shape == (64, R) and set(targets) <= set(risks)
                hits = ci.detect_rows(img, g, w, ci.NEAR_FULL_RATE, maxd=ci.MAX_DISTANCE.get((TB, NW), 400.0), **ci.NEAR_FULL_GATE)
                for a in range(64):
                    b, c = targets[a]
                    assert ci.sensitive_row_differs(img[a], g, w, ci.NEAR_FULL_RATE, [targets[a]]), (R, g, w, direction, a)
                    assert hits[a, b] == (direction == "missed")  # the true decision: no detection where a false one threatens, one where it would go missing
                directions.add(direction)
                built += 1
            assert built, (R, g, w)
            cases += 1
            if (TB, R, g, w) == (28, 3580, 20, 10):
                assert {t[0] for t in ci.sensitive_image(p, R, g, w, "false")[1]} >= {3558, 3559}
    assert cases >= 2
    if (TB, NW) in ((28, 2), (32, 4)):
        assert directions == {"false", "missed"}


def test_near_ties_lie_on_both_sides():
    """per integer scale: combinations above (detections) and below the threshold; the distances themselves are what the bytes allow (recorded in
    profiles/cfar_layout_tests.txt), only their presence and their sides are asserted; the images carry them with whole windows"""
    for w, r, sh, kopen in ci.scale_detectors():
        above, below = ci.near_ties(w, r)
        assert above and below and all(t[0] > 0 for t in above) and all(-0.5 < t[0] <= 0 for t in below)
        img, da, db, sites = ci.tie_image(ci.SCALE_R, w, ci.SCALE_GUARD, r)
        assert da == above[0][0] and db == below[0][0]
        hits = ci.detect_rows(img, ci.SCALE_GUARD, w, r, 0.0, 0.0)
        span = 2 * (ci.SCALE_GUARD + w) + 1
        bins = 60 + np.arange(sites) * span + ci.SCALE_GUARD + w
        assert bins[-1] + ci.SCALE_GUARD + w <= ci.SCALE_R
        for a in range(img.shape[0]):
            assert [bool(h) for h in hits[a, bins]] == [(a + s) % 2 == 0 for s in range(sites)], (w, r, a)


@pytest.mark.parametrize("R,wave", ci.SPIKE_CASES)
def test_spike_rows_have_the_counts_they_are_named_for(R, wave):
    d = ci.SPIKE_DETECTOR
    p = ci.plan(R, d["window"], d["guard"], d["pfa"])
    assert p["kernel"] == "owner" and wave < p["NW"]
    img, counts = ci.spike_image(R, p["TB"], wave, R)
    hits = ci.detect_rows(img, d["guard"], d["window"], d["pfa"], d["zmin"], d["mind"])
    seg = 64 * p["TB"]
    assert sorted(counts.values()) == list(ci.SPIKE_COUNTS) and {7, 8, 9, 63, 64, 65} <= set(counts.values())
    kinds = set()
    for a in range(img.shape[0]):
        per_seg = [int(hits[a, k * seg:(k + 1) * seg].sum()) for k in range(p["NW"])]
        if a in counts:
            assert per_seg == [counts[a] if k == wave else 0 for k in range(p["NW"])], (a, per_seg)
        else:
            kinds.add("empty" if sum(per_seg) == 0 else "clutter")
            assert sum(per_seg) == 0 or max(per_seg) > 64
    assert kinds == {"empty", "clutter"}


def test_the_definition_in_numpy_is_the_oracles(oracle):
    """detect_rows - what the conditions above are evaluated with - against the oracle's detector, counts per image"""
    for R, g, w, pfa, zmin, mind, maxd in ((777, 20, 10, 0.01, 60.0, 2.5, 400.0), (3580, 0, 150, 0.01, 5.0, 2.5, 400.0), (8188, 20, 70, 0.01, 5.0, 2.5, 600.0)):
        img = ci.random_hot_tail(R, 28, 6, R)
        exp = oracle.cfar(img, ci.RR, zmin, mind, w, g, pfa, maxd, prefix=True)
        hits = ci.detect_rows(img, g, w, pfa, zmin, mind, maxd)
        assert int(hits.sum()) == len(exp) > 100
        assert np.array_equal(exp[:, 2], img[hits].astype(np.float32))


def test_trip_counts():
    W = ci.plan(ci.TRIP_R, 10, 20)["workgroups"]
    assert W == 1536 and ci.plan(ci.TRIP_R, 10, 20)["TB"] == 28
    rows = ci.trip_rows(W)
    assert rows == [1535, 1536, 1537, 4607, 4608, 4609, 6143, 6144, 6145, 9215, 9216, 9217] and max(rows) * ci.TRIP_R <= 7.2e6
