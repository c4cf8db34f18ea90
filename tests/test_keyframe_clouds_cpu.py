"""The keyframe log's point clouds (cfear_odometry_set_keyframe_clouds) without a GPU: the crafted first sweeps of tests/test_keyframe_clouds_gpu.py
hit the kept-point totals they are meant to hit - asserted on the ORACLE's slots, so a case cannot miss its edge silently -, the .npz of
replay.write_keyframe_clouds reads back bit for bit, and the public constants agree between the header and the binding.

A crafted image is zeros plus single pixels. A pixel at least 7 range bins from every other one is a peak of AxialNonMaxSupress (its 7-bin
window sum equals that of its three neighbours on either side: radar_filters.cpp:282 keeps it); the two pixels of a pair (m, m + 4) are
both suppressed (the window sums at m + 1 and m + 3 hold both). Bearings are filled to k before the next one starts, so the kept points
are the logical items 0 .. n - 1 of the cloud pass and a total of n puts the last point on the wave / round boundary the case is named for."""
import math
import os
import re

import numpy as np
import pytest

from cfear_radarodometry_code_public_amd import capi, replay

RR = np.float32(0.0595238)
MIN_DISTANCE = 2.5
Z_MIN = 60
GATE = int(math.ceil(float(np.float32(MIN_DISTANCE)) / float(RR)))  # radar_filters.cpp:315: points at range <= GATE are dropped
R0, STEP = 64, 8  # first range bin of the crafted returns (beyond the gate), bins between isolated returns
SHAPES = [(16, 512, 12), (16, 512, 40), (400, 3360, 12), (400, 3360, 40)]  # (A, R, k): k = 40 at A = 400 is the general branch of cloud_step_block
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rounds(A, k):
    """rounds of 64 items a wave of the 512-thread cloud pass takes (features_dev.h: RC)"""
    return (A * k + 511) // 512


def edge_totals(A, k):
    rc = rounds(A, k)
    want = {0, 1, 63, 64, 65, rc * 64 - 1, rc * 64, rc * 64 + 1, 511, 512, 513}
    return sorted(v for v in want if v <= A * k)


def isolated(A, R, k, n, pairs=0):
    """n returns that are all peaks, bearing after bearing, then `pairs` pairs of returns that are all suppressed"""
    assert R0 > GATE + 3 and R0 + STEP * k + 8 < R and n + 2 * pairs <= A * k
    img = np.zeros((A, R), dtype=np.uint8)
    for i in range(n):
        img[i // k, R0 + STEP * (i % k)] = 70 + (i * 37) % 180
    for p in range(pairs):
        i = n + (-n % 2) + 2 * p  # (pairs start on an even slot: a pair never straddles two bearings)
        b, j = i // k, i % k
        img[b, R0 + STEP * j] = 70 + (p * 11) % 90
        img[b, R0 + STEP * j + 4] = 160 + (p * 7) % 90
    return img


def crafted(A, R, k):
    """-> list of (name, image [A, R], points of the filtered cloud, points of the peaks cloud) - the last two as intended"""
    out = [("n=%d" % n, isolated(A, R, k, n), n, n) for n in edge_totals(A, k)]
    out.append(("one per bearing", np.where(np.arange(R)[None, :] == R0 + 3 * (np.arange(A)[:, None] % 50), 200, 0).astype(np.uint8), A, A))
    out.append(("saturated", np.full((A, R), 255, dtype=np.uint8), A * k, None))  # every slot valid (the peaks are the oracle's)
    full = np.zeros((A, R), dtype=np.uint8)  # a full filtered cloud of suppressed pairs: no peaks at all
    for j in range(k // 2):
        full[:, R0 + 16 * j] = 80 + 3 * j
        full[:, R0 + 16 * j + 4] = 150 + 2 * j
    out.append(("full, no peaks", full, A * k, 0))
    out.append(("mixed", isolated(A, R, k, 65, pairs=32), 129, 65))  # both kinds in one sweep: the two clouds differ in size
    gate = np.zeros((A, R), dtype=np.uint8)  # the three weakest returns of four bearings lie in front of the gate: valid slots, no points
    for b in range(4):
        for j, r in enumerate((8, 16, 24)):
            gate[b, r] = 61 + j
        gate[b, GATE] = 66  # (the gate itself is dropped: range > GATE)
        for j in range(5):
            gate[b, GATE + 1 + STEP * j] = 100 + 10 * j + b
    out.append(("gate", gate, 20, 20))
    return out


def oracle_clouds(oracle, img, k, motion=(0.0, 0.0, 0.0), ccw=0, z_min=Z_MIN, compensate=True):
    """the expected value of both clouds: filter_polar -> cloud -> compensate (odometrykeyframefuser.cpp:147-149) -> (slots, cloud, peaks)"""
    slots = oracle.filter_polar(img, z_min, k)
    both = []
    for peaks in (False, True):
        c = oracle.cloud(slots, RR, np.float32(MIN_DISTANCE), peaks)
        both.append(oracle.compensate(c, motion, ccw) if compensate else c)
    return slots, both[0], both[1]


@pytest.mark.parametrize("A,R,k", SHAPES)
def test_crafted_sweeps_hit_their_totals(oracle, A, R, k):
    cases = crafted(A, R, k)
    names = [c[0] for c in cases]
    rc = rounds(A, k)
    for n in (0, 1, 63, 64, 65, rc * 64 - 1, rc * 64, rc * 64 + 1):
        assert "n=%d" % n in names or n > A * k
    assert (rc <= 10) == ((A, k) != (400, 40))  # k = 40 at 400 azimuths is the only shape here beyond the register branch (CFEAR_PT = 10)
    for name, img, want, want_peaks in cases:
        slots, cloud, peaks = oracle_clouds(oracle, img, k)
        valid = (slots >> 24) & 1
        kept = valid & ((slots & 0xFFFF) > GATE)
        assert len(cloud) == int(kept.sum()) == want, (name, len(cloud), want)
        assert len(peaks) == int((kept & (slots >> 25) & 1).sum())
        if want_peaks is not None:
            assert len(peaks) == want_peaks, (name, len(peaks), want_peaks)
        if name == "saturated":
            assert valid.all()
        if name == "gate":
            assert int(valid.sum()) == 4 * 9 and int(kept.sum()) == 20 and (valid[:4, :4] == 1).all() and not kept[:4, :4].any()  # dropped at the FRONT of the bearing
        if name.startswith("n=") and want > 0:  # bearings fill up in turn: the points are the items 0 .. n - 1
            assert kept.reshape(-1)[:want].all()
        # zero motion leaves every bit where it was: the first keyframe's clouds are bit-exact with compensation on
        assert cloud.tobytes() == oracle.cloud(slots, RR, np.float32(MIN_DISTANCE), False).tobytes()


def test_npz_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    clouds = [[rng.normal(size=(n, 3)).astype(np.float32) for n in (5, 0, 17)], [], [rng.normal(size=(1, 3)).astype(np.float32)]]
    peaks = [[c[::2] for c in lst] for lst in clouds]
    clouds[0][0][0, 0] = np.float32(np.nan)  # bits, not values
    for pk in (peaks, None):
        path = tmp_path / ("clouds_%d.npz" % (pk is not None))
        replay.write_keyframe_clouds(path, clouds, pk)
        back, back_pk = replay.read_keyframe_clouds(path)
        assert [len(lst) for lst in back] == [3, 0, 1]
        for q, lst in enumerate(clouds):
            for i, c in enumerate(lst):
                assert back[q][i].dtype == np.float32 and back[q][i].shape == c.shape and back[q][i].tobytes() == c.tobytes()
        if pk is None:
            assert back_pk is None
        else:
            assert all(back_pk[q][i].tobytes() == c.tobytes() for q, lst in enumerate(pk) for i, c in enumerate(lst))
    with pytest.raises(ValueError):
        replay.write_keyframe_clouds(tmp_path / "bad.npz", clouds, peaks[:2])


def test_constants_and_entries_of_the_header():
    txt = open(os.path.join(ROOT, "include", "cfear_hip.h")).read()
    defs = dict(re.findall(r"#define (CFEAR_KF_[A-Z]+) (\d+)", txt))
    assert {k: int(v) for k, v in defs.items()} == {"CFEAR_KF_NODES": capi.KF_NODES, "CFEAR_KF_CELLS": capi.KF_CELLS, "CFEAR_KF_CLOUD": capi.KF_CLOUD,
                                                    "CFEAR_KF_PEAKS": capi.KF_PEAKS}
    assert (capi.KF_CLOUD, capi.KF_PEAKS) == (4, 8) and capi.KEYFRAME_NODE_DTYPE.itemsize == 376  # the node keeps its layout: sizes travel beside it
    for name in ("cfear_odometry_set_keyframe_clouds", "cfear_odometry_keyframe_cloud_sizes", "cfear_odometry_keyframe_cloud", "cfear_odometry_keyframe_clouds"):
        assert name in capi.EXPORTS and re.search(r"\bint %s\(" % name, txt)
    import inspect
    sig = inspect.signature(capi.Odometry.record_keyframes)
    assert sig.parameters["max_points"].default == 0 and list(sig.parameters)[1:4] == ["what", "max_keyframes", "max_cells"]  # every existing call stays as it is


def test_command_line_refuses_clouds_without_a_graph():
    with pytest.raises(SystemExit):
        replay.main(["--oxford_png_dir", "nowhere", "--store_clouds", "c.npz"])
