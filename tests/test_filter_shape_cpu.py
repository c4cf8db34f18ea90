"""Launch shape of the k-strongest filter (csrc/kstrongest_shape.h: the arithmetic cfear_launch_kstrongest launches with and
cfear_kstrongest_launch_shape reads back) against the shapes the documents state - include/cfear_hip.h at the declaration, the comment
at the arithmetic itself: never against a run of the helper. A context needs a GPU, so here the header is driven by
host/filter_shape_check; tests/test_kstrongest_gpu.py pins the same values through the export."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cfear_radarodometry_code_public_amd", "host")


def shapes(*queries):
    """queries: (A, R, n_scans, occupancy knob, rows knob) -> [(rows_per_wave, workgroups, occupancy, nch)]"""
    subprocess.check_call(["make", "-C", HOST, "filter_shape_check"], stdout=subprocess.DEVNULL)
    args = [str(int(v)) for q in queries for v in q]
    out = subprocess.run([os.path.join(HOST, "filter_shape_check")] + args, capture_output=True, text=True, check=True)
    res = [tuple(int(v) for v in line.split()) for line in out.stdout.splitlines()]
    assert len(res) == len(queries)
    return res


def ceil_div(a, b):
    return -(-a // b)


def test_documented_shapes():
    (r4608, w4608, o, nch), (r1535, w1535, *_), (r1536, w1536, *_), (r5, w5, *_) = shapes(
        (400, 3360, 4608, 7, 0), (400, 3360, 1535, 7, 0), (400, 3360, 1536, 7, 0), (400, 3360, 5, 7, 0))
    assert (r4608, r1535, r1536, r5) == (6, 4, 6, 1)  # the benchmark's launch; the default cap is 4, and 6 from 1536 scans up; 2000 rows < 7168 slots
    assert (o, nch) == (7, 4)
    # workgroups = ceil(ceil(n_rows / rows) / 4): four waves per workgroup
    assert w4608 == ceil_div(ceil_div(4608 * 400, 6), 4) == 76800
    assert w1535 == ceil_div(ceil_div(1535 * 400, 4), 4) and w1536 == ceil_div(ceil_div(1536 * 400, 6), 4) and w5 == 500


def test_a_wave_gets_r_rows_once_the_rows_exceed_r_minus_1_times_the_slots():
    """rows_per_wave = min(cap, ceil(n_rows / (1024 * occupancy))), with partial last waves and workgroups counted"""
    for occ in (5, 6, 7):
        slots = 1024 * occ
        q, exp = [], []
        for r in (1, 2, 3, 5, 8):
            for n_rows in ((r - 1) * slots + 1, r * slots):  # A = 1: n_scans = n_rows
                if n_rows >= 1:
                    q.append((1, 64, n_rows, occ, 8))
                    exp.append((r, ceil_div(ceil_div(n_rows, r), 4), occ, 4))
        assert shapes(*q) == exp
    # A = 7: 731 scans = 5117 rows fit the 5120 slots of occupancy 5, 732 scans = 5124 rows do not
    assert [s[0] for s in shapes((7, 37, 731, 5, 8), (7, 37, 732, 5, 8))] == [1, 2]


def test_the_rows_knob_is_a_cap_and_only_lowers():
    n = 4608
    got = [s[0] for s in shapes(*[(400, 3360, n, 7, cap) for cap in (0, 1, 2, 3, 6, 8, 12, 300)])]
    assert got == [6, 1, 2, 3, 6, 8, 12, 258]  # ceil(4608 * 400 / 7168) = 258 rows would fill every slot once
    # a small launch stays at one row per wave whatever the cap; negative values mean "no knob"
    assert [s[0] for s in shapes((400, 3360, 2, 7, 1), (400, 3360, 2, 7, 8), (400, 3360, 2, 7, 4), (400, 3360, 2, 7, -3))] == [1, 1, 1, 1]
    assert [s[0] for s in shapes((400, 3360, 100, 7, 0), (400, 3360, 100, 7, 5), (400, 3360, 100, 7, 8))] == [4, 5, 6]  # 40000 rows: ceil = 6


def test_occupancy_variants():
    # the knob picks one of three builds of the 4 KiB-window kernel; longer rows have one build each (R + 27 bytes must fit the window)
    assert [s[2:4] for s in shapes(*[(400, 3360, 64, occ, 0) for occ in (-1, 0, 4, 5, 6, 7, 8, 100)])] == \
        [(5, 4), (5, 4), (5, 4), (5, 4), (6, 4), (7, 4), (7, 4), (7, 4)]
    assert [s[2:4] for s in shapes((9, 4069, 9, 7, 0), (9, 4070, 9, 7, 0), (9, 5000, 9, 7, 0), (9, 8165, 9, 5, 0), (9, 8166, 9, 7, 0),
                                   (9, 9000, 9, 6, 0), (9, 16357, 9, 7, 0))] == [(7, 4), (3, 8), (3, 8), (3, 8), (2, 16), (2, 16), (2, 16)]
    assert shapes((9, 16358, 9, 7, 0))[0][3] == 0  # no kernel: the launcher and the read-back refuse
    # the slots follow the occupancy: 9 x 5000 needs more than 3072 rows for two per wave, 9 x 9000 more than 2048
    assert [s[0] for s in shapes((9, 5000, 341, 7, 0), (9, 5000, 342, 7, 0), (9, 9000, 227, 7, 0), (9, 9000, 228, 7, 0))] == [1, 2, 1, 2]

