"""What a batched odometry object is sized and scheduled by (csrc/odometry_plan.h) through host/odometry_plan_check: the compute-unit
masks of cfear_tune FILTER_CUS, the replay's chunk size, the capacities and the overlap clamp - without a GPU.

The expectations are worked out by hand from the rules as cfear_odometry_create and the replay have always applied them (stated with
each table), not taken from the header under test. Every case runs through the plain build and through an -fsanitize=address,undefined
build of the same program (a stand-alone program on the CPU; where the sanitizer runtime is missing that half is skipped)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cfear_radarodometry_code_public_amd", "host")
MiB = 1 << 20


def _sanitizer_runtime():
    src = os.path.join(HOST, "_san_probe_plan.cpp")
    exe = os.path.join(HOST, "_san_probe_plan")
    try:
        with open(src, "w") as f:
            f.write("int main() { return 0; }\n")
        ok = subprocess.run(["g++", "-fsanitize=address,undefined", "-o", exe, src], capture_output=True).returncode == 0
        return ok and subprocess.run([exe], capture_output=True).returncode == 0
    finally:
        for p in (src, exe):
            if os.path.exists(p):
                os.remove(p)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def prog(request):
    target = "odometry_plan_check" if request.param == "plain" else "odometry_plan_check_san"
    if request.param == "sanitized" and not _sanitizer_runtime():
        pytest.skip("no -fsanitize=address,undefined runtime for g++ here: the sanitized half of the cases does not run")
    subprocess.check_call(["make", "-C", HOST, target], stdout=subprocess.DEVNULL)
    return os.path.join(HOST, target)


def run(prog, *commands):
    """one output line (split into words) per command, each command a tuple of words"""
    out = subprocess.run([prog] + [str(w) for c in commands for w in c], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", (out.returncode, out.stderr)  # (a sanitizer report is on stderr and in the exit status)
    lines = [l.split() for l in out.stdout.splitlines()]
    assert len(lines) == len(commands) and all(l[0] == c[0] for l, c in zip(lines, commands))
    return lines


def masks(prog, *cases):
    """[(filter mask, odometry mask, words)] as integers (bit i = compute unit i) of (ncu, filter_cus) cases"""
    out = []
    for l in run(prog, *[("masks", ncu, f) for ncu, f in cases]):
        w = int(l[1])
        assert l[2] == "f" and l[3 + w] == "o" and len(l) == 4 + 2 * w
        val = lambda words: sum(int(x, 16) << (32 * i) for i, x in enumerate(words))
        out.append((val(l[3:3 + w]), val(l[4 + w:]), w))
    return out


def bits(lo, hi):
    return ((1 << (hi - lo)) - 1) << lo


def group(g):
    return bits(8 * g, 8 * g + 8)


# ---- compute-unit masks: groups of 8 bits; gf = max(1, min(groups - 1, (F + 4) / 8)) groups for the filter, taken in the order
# 0, 4, 8, ... then 2, 6, ... then 1, 5, ... then 3, 7, ...; the other groups and the bits past the last whole group for the odometry
def test_masks_256_units_32_for_the_filter(prog):
    (f, o, w), = masks(prog, (256, 32))
    assert w == 8
    assert f == group(0) | group(4) | group(8) | group(12)
    assert [(f >> (32 * i)) & 0xFFFFFFFF for i in range(8)] == [0xFF] * 4 + [0] * 4
    assert o == bits(0, 256) & ~f


def test_masks_round_up_to_one_group(prog):
    (f, o, w), = masks(prog, (256, 1))
    assert (f, o, w) == (group(0), bits(8, 256), 8)


def test_masks_leave_the_odometry_one_group(prog):
    (f, o, w), = masks(prog, (256, 1000))
    assert o == bits(248, 256)  # group 31: the last of the spread order
    assert f == bits(0, 248) and w == 8


@pytest.mark.parametrize("filter_cus", [1, 40, 96, 5000])
def test_masks_of_a_device_that_is_no_multiple_of_eight(prog, filter_cus):
    (f, o, w), = masks(prog, (100, filter_cus))
    assert w == 4
    assert f | o == bits(0, 100) and f & o == 0
    assert o & bits(96, 100) == bits(96, 100)
    gf = max(1, min(11, (filter_cus + 4) // 8))  # 12 groups
    assert bin(f).count("1") == 8 * gf and f & bits(96, 100) == 0


def test_no_masks(prog):
    assert masks(prog, (8, 4), (15, 4), (15, 1000), (256, 0), (256, -3), (0, 8)) == [(0, 0, 0)] * 6


@pytest.mark.parametrize("ncu", [256, 304])
def test_masks_partition_the_device(prog, ncu):
    F = range(1, 261)
    for filter_cus, (f, o, w) in zip(F, masks(prog, *[(ncu, x) for x in F])):
        gf = max(1, min(ncu // 8 - 1, (filter_cus + 4) // 8))
        assert w == (ncu + 31) // 32
        assert f & o == 0 and f | o == bits(0, ncu), filter_cus
        assert f != 0 and o != 0, filter_cus
        assert bin(f).count("1") == 8 * gf, filter_cus


# ---- the replay's chunk: min(64, 256 MiB / bytes per sweep), at least 1, at most the sweeps there are; the larger buffers of an
# earlier call win (device route: the slot buffers; host route: the smaller of slot and staging buffers). Bytes per sweep: the filter's
# output (4 per slot, 12 per CA-CFAR point) on the device route, the larger of that and the input images on the host route.
def chunk(prog, on_device, cfar, sweep_bytes, slots, n_sweeps, have=0, have_polar=0):
    (l,) = run(prog, ("chunk", int(on_device), int(cfar), sweep_bytes, slots, n_sweeps, have, have_polar))
    return int(l[1])


ROUTES = [  # (on_device, cfar, sweep_bytes, slots) of `per_sweep` bytes per sweep, on every route
    lambda per: (False, False, per, 16),           # host route: the images dominate
    lambda per: (False, False, 64, per // 4),      # host route: the slots dominate
    lambda per: (True, False, 1 << 40, per // 4),  # device route: the images do not count
    lambda per: (True, True, 1 << 40, per // 12),  # device route, CA-CFAR: 12 bytes per point
    lambda per: (False, True, 64, per // 12),
]


@pytest.mark.parametrize("route", range(len(ROUTES)))
@pytest.mark.parametrize("per_sweep,n_sweeps,expected", [(4 * MiB, 1000, 64), (8 * MiB, 1000, 32), (300 * MiB, 1000, 1), (4 * MiB, 5, 5),
                                                          (3 * MiB, 1000, 64), (12 * MiB, 1000, 21)])
def test_chunk(prog, route, per_sweep, n_sweeps, expected):
    # (a CA-CFAR route holds whole points, up to 8 bytes less per sweep: 256 MiB / (4 MiB - 4) is still 64, / (8 MiB - 8) still 32)
    assert chunk(prog, *ROUTES[route](per_sweep), n_sweeps) == expected


def test_chunk_keeps_the_larger_buffers_of_an_earlier_call(prog):
    assert chunk(prog, True, False, 1 << 40, 2 * MiB, 100) == 32                      # 8 MiB of slots per sweep
    assert chunk(prog, True, False, 1 << 40, 2 * MiB, 100, have=48, have_polar=0) == 48  # device route: the slot buffers alone
    assert chunk(prog, False, False, 8 * MiB, 16, 100, have=48, have_polar=16) == 32     # host route: the staging holds 16 only
    assert chunk(prog, False, False, 8 * MiB, 16, 100, have=48, have_polar=40) == 40
    assert chunk(prog, True, False, 1 << 40, 2 * MiB, 40, have=48) == 40               # ... never more than the sweeps there are
    assert chunk(prog, True, False, 1 << 40, 2 * MiB, 100, have=16) == 32


# ---- capacities: cap_points = A * k (CA-CFAR: cfar_max_points, 32768 when 0); cap_cells = min(MAX_CELLS, cap_points) when tuned, else
# cap_points up to submap 7 and min(cap_points, 4096) above; pair_cap = max(submap, 4) * cap_cells, at least 8192 under a tie rule
CAPS = [  # (cfar, A, k, cfar_max_points, submap, MAX_CELLS, tie rule) -> (cap_points, cap_cells, pair_cap)
    ((0, 400, 12, 0, 4, 0, 0), (4800, 4800, 19200)),
    ((0, 400, 12, 0, 3, 0, 0), (4800, 4800, 19200)),     # pair_cap counts at least four keyframes
    ((0, 400, 12, 0, 7, 0, 0), (4800, 4800, 33600)),     # the last submap with every point a cell
    ((0, 400, 12, 0, 8, 0, 0), (4800, 4096, 32768)),     # the 4096 default
    ((0, 400, 40, 0, 50, 0, 0), (16000, 4096, 204800)),
    ((0, 100, 12, 0, 8, 0, 0), (1200, 1200, 9600)),      # ... which never exceeds the points
    ((0, 400, 12, 0, 4, 1500, 0), (4800, 1500, 6000)),
    ((0, 400, 12, 0, 8, 6000, 0), (4800, 4800, 38400)),  # MAX_CELLS above cap_points: clamped (and no 4096 default)
    ((0, 48, 12, 0, 4, 0, 1), (576, 576, 8192)),         # a tie rule: the 8192 floor (4 * 576 = 2304)
    ((0, 48, 12, 0, 4, 0, 2), (576, 576, 8192)),
    ((0, 48, 12, 0, 4, 0, 0), (576, 576, 2304)),
    ((0, 400, 12, 0, 4, 0, 2), (4800, 4800, 19200)),     # ... which a larger pair_cap is above
    ((1, 400, 12, 0, 4, 0, 0), (32768, 32768, 131072)),  # CA-CFAR: the 32768 default
    ((1, 400, 12, 9000, 4, 0, 0), (9000, 9000, 36000)),
    ((1, 400, 12, 9000, 10, 0, 0), (9000, 4096, 40960)),
]


def test_capacities(prog):
    got = run(prog, *[("caps",) + c for c, _ in CAPS])
    assert [tuple(int(x) for x in l[1:]) for l in got] == [e for _, e in CAPS]


# ---- overlap: 0 .. 8, at most B, 0 with CA-CFAR
def test_overlap_clamp(prog):
    cases = [((9, 20, 0), 8), ((5, 3, 0), 3), ((2, 3, 0), 2), ((0, 3, 0), 0), ((-1, 3, 0), 0), ((8, 8, 0), 8), ((1, 3, 1), 0), ((8, 20, 1), 0), ((5, 3, 1), 0)]
    got = run(prog, *[("overlap",) + c for c, _ in cases])
    assert [int(l[1]) for l in got] == [e for _, e in cases]
