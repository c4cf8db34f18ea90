"""CA-CFAR detector grids (cfear_filter_cfar_grid_device / cfear_odometry_set_sequence_detectors), the host-only part: replay.cfar_grid's
loop order, the cfear_seq_detector layout and the three exports, and the grouping of csrc/cfar_grid.h - which (source, detector) pairs a
launch decides and which cloud is emitted from which - through host/cfar_grid_check."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

from cfear_radarodometry_code_public_amd import capi, replay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cfear_radarodometry_code_public_amd", "host")
# the values of the detector loops of the reference's params/kstrong_vs_cfar/oxford-cfear-3-ca-cfar
OXFORD = json.load(open(os.path.join(ROOT, "tests", "golden", "cfar_grid_oxford.json")))


def cfar_base(**kw):
    return capi.default_params(filter_type=capi.FILTER_CACFAR, z_min=20.0, res=3.0, **kw)


def test_cfar_grid_of_the_reference_file_is_49_rows_rate_innermost(hip_lib):
    rows = replay.cfar_grid(cfar_base(), cfar_false_alarm_rate=OXFORD["cfar_false_alarm_rate"], cfar_window_size=OXFORD["cfar_window_size"])
    assert len(rows) == 49
    key = [(r.cfar_window_size, r.cfar_false_alarm_rate) for r in rows]
    f32 = lambda v: C.c_float(v).value
    assert key[0] == (40, f32(0.1)) and key[1] == (40, f32(0.05)) and key[7] == (70, f32(0.1)) and key[48] == (500, f32(0.0001))
    assert key == [(w, f32(p)) for w in OXFORD["cfar_window_size"] for p in OXFORD["cfar_false_alarm_rate"]]
    assert all(r.filter_type == capi.FILTER_CACFAR and r.cfar_nb_guard_cells == rows[0].cfar_nb_guard_cells and r.z_min == 20.0 for r in rows)
    dets = replay.grid_detectors(rows)
    assert all(isinstance(d, capi.SeqDetector) for d in dets)
    assert [(d.window_size, d.nb_guard_cells, d.false_alarm_rate, d.z_min) for d in dets] == [(w, rows[0].cfar_nb_guard_cells, p, 20.0) for w, p in key]


def test_guard_cells_and_z_min_nest_outside_window_and_rate(hip_lib):
    rows = replay.cfar_grid(cfar_base(), cfar_window_size=[40, 70], z_min=[10.0, 20.0], cfar_false_alarm_rate=[0.1, 0.01], cfar_nb_guard_cells=[5, 10],
                            res=[2.5, 3.5], weight_opt=[0, 1])
    got = [(r.res, r.cfar_nb_guard_cells, r.z_min, r.cfar_window_size, round(r.cfar_false_alarm_rate, 6), r.weight_opt) for r in rows]
    exp = [(res, g, z, w, p, wo) for res in (2.5, 3.5) for g in (5, 10) for z in (10.0, 20.0) for w in (40, 70) for p in (0.1, 0.01) for wo in (0, 1)]
    assert got == exp  # the worker's order: res, kstrong (guard cells), zmin, ..., covar_scale (window), regularization (rate), ..., weight_opt
    # the loops that carry the detector's values are no axes of their own; a k-strongest base is param_grid's
    for k in ("k_strongest", "covar_scale", "regularization"):
        with pytest.raises(ValueError):
            replay.cfar_grid(cfar_base(), **{k: [1, 2]})
    with pytest.raises(ValueError):
        replay.cfar_grid(capi.default_params(), cfar_window_size=[40])
    with pytest.raises(AttributeError):
        replay.cfar_grid(cfar_base(), no_such_field=[1])


def test_seq_detector_layout_and_exports(hip_lib):
    assert C.sizeof(capi.SeqDetector) == 16
    assert [getattr(capi.SeqDetector, f).offset for f in ("window_size", "nb_guard_cells", "false_alarm_rate", "z_min")] == [0, 4, 8, 12]
    assert [t for _, t in capi.SeqDetector._fields_] == [C.c_int32, C.c_int32, C.c_float, C.c_float]
    txt = open(os.path.join(ROOT, "include", "cfear_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"typedef\s+struct\s+cfear_seq_detector\s*\{\s*int32_t\s+window_size\s*,\s*nb_guard_cells;\s*float\s+false_alarm_rate;\s*float\s+z_min;\s*\}\s*cfear_seq_detector;", code)
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path()]).decode()
    exported = [l.split()[-1] for l in out.splitlines() if " T " in l]
    for name in ("cfear_filter_cfar_grid_device", "cfear_odometry_set_sequence_detectors", "cfear_odometry_sequence_detector"):
        assert name in exported and name in capi.EXPORTS and hasattr(hip_lib, name) and re.search(r"int\s+%s\s*\(" % name, code)


def plan(n_sources, clouds):
    """clouds: [(source, window, guard, rate, z_min)] -> dict(sets, pairs, max_reach, pair_begin, clouds) or None (refused)"""
    subprocess.check_call(["make", "-C", HOST, "cfar_grid_check"], stdout=subprocess.DEVNULL)
    args = [str(n_sources)] + [repr(v) for c in clouds for v in c]
    out = subprocess.run([os.path.join(HOST, "cfar_grid_check")] + args, capture_output=True, text=True)
    if out.returncode == 1 and out.stdout.strip() == "invalid":
        return None
    assert out.returncode == 0, out.stderr
    res = {"sets": [], "pairs": [], "clouds": []}
    for line in out.stdout.splitlines():
        w = line.split()
        if w[0] == "sets":
            res["n_sets"], res["n_pairs"], res["max_reach"] = int(w[1]), int(w[3]), int(w[5])
        elif w[0] == "set":
            res["sets"].append((int(w[2]), int(w[3]), float(w[4]), float(w[5])))
        elif w[0] == "pair":
            res["pairs"].append((int(w[3]), int(w[5])))
        elif w[0] == "pair_begin":
            res["pair_begin"] = [int(v) for v in w[1:]]
        elif w[0] == "cloud":
            res["clouds"].append((int(w[3]), int(w[5]), int(w[7])))
    return res


def test_equal_source_and_detector_is_decided_once():
    a, b, c = (40, 10, 0.01, 20.0), (70, 10, 0.01, 20.0), (40, 10, 0.01, 10.0)
    clouds = [(1,) + a, (0,) + a, (1,) + a, (1,) + b, (0,) + c, (2,) + b, (0,) + a]
    G = plan(4, clouds)
    assert G["n_sets"] == 3 and G["sets"] == [a, b, c] and G["max_reach"] == 80
    assert G["pairs"] == [(0, 0), (0, 2), (1, 0), (1, 1), (2, 1)] and G["n_pairs"] == 5  # sorted by (source, set); source 3 has none
    assert G["pair_begin"] == [0, 2, 4, 5, 5]
    for (src, k, p), cl in zip(G["clouds"], clouds):
        assert src == cl[0] and G["sets"][k] == cl[1:] and G["pairs"][p] == (src, k)
        assert G["pair_begin"][src] <= p < G["pair_begin"][src + 1]
    assert G["clouds"][0] == G["clouds"][2] and G["clouds"][1] == G["clouds"][6]  # exact duplicates share a pair
    # the reference's grid over one source: 49 sets, 49 pairs, the far corner's reach
    grid = [(0, w, 10, p, 20.0) for w in OXFORD["cfar_window_size"] for p in OXFORD["cfar_false_alarm_rate"]]
    G = plan(1, grid)
    assert G["n_sets"] == 49 and G["n_pairs"] == 49 and G["max_reach"] == 510 and G["pair_begin"] == [0, 49]
    assert [c[2] for c in G["clouds"]] == list(range(49))
    # a source outside [0, n_sources) is refused, never grouped
    assert plan(2, [(2,) + a]) is None and plan(2, [(-1,) + a]) is None
