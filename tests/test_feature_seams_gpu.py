"""The feature build at the exact limits of its compact path (features_compact_dev.h, features_dev.h, features_dispatch in
odometry_step_dev.h), device vs the oracle: every cloud of feature_inputs.py - the value at a limit and the value one past it, by the
numpy twin of the build's bookkeeping (test_feature_inputs_cpu.py holds the clouds to that) - through the per-call entry
(cfear_scan_create) and through the batched cloud entry (cfear_odometry_step_cloud_device: features_cloud_step_body), next to two plain
clouds whose cells must not notice their neighbour; and polar sweeps whose filter keeps a stated number of slots through the slot route
(cfear_odometry_step_host: features_step_body, points in registers from ballots, bounds precomputed), sweep by sweep against the oracle's
fuser. Same cells in the same order, fields at rtol = atol = 1e-9 (the bar of
test_feature_fuzz_gpu.py), nsamples exactly, the 1-NN grid the same answers on 200 queries per radius. Every test prints the branch the
twin predicts ("[regime] ...", pytest -rA)."""
import numpy as np
import pytest

import feature_inputs as fi
from cfear_radarodometry_code_public_amd import capi
from sweep_compare import assert_sweep_is_the_fusers

pytestmark = pytest.mark.gpu
NAMES = list(fi.CASES)
FIELDS = ("mean", "cov", "normal", "lambda_min", "lambda_max", "scale", "sum_intensity", "avg_intensity")
LOG_FIELDS = ("mean", "normal", "cov", "scale")  # what the keyframe log keeps of a cell (+ nsamples)
R_BINS = 64  # the range axis of the contexts: no test here reads a polar sweep


def _regime(entry, c, P):
    print("[regime] %s %s: n %d against %d, grid %d x %d = %d (%s), nv %d -> %d counter set(s), vst[nv] in the %s half, window rows %s, chunks of %d: "
          "NC %d + NA %d %s, %d cells (%s LDS means), twin says the %s path"
          % (entry, c.name, P.n, min(fi.CPT_CAP, c.ccap if entry == "per-call" else c.n), P.div0, P.div1, P.G, "extra bitmap word" if P.extra_word else "no extra word",
             P.nv, P.sets, "high" if P.odd_nv else "low", sorted(set(P.rows.tolist())), P.C, P.NC, P.NA, "listed" if P.listed else "not listed", c.cells,
             "within the" if c.cells <= fi.LM_CAP else "beyond the", P.path))


def _same_cells(tag, got, exp, fields):
    assert len(got) == len(exp), (tag, len(got), len(exp))
    if len(exp):
        for f in fields:
            assert np.allclose(got[f], exp[f], rtol=1e-9, atol=1e-9), (tag, f, float(np.max(np.abs(got[f] - exp[f]))))
        assert np.array_equal(got["nsamples"], exp["nsamples"]), tag


@pytest.mark.parametrize("name", NAMES)
def test_per_call_build_at_the_seam(oracle, name):
    """cfear_scan_create; the context is created for A * k = the case's ccap points, so that the scratch the chunk list is measured against is the
    case's (4864, or the cloud's own size)"""
    c = fi.case(name)
    _regime("per-call", c, c.plan())
    ctx = capi.Context(fi.params(capi, c.res, c.df), c.ccap, R_BINS)
    so = fi.oracle_scan(c.xyi, c.res, c.df)
    sg = ctx.scan_create(ctx.cloud_upload(c.xyi))
    co, cg = so.cells(), sg.cells()
    assert len(co) == c.cells
    _same_cells(name, cg, co, FIELDS)
    q = fi.queries(co)
    assert len(q) == 200
    for d in (2.0, 4.0):
        exp = np.array([so.closest(x, y, d) for x, y in q])
        assert np.array_equal(sg.closest(q, d), exp), (name, d)
        assert (exp >= 0).sum() >= 30, (name, d)  # (queries that find a cell)
    ctx.close()


def _step_clouds(ctx, clouds, cap):
    """one sweep of a fresh batched object from clouds on the device -> (keyframe 0's cells per sequence, cell counts of the current scans)"""
    import torch
    B = len(clouds)
    odo = ctx.odometry(B)
    odo.record_keyframes(capi.KF_NODES | capi.KF_CELLS, 2, cap)
    h = np.zeros((B, cap, 3), dtype=np.float32)
    for q, x in enumerate(clouds):
        h[q, :len(x)] = x
    d_xyi = torch.from_numpy(h).cuda()
    d_n = torch.tensor([len(x) for x in clouds], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    odo.step_cloud_device(d_xyi.data_ptr(), cap, d_n.data_ptr())
    counts = [odo.summary(q)[1] for q in range(B)]
    assert not odo.status(per_sequence=True).any()
    rec, dropped = odo.keyframe_counts()
    assert list(rec) == [1] * B and not dropped.any()  # the first sweep is a keyframe (compensated with zero motion)
    cells = [odo.keyframe_cells(q, 0) for q in range(B)]
    odo.release()
    return cells, counts


@pytest.mark.parametrize("name", NAMES)
def test_batched_cloud_entry_at_the_seam(oracle, name):
    """cfear_odometry_step_cloud_device, B = 3: the case in sequence 1 between two plain clouds, on an object created for exactly n points per scan
    (its scratch, the chunk list's capacity included, is min(4864, n)). The log's cells of the first keyframe against the oracle; the neighbours'
    cells bit for bit those of a run in which sequence 1 holds a plain cloud too"""
    c = fi.case(name)
    n = c.n
    _regime("batched", c, c.plan(n))
    ctx = capi.Context(fi.params(capi, c.res, c.df), n, R_BINS)
    plain = [fi.plain_cloud(n, s) for s in range(3)]
    cells, counts = _step_clouds(ctx, [plain[0], c.xyi, plain[2]], n)
    co = fi.oracle_scan(c.xyi, c.res, c.df).cells()
    assert counts[1] == len(co) == c.cells
    _same_cells(name, cells[1], co, LOG_FIELDS)
    for q in (0, 2):
        _same_cells((name, q), cells[q], fi.oracle_scan(plain[q], c.res, c.df).cells(), LOG_FIELDS)
    alone, _ = _step_clouds(ctx, plain, n)
    for q in (0, 2):
        assert len(cells[q]) > 0
        assert cells[q].tobytes() == alone[q].tobytes(), (name, q)  # a neighbour's seam leaks into nobody
    ctx.close()


@pytest.mark.parametrize("name", list(fi.SLOT_CASES))
def test_slot_route_at_the_seam(oracle, name):
    """The cases of h and those of a and c that a polar image can produce (feature_inputs.SLOT_CASES says which of a - c it cannot, and why).
    cfear_odometry_step_host over four sweeps of a moving world, B = 2: the case's sweeps and the same sweeps with the bearings reversed
    ("holes": the same sweeps under a z_min of its own, above the filter's). Every sweep against the oracle's fuser at the bars of
    test_odometry_fuzz_gpu.py; the first keyframe's cells in the log against the fuser's first scan"""
    case = fi.SLOT_CASES[name]
    A, k, full = case.A, case.k, case.full
    imgs = fi.slot_sweeps(name)
    zs = (60.0, 60.0) if full else fi.HOLES_Z
    streams = [imgs, imgs[:, ::-1].copy() if full else imgs]
    n0 = [len(fi.slot_cloud(streams[q][0], k, zs[q])) for q in range(2)]
    P = fi.plan(fi.slot_cloud(imgs[0], k, zs[0]), 3.0, 1.0, A * k)
    print("[regime] slots %s: %d bearings (%s the table of %d) x k %d = %d slots (%s the registers' %d), first sweep keeps %s points in %d voxels -> %d counter set(s), twin says the %s path"
          % (name, A, "within" if A <= fi.BEARINGS else "beyond", fi.BEARINGS, k, A * k, "within" if A * k <= fi.REG_POINTS else "beyond", fi.REG_POINTS, n0, P.nv, P.sets, P.path))
    ctx = capi.Context(fi.slot_params(capi, k, min(zs)), A, fi.SLOT_R)
    odo = ctx.odometry(2)
    if not full:
        odo.set_sequence_params([fi.slot_params(capi, k, z) for z in zs])
    odo.record_keyframes(capi.KF_NODES | capi.KF_CELLS, fi.SLOT_T, fi.SLOT_T * A * k)
    fus = [oracle.Fuser(fi.slot_params(oracle, k, z)) for z in zs]
    first = [None, None]
    for t in range(fi.SLOT_T):
        odo.step_host(np.stack([s[t] for s in streams]))
        got = odo.poses()
        for q in range(2):
            exp = fus[q].process_polar(streams[q][t])
            assert_sweep_is_the_fusers(odo, q, t, got[q], fus[q], exp)
            if t == 0:
                first[q] = fus[q].last_cells()
    assert np.hypot(*got[0][:2]) > 2.0  # the world moved: the later sweeps were compensated with a motion
    assert not odo.status(per_sequence=True).any()
    for q in range(2):
        assert len(first[q]) >= 30
        _same_cells((name, q), odo.keyframe_cells(q, 0), first[q], LOG_FIELDS)
    odo.release(); ctx.close()
