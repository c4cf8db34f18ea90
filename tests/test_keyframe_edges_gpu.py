"""Constraints between any keyframes of a log, registered in one batch (cfear_odometry_keyframe_edges, keyframes.hip): against the per-call
route over the same log (cfear_odometry_keyframe_scans + cfear_register: byte for byte), against numpy / the host rule for the constraint,
and against the CPU oracle for the loop closures of the drive.

The drive is test_keyframes_gpu's: 35 sweeps played forwards, then backwards (T = 70, ~35 keyframes), so the way back revisits the way out:
43 pairs of keyframes at least 6 nodes apart lie within 3 m of each other. It is replayed once per module (two rolled copies, P2L).

Worst figures of a run on one MI355X: profiles/keyframe_edges_gpu_tests.txt."""
import numpy as np
import pytest

from cfear_radarodometry_code_public_amd import capi, replay
import test_keyframes_gpu as kg
from test_keyframes_gpu import A, R, T, KW, RR, P2L, P2D, MAX_CELLS, WHAT, images, frames, mat, xyt

pytestmark = pytest.mark.gpu
_C = {}


@pytest.fixture(scope="module")
def run():
    """two rolled copies of the drive through one object with the cells recorded: (ctx, odo, records, nodes per sequence)"""
    ctx = capi.Context(capi.default_params(**KW), A, R)
    odo = ctx.odometry(2)
    odo.record_keyframes(WHAT, T, MAX_CELLS)
    rec = odo.replay_host(frames(2))
    nodes = [odo.keyframes(q) for q in range(2)]
    yield ctx, odo, rec, nodes
    odo.release()
    ctx.close()


def per_call(ctx, odo, nodes, job):
    """the route of the parent commit for one job (a dict of capi.keyframe_edge_jobs): scans from the log, cfear_register, release
    -> (pose of `to`, cov [6, 6], RegSummary)"""
    q, to, frm = int(job["sequence"]), int(job["to"]), [int(v) for v in np.atleast_1d(job["from"])]
    guess = job.get("guess")
    scans = odo.keyframe_scans(q, frm + [to])
    poses = np.vstack([nodes[q]["pose"][frm], nodes[q]["pose"][to] if guess is None else np.asarray(guess, dtype=np.float64)])
    _, P, cov, S = ctx.register(scans, poses)
    for s in scans:
        s.release()
    return P[-1], cov, S


def same_as_per_call(tag, ctx, odo, nodes, jobs, edges, cov, sums):
    """every job's edge, covariance and summary against the per-call route: the same bytes"""
    paths, blocks = set(), []
    for k, job in enumerate(jobs):
        P, c, S = per_call(ctx, odo, nodes, job)
        e = edges[k]
        assert bytes(sums[k]) == bytes(S), (tag, k, "summary")  # assoc_path and the per-outer iteration counts included
        assert cov[k].tobytes() == c.tobytes(), (tag, k, "covariance")
        assert e["pose"].tobytes() == P.tobytes(), (tag, k, "pose")
        assert np.float64(e["final_cost"]).tobytes() == np.float64(S.final_cost).tobytes() and np.float64(e["score"]).tobytes() == np.float64(S.score).tobytes(), (tag, k)
        got = tuple(int(e[f]) for f in ("success", "usable", "outer_iterations", "num_residuals", "num_residual_blocks", "assoc_path"))
        assert got == (S.success, S.usable, S.outer_iterations, S.num_residuals, S.num_residual_blocks, S.assoc_path), (tag, k, got)
        frm = [int(v) for v in np.atleast_1d(job["from"])]
        assert (int(e["sequence"]), int(e["to"]), int(e["from"]), int(e["n_from"]), int(e["status"])) == \
            (int(job["sequence"]), int(job["to"]), frm[int(job.get("ref", 0))], len(frm), 0), (tag, k)
        paths.add(S.assoc_path)
        blocks.append((len(frm), S.num_residual_blocks))
    print(tag, "jobs", len(jobs), "assoc paths", sorted(paths), "(n_from, residual blocks)", sorted(set(blocks)))
    return blocks


def constraint_check(tag, nodes, jobs, edges, cov):
    """t_be / information of the edges with `success` against the host rule on (edge pose, node pose of from[ref], covariance)"""
    worst, n = [0.0, 0.0], 0
    for k, job in enumerate(jobs):
        e = edges[k]
        if not int(e["success"]):
            continue
        ref = nodes[int(job["sequence"])][int(e["from"])]
        t_be, info = capi.keyframe_constraint(e["pose"], ref["pose"], cov[k])
        worst[0] = max(worst[0], float(np.max(np.abs(e["t_be"] - t_be))))
        worst[1] = max(worst[1], float(np.max(np.abs(e["information"] - info)) / np.max(np.abs(info))))
        n += 1
    print(tag, "constraints", n, "t_be err", worst[0], "information rel err", worst[1])
    assert n > 0 and worst[0] <= 1e-12 and worst[1] <= 1e-6, (tag, worst)


def batch_jobs(nodes):
    """about 40 jobs over both sequences: n_from 1, 3, 4, 5, 8, 9 and 16 (neighbours in front of `to`; 16 also as four keyframes repeated),
    loop closures alone and with their neighbours, `to` among its own `from`, ref at 0 and in the middle, guesses given and defaulted,
    keyframes shared between jobs, and two jobs twice"""
    jobs = []
    for q in range(2):
        n = len(nodes[q])
        to = n - 3
        for nf in (1, 3, 4, 5, 8, 9, 16):
            job = dict(sequence=q, to=to, ref=(nf // 2 if q else 0))
            job["from"] = list(range(to - nf, to))
            if nf % 2 == 0:
                job["guess"] = nodes[q]["pose"][to] + np.array([0.3, -0.2, 0.01])
            jobs.append(job)
        cands = replay.loop_candidates(nodes[q], 6, 3.0)
        assert len(cands) >= 8, len(cands)
        for f, t in cands[:: max(1, len(cands) // 4)][:4]:
            f, t = int(f), int(t)
            jobs.append(dict(sequence=q, to=t, **{"from": [f]}))
            side = [i for i in (f - 2, f - 1, f + 1, f + 2) if 0 <= i < n and i != t]
            jobs.append(dict(sequence=q, to=t, ref=2, guess=nodes[q]["pose"][t] + np.array([-0.2, 0.25, -0.02]), **{"from": side[:2] + [f] + side[2:]}))
        f, t = next((int(f), int(t)) for f, t in cands if f >= 1 and f + 3 < t)
        jobs.append(dict(sequence=q, to=t, ref=1, **{"from": [f - 1, f, f + 1, f + 2]}))
        jobs.append(dict(sequence=q, to=t, ref=5, **{"from": [f, f + 1, f + 2, f + 3] * 4}))
        jobs.append(dict(sequence=q, to=t, ref=1, **{"from": [t, f]}))
    jobs.append(dict(jobs[3]))
    jobs.append(dict(jobs[-5]))
    return jobs


def test_one_batch_is_the_per_call_route_byte_for_byte(run):
    ctx, odo, rec, nodes = run
    jobs = batch_jobs(nodes)
    assert 36 <= len(jobs) <= 44 and {len(j["from"]) for j in jobs} >= {1, 3, 4, 5, 8, 9, 16}
    edges, cov, sums = odo.keyframe_edges(jobs, details=True)
    blocks = same_as_per_call("batch", ctx, odo, nodes, jobs, edges, cov, sums)
    assert min(b for _, b in blocks) < 512 < max(b for _, b in blocks), blocks  # both sides of the 512-block edge of the LDS match array
    assert edges["success"].all()
    # the two copies
    for a, b in ((3, len(jobs) - 2), (len(jobs) - 6, len(jobs) - 1)):
        assert edges[a].tobytes() == edges[b].tobytes() and cov[a].tobytes() == cov[b].tobytes() and bytes(sums[a]) == bytes(sums[b]), (a, b)
    # alone (m = 1) and inside the batch
    for k in (0, 6, 9, len(jobs) // 2, len(jobs) - 3):
        e1, c1, s1 = odo.keyframe_edges([jobs[k]], details=True)
        assert e1[0].tobytes() == edges[k].tobytes() and c1[0].tobytes() == cov[k].tobytes() and bytes(s1[0]) == bytes(sums[k]), k
    # the structured array is the list
    again = odo.keyframe_edges(capi.keyframe_edge_jobs(jobs))
    assert again.tobytes() == edges.tobytes()
    constraint_check("batch", nodes, jobs, edges, cov)


def test_a_nodes_own_registration_again(run):
    """to = j against from = [j-4 .. j-1], ref = 3, from the guess the sweep started at: the sweep's pose (register_again's bars), and a
    constraint that agrees with node j's own within what those bars allow - t_be = R(-theta)(to - from) moves by the pose's 1e-4 m per
    axis (1.42e-4 in norm) plus 1e-5 rad times its own length"""
    ctx, odo, rec, nodes = run
    jobs, where = [], []
    for q in range(2):
        for j in range(4, len(nodes[q])):
            t = int(nodes[q][j]["sweep"])
            jobs.append(dict(sequence=q, to=j, ref=3, guess=xyt(mat(rec["pose"][t - 1, q]) @ mat(nodes[q][j]["motion"])), **{"from": list(range(j - 4, j))}))
            where.append((q, j, t))
    edges, cov, sums = odo.keyframe_edges(jobs, details=True)
    worst = [0.0, 0.0, 0.0, 0.0, 0.0]
    for e, S, (q, j, t) in zip(edges, sums, where):
        r, nd = rec[t, q], nodes[q][j]
        assert int(e["success"]) == 1 and (S.outer_iterations, S.num_residuals) == (int(r["outer_iterations"]), int(r["num_residuals"])), (q, j)
        worst[0] = max(worst[0], abs(e["final_cost"] - r["final_cost"]) / abs(r["final_cost"]))
        worst[1] = max(worst[1], float(np.max(np.abs(e["pose"][:2] - r["pose"][:2]))))
        worst[2] = max(worst[2], abs(e["pose"][2] - r["pose"][2]))
        worst[3] = max(worst[3], float(np.max(np.abs(e["t_be"][:2] - nd["t_be"][:2])) - 1e-5 * np.hypot(*nd["t_be"][:2])))
        worst[4] = max(worst[4], abs(e["t_be"][2] - nd["t_be"][2]))
        assert int(e["from"]) == j - 1 == int(nd["prev"])
    print("own registrations", len(jobs), "final_cost rel err", worst[0], "pose err", worst[1], worst[2], "t_be err beyond 1e-5 |t_be|", worst[3], "t_be angle err", worst[4])
    assert worst[0] <= 1e-9 and worst[1] <= 1e-4 and worst[2] <= 1e-5 and worst[3] <= 1.5e-4 and worst[4] <= 1e-5, worst
    constraint_check("own", nodes, jobs, edges, cov)


@pytest.mark.parametrize("n_side", [0, 2])
def test_loop_closures_against_the_oracle(run, oracle, n_side):
    """the 43 candidates of sequence 0, alone and with two neighbours on each side: every one against oracle.register on oracle scans of
    the same sweeps at the same poses, by the bars of test_register_fuzz_gpu.compare. None is left out, and all are usable."""
    ctx, odo, rec, nodes = run
    nd = nodes[0]
    pairs = replay.loop_candidates(nd, 6, 3.0)
    oposes, _, _ = kg.oracle_run(oracle, 0)
    sweeps = kg.rule_sweeps(oposes)
    assert list(nd["sweep"]) == sweeps
    opairs = replay.loop_candidates({"pose": oposes[sweeps]}, 6, 3.0)
    assert len(pairs) == len(opairs) == 43, (len(pairs), len(opairs))
    assert np.array_equal(pairs, opairs)
    jobs = replay.edge_jobs(0, pairs, n_side, len(nd))
    edges, cov, sums = odo.keyframe_edges(jobs, details=True)
    po = oracle.default_params(**KW)
    if "oscans" not in _C:
        _C["oscans"] = [oracle.Scan(oracle.compensate(oracle.cloud(oracle.filter_polar(images()[int(n["sweep"])], 60, 12), RR, po.min_distance), n["motion"],
                                                      po.radar_ccw), po) for n in nd]
    oscans = _C["oscans"]
    worst = [0.0, 0.0, 0.0, 0.0]
    moved = []
    for k, job in enumerate(jobs):
        frm, to = [int(v) for v in job["from"][:int(job["n_from"])]], int(job["to"])
        poses = np.vstack([nd["pose"][frm], nd["pose"][to]])
        reto, Po, covo, So = oracle.register([oscans[i] for i in frm] + [oscans[to]], poses, po)
        e, Sg = edges[k], sums[k]
        assert So.usable == 1 and reto, (k, "the oracle itself registers every candidate usably")
        assert bool(reto) == bool(e["success"]) and So.usable == Sg.usable == int(e["usable"]) and So.success == Sg.success, k
        assert So.outer_iterations == Sg.outer_iterations and list(So.inner_iterations[:8]) == list(Sg.inner_iterations[:8]), k
        assert list(So.termination[:8]) == list(Sg.termination[:8]), k
        assert So.num_residuals == Sg.num_residuals == int(e["num_residuals"]) and So.num_residual_blocks == Sg.num_residual_blocks, k
        worst[0] = max(worst[0], abs(Sg.final_cost - So.final_cost) / abs(So.final_cost))
        worst[1] = max(worst[1], float(np.max(np.abs(e["pose"][:2] - Po[-1, :2]))))
        worst[2] = max(worst[2], abs(e["pose"][2] - Po[-1, 2]))
        worst[3] = max(worst[3], float(np.max(np.abs(cov[k] - covo) / (1e-6 * np.abs(covo) + 1e-12))))
        moved.append(float(np.hypot(*(e["pose"][:2] - nd["pose"][to][:2]))))
    print("loop closures n_side", n_side, "jobs", len(jobs), "final_cost rel err", worst[0], "pose err", worst[1], worst[2], "cov err / (1e-6 |ref| + 1e-12)", worst[3],
          "outer", sorted(set(int(v) for v in edges["outer_iterations"])), "blocks %d..%d" % (edges["num_residual_blocks"].min(), edges["num_residual_blocks"].max()),
          "moved %.2f..%.2f m" % (min(moved), max(moved)))
    assert worst[0] <= 1e-9 and worst[1] <= 1e-4 and worst[2] <= 1e-5 and worst[3] <= 1.0, worst
    constraint_check("loop closures", nodes, [dict(sequence=0) for _ in jobs], edges, cov)


def test_rows_run_under_their_own_parameters():
    """two sequences over one source, a P2L and a P2D row: jobs of both in one call, each row's against a context of that row's parameters"""
    kw = dict(KW, regularization=0.1, covar_scale=1.0)
    rows = [dict(kw, cost=P2L), dict(kw, cost=P2D)]
    ctx = capi.Context(capi.default_params(**rows[0]), A, R)
    odo = ctx.odometry(2)
    odo.set_sequence_shapes([(P2L, 4), (P2D, 4)])
    odo.set_sequence_params([capi.default_params(**r) for r in rows])
    odo.set_sequence_sources(np.zeros(2, dtype=np.int32), 1)
    odo.record_keyframes(WHAT, T, MAX_CELLS)
    odo.replay_host(images()[:, None])
    nodes = [odo.keyframes(q) for q in range(2)]
    assert nodes[0]["pose"].tobytes() != nodes[1]["pose"].tobytes()
    jobs = []
    for q in range(2):
        pairs = replay.loop_candidates(nodes[q], 6, 3.0)[:5]
        assert len(pairs) == 5
        for k, (f, t) in enumerate(pairs):
            jobs.append(dict(sequence=q, to=int(t), **{"from": [int(f)] if k % 2 else [int(f), int(f) + 1, int(f) + 2]}))
    jobs = [jobs[i // 2 + (len(jobs) // 2) * (i % 2)] for i in range(len(jobs))]  # the rows' jobs interleaved
    edges, cov, sums = odo.keyframe_edges(jobs, details=True)
    for q in range(2):
        own = capi.Context(capi.default_params(**rows[q]), A, R)
        mine = [k for k, j in enumerate(jobs) if j["sequence"] == q]
        same_as_per_call("row %d" % q, own, odo, nodes, [jobs[k] for k in mine], edges[mine], cov[mine], [sums[k] for k in mine])
        own.close()
    # (the two costs count residuals differently: a P2D block has two)
    assert all(int(e["num_residuals"]) == (1 if j["sequence"] == 0 else 2) * int(e["num_residual_blocks"]) for e, j in zip(edges, jobs))
    odo.release(); ctx.close()


def raw_call(odo, J):
    """the C entry on a job array, the edges prefilled -> (rc, message, edge bytes)"""
    edges = np.full(len(J) * capi.KEYFRAME_EDGE_DTYPE.itemsize, 0xAB, dtype=np.uint8)
    c = odo._ctx
    rc = c._L.cfear_odometry_keyframe_edges(c._h, odo._h, J.ctypes.data, len(J), edges.ctypes.data, None, None)
    return rc, c._L.cfear_last_error(c._h).decode(), edges


def test_failures_and_refusals(run):
    ctx, odo, rec, nodes = run
    n = len(nodes[0])
    pairs = replay.loop_candidates(nodes[0], 6, 3.0)
    good = [dict(sequence=0, to=int(t), **{"from": [int(f)]}) for f, t in pairs[:3]]
    lost = dict(sequence=0, to=int(pairs[1][1]), guess=nodes[0]["pose"][int(pairs[1][1])] + np.array([500.0, 300.0, 0.0]), **{"from": [int(pairs[1][0]), int(pairs[1][0]) + 1]})
    alone = odo.keyframe_edges(good)
    mixed, cov, sums = odo.keyframe_edges([good[0], lost, good[1], good[2]], details=True)
    e = mixed[1]
    assert int(e["success"]) == 0 and int(e["usable"]) == 0 and int(e["num_residuals"]) <= 1 and int(e["status"]) == 0
    assert not e["t_be"].any() and not e["information"].any() and not cov[1].any()
    assert e["pose"].tobytes() == np.asarray(lost["guess"]).tobytes()
    assert mixed[[0, 2, 3]].tobytes() == alone.tobytes()  # its neighbours in the call are unaffected
    # refusals: the code, a message that names job and field, and no edge written
    J = capi.keyframe_edge_jobs(good)
    blank = np.full(len(J) * capi.KEYFRAME_EDGE_DTYPE.itemsize, 0xAB, dtype=np.uint8)

    def refused(field, value, code, word, job=1):
        bad = J.copy()
        if field == "from0":
            bad[job]["from"][0] = value
        else:
            bad[job][field] = value
        rc, msg, edges = raw_call(odo, bad)
        assert rc == code and "jobs[%d]" % job in msg and word in msg, (field, value, rc, msg)
        assert edges.tobytes() == blank.tobytes(), field
    refused("sequence", 2, -1, "sequence"); refused("sequence", -1, -1, "sequence")
    refused("to", n, -1, ".to"); refused("to", -1, -1, ".to", job=2)
    refused("from0", n, -1, "from[0]"); refused("from0", -3, -1, "from[0]", job=0)
    refused("n_from", 0, -1, "n_from"); refused("n_from", capi.KF_EDGE_MAX_FROM + 1, -1, "n_from")
    refused("ref", 1, -1, ".ref"); refused("ref", -1, -1, ".ref")
    bad = J.copy(); bad[2]["flags"] = 1; bad[2]["guess_xyt"] = [0.0, np.nan, 0.0]
    rc, msg, edges = raw_call(odo, bad)
    assert rc == -1 and "jobs[2].guess_xyt" in msg and edges.tobytes() == blank.tobytes(), (rc, msg)
    bad[2]["guess_xyt"] = [np.inf, 0.0, 0.0]
    assert raw_call(odo, bad)[0] == -1
    bad[2]["flags"] = 0  # a guess that is not given is not read
    assert raw_call(odo, bad)[0] == 0
    with pytest.raises(capi.CfearError, match="rc=-1"):
        odo.keyframe_edges([dict(sequence=0, to=n, **{"from": [0]})])
    # a log without cells; a keyframe without cells (a blank first sweep is the first keyframe)
    o2 = ctx.odometry(1)
    o2.record_keyframes(capi.KF_NODES, 16, 0)
    o2.replay_host(images()[:8, None])
    rc, msg, edges = raw_call(o2, capi.keyframe_edge_jobs([(0, 2, [0])]))
    assert rc == -1 and "CFEAR_KF_CELLS" in msg and edges.tobytes() == blank[:400].tobytes(), (rc, msg)
    o2.release()
    ctx3 = capi.Context(capi.default_params(**dict(KW, use_keyframe=0)), A, R)  # every sweep is a keyframe: a blank sweep is a keyframe without cells
    o3 = ctx3.odometry(1)
    o3.record_keyframes(WHAT, 16, 16 * 1024)
    fr = images()[:8, None].copy(); fr[3] = 0
    o3.replay_host(fr)
    nd = o3.keyframes(0)
    assert len(nd) == 8 and int(nd[3]["n_cells"]) == 0 and int(nd[1]["n_cells"]) > 0 and int(nd[2]["n_cells"]) > 0
    for job, word in (((0, 2, [1, 3]), "from[1]"), ((0, 3, [1]), ".to")):
        rc, msg, edges = raw_call(o3, capi.keyframe_edge_jobs([(0, 2, [1]), job]))
        assert rc == -4 and "jobs[1]" in msg and word in msg and edges.tobytes() == blank[:800].tobytes(), (rc, msg)
    assert int(o3.keyframe_edges([(0, 2, [1])])[0]["usable"]) == 1
    o3.release(); ctx3.close()
    # recording off
    o4 = ctx.odometry(1)
    rc, msg, _ = raw_call(o4, capi.keyframe_edge_jobs([(0, 1, [0])]))
    assert rc == -1 and "recording is off" in msg
    o4.release()


def test_kd_tree_parity_mode():
    """cfear_tune NN_TIE_RULE = 2, the object created after the tune call: three jobs against the per-call route in that mode"""
    ctx = capi.Context(capi.default_params(**KW), A, R)
    ctx.tune(capi.TUNE_NN_TIE_RULE, 2)
    odo = ctx.odometry(1)
    odo.record_keyframes(WHAT, 16, 16 * 1024)
    odo.replay_host(images()[:12, None])
    nodes = [odo.keyframes(0)]
    n = len(nodes[0])
    assert n >= 4
    jobs = [dict(sequence=0, to=n - 1, **{"from": [n - 2]}), dict(sequence=0, to=n - 1, ref=1, guess=nodes[0]["pose"][n - 1] + np.array([0.2, 0.1, 0.01]), **{"from": [n - 3, n - 2]}),
            dict(sequence=0, to=2, **{"from": list(range(n)) + [0]})]
    edges, cov, sums = odo.keyframe_edges(jobs, details=True)
    same_as_per_call("NN_TIE_RULE 2", ctx, odo, nodes, jobs, edges, cov, sums)
    assert edges["success"].all() and set(int(v) for v in edges["assoc_path"]) == {3}
    odo.release(); ctx.close()


def test_the_call_writes_nothing(run):
    """the log, and a replay continued afterwards, with and without a keyframe_edges call in between"""
    ctx = run[0]
    fr = np.ascontiguousarray(frames(2)[:, :1])
    out = []
    for call in (False, True):
        odo = ctx.odometry(1)
        odo.record_keyframes(WHAT, T, MAX_CELLS)
        first = odo.replay_host(fr[:48])
        before = kg.log_of(odo)
        if call:
            nd = odo.keyframes(0)
            pairs = replay.loop_candidates(nd, 6, 3.0)
            assert len(pairs) >= 3
            edges = odo.keyframe_edges(replay.edge_jobs(0, pairs, 1, len(nd)))
            assert edges["success"].all()
            kg.logs_equal(before, kg.log_of(odo))
        rest = odo.replay_host(fr[48:])
        out.append((first, rest, kg.log_of(odo), odo.poses(), odo.keyframe_counts()))
        odo.release()
    (f0, r0, l0, p0, c0), (f1, r1, l1, p1, c1) = out
    assert f0.tobytes() == f1.tobytes() and r0.tobytes() == r1.tobytes() and p0.tobytes() == p1.tobytes()
    kg.logs_equal(l0, l1)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(c0, c1))


def test_replay_grid_and_the_command_line_carry_the_edges(tmp_path):
    from cfear_radarodometry_code_public_amd import readers
    rows = [capi.default_params(**KW), capi.default_params(**dict(KW, min_keyframe_dist=3.0))]
    spec = dict(min_index_gap=4, max_dist=3.0, n_side=1)
    out = replay.replay_grid(images(), rows, keyframes="cells", edges=spec)
    assert len(out["keyframe_edges"]) == 2 and not out["keyframes_dropped"].any()
    for q in range(2):
        one = replay.replay_grid(images(), [rows[q]], keyframes="cells", edges=spec)
        assert one["keyframes"][0].tobytes() == out["keyframes"][q].tobytes(), q
        e = out["keyframe_edges"][q]
        pairs = replay.loop_candidates(out["keyframes"][q], 4, 3.0)
        assert len(e) == len(pairs) >= 5 and np.array_equal(e["to"], pairs[:, 1]) and np.array_equal(e["from"], pairs[:, 0]) and np.all(e["sequence"] == q)
        assert one["keyframe_edges"][0]["sequence"].tolist() == [0] * len(e)
        for f in capi.KEYFRAME_EDGE_DTYPE.names:
            if f != "sequence":
                assert one["keyframe_edges"][0][f].tobytes() == e[f].tobytes(), (q, f)
        assert e["success"].all()
    assert "keyframe_edges" not in replay.replay_grid(images()[:4], rows, keyframes="cells")
    with pytest.raises(ValueError):
        replay.replay_grid(images()[:4], rows, keyframes="nodes", edges=spec)
    # the command line over the same sweeps as an Oxford PNG directory: the file's loop edges are row 0's
    d = tmp_path / "radar"
    d.mkdir()
    for i in range(T):
        ts = 1547131046353776 + i * 250000
        readers.write_png_gray8(d / ("%d.png" % ts), readers.oxford_png_rows(images()[i], ts + np.arange(A) * 625), filter_type=2)
    g = tmp_path / "graph.g2o"
    res = replay.main(["--oxford_png_dir", str(d), "--est_directory", str(tmp_path / "est"), "--range-res", "0.0595238", "--z-min", "60", "--res", "3.0",
                       "--submap_scan_size", "4", "--weight_option", "4", "--store_graph", str(g), "--loop_edges", "4,3.0,1"])
    e = out["keyframe_edges"][0]
    assert res["keyframes"] == len(out["keyframes"][0]) and res["loop_candidates"] == len(e) and res["loop_edges"] == int(e["success"].sum())
    back = replay.read_g2o_edges(g)
    blk = np.ix_(replay.G2O_INFO, replay.G2O_INFO)
    assert back["to"].tobytes() == e["to"].tobytes() and back["from"].tobytes() == e["from"].tobytes() and back["t_be"].tobytes() == e["t_be"].tobytes()
    assert all(np.triu(b["information"][blk]).tobytes() == np.triu(a["information"][blk]).tobytes() for a, b in zip(e, back))  # (the text carries the upper triangle)
    nodes_back = replay.read_g2o(g)
    for f in ("index", "prev", "pose", "t_be"):
        assert nodes_back[f].tobytes() == out["keyframes"][0][f].tobytes(), f
