"""ROS-free replay of a recorded sequence through the device odometry (the reference's offline_odometry.cpp:60-127 loop):

    python -m cfear_radarodometry_code_public_amd.replay --bag radar.bag --est_directory out [--gt_directory out]
    python -m cfear_radarodometry_code_public_amd.replay --oxford_png_dir <sequence>/radar --est_directory out

Reads /Navtech/Polar sweeps (and /gt odometry when present) from a rosbag v2.0 file, or the PNG sweeps of an Oxford Radar
RobotCar sequence in file-name (timestamp) order, hands them to cfear_odometry_replay_host in pieces (one sequence; no host
round trip per sweep) and writes the trajectory in the KITTI text format of EvalTrajectory::Write (est_00.txt, gt_00.txt).
Prints the replay rate (sweeps / second, what offline_odometry.cpp:125 prints) and, with ground truth, the KITTI drift.
Needs a GPU: there is no CPU path.
"""
import argparse
import glob
import json
import os

import numpy as np

from . import capi, kitti, readers


# the nesting of the reference's evaluation grids (utils/worker:42-87, outermost loop first) by the cfear_params field each loop sets
GRID_ORDER = ("radar_ccw", "compensate", "cost", "submap_scan_size", "min_keyframe_dist", "res", "k_strongest", "z_min", "loss", "loss_limit",
              "covar_scale", "regularization", "weight_intensity", "weight_opt")


def param_grid(base, **axes):
    """The parameter sets of a nested-loop evaluation grid in the reference's loop order (utils/worker:26-99: ... res, k_strongest, z_min,
    loss, loss_limit, covar_scale, regularization, weight_intensity, weight_opt innermost), whatever order the axes are given in; axes the
    reference's worker does not loop over (iteration limits, ...) nest inside those, in the order given. base: a capi.Params; each axis a
    list of values of that field. -> list of capi.Params, job 1 first. Pure Python (no device)."""
    import copy
    import itertools
    for k in axes:
        if not hasattr(base, k):
            raise AttributeError(k)
    names = [k for k in GRID_ORDER if k in axes] + [k for k in axes if k not in GRID_ORDER]
    rows = []
    for values in itertools.product(*[list(axes[k]) for k in names]):
        p = copy.copy(base) if not isinstance(base, capi.Params) else capi.Params.from_buffer_copy(base)
        for k, v in zip(names, values):
            setattr(p, k, v)
        rows.append(p)
    return rows


# ... of a CA-CFAR base: offline_odometry.cpp:260-265 hands the worker's kstrong loop to nb_guard_cells, its covar_scale loop to window_size
# and its regularization loop to false_alarm_rate (params/kstrong_vs_cfar/oxford-cfear-3-ca-cfar:28-30), so the detector axes sit in those
# loops' positions: guard cells, then z_min, then the window, the rate innermost of the three
CFAR_GRID_ORDER = tuple({"k_strongest": "cfar_nb_guard_cells", "covar_scale": "cfar_window_size", "regularization": "cfar_false_alarm_rate"}.get(k, k)
                        for k in GRID_ORDER)


def cfar_grid(base, **axes):
    """param_grid for a filter_type CA-CFAR base with the detector's cfar_nb_guard_cells, cfar_window_size and cfar_false_alarm_rate as
    axes, in the loop positions the reference's worker gives them (utils/worker:61-77 through offline_odometry.cpp:260-265): ...
    res, cfar_nb_guard_cells, z_min, loss, loss_limit, cfar_window_size, cfar_false_alarm_rate, weight_intensity, weight_opt
    innermost. k_strongest, covar_scale and regularization are no axes here (their loops carry the detector's values). -> list of
    capi.Params, job 1 first - what replay_grid runs as the sequences of one object. Pure Python (no device)."""
    import itertools
    if int(base.filter_type) != capi.FILTER_CACFAR:
        raise ValueError("cfar_grid: the base's filter_type is not CA-CFAR (param_grid builds k-strongest grids)")
    for k in axes:
        if not hasattr(base, k):
            raise AttributeError(k)
        if k in ("k_strongest", "covar_scale", "regularization"):
            raise ValueError("cfar_grid: %s is no axis of a CA-CFAR grid (the worker's loop of that name carries a detector value)" % k)
    names = [k for k in CFAR_GRID_ORDER if k in axes] + [k for k in axes if k not in CFAR_GRID_ORDER]
    rows = []
    for values in itertools.product(*[list(axes[k]) for k in names]):
        p = capi.Params.from_buffer_copy(base)
        for k, v in zip(names, values):
            setattr(p, k, v)
        rows.append(p)
    return rows


def grid_detectors(rows):
    """The capi.SeqDetector of every row of a CA-CFAR grid (its cfar_window_size, cfar_nb_guard_cells, cfar_false_alarm_rate and z_min):
    what Odometry.set_sequence_detectors takes before the table. Pure Python (no device)."""
    return [capi.SeqDetector(int(r.cfar_window_size), int(r.cfar_nb_guard_cells), float(r.cfar_false_alarm_rate), float(r.z_min)) for r in rows]


def grid_context_params(rows):
    """The parameters of the context a grid's rows run under: a copy of rows[0] with k_strongest the largest of the rows - the filter runs
    with it and the object is sized for it, every row takes its own k strongest out of those (cfear_odometry_set_sequence_params) - and
    submap_scan_size the largest of the rows: the object's scan slots and scratch are sized for it, every row keeps a ring of its own
    length (grid_shapes, cfear_odometry_set_sequence_shapes). The cost is rows[0]'s. Rows of equal k and submap size: rows[0]. Pure
    Python (no device); `rows` stays as it is."""
    rows = list(rows)
    p = capi.Params.from_buffer_copy(rows[0])
    p.k_strongest = max(int(r.k_strongest) for r in rows)
    p.submap_scan_size = max(int(r.submap_scan_size) for r in rows)
    return p


def grid_shapes(rows, context_params):
    """The capi.SeqShape of every row (its cost and submap_scan_size) - what Odometry.set_sequence_shapes takes before the table of a grid
    with cost or submap_scan_size among its axes (utils/worker:49-52) - or None when every row equals context_params in both fields (no
    shapes needed). Pure Python (no device)."""
    rows = list(rows)
    if all(int(r.cost) == int(context_params.cost) and int(r.submap_scan_size) == int(context_params.submap_scan_size) for r in rows):
        return None
    return [capi.SeqShape(int(r.cost), int(r.submap_scan_size)) for r in rows]


# ... with the fuser's own switches (capi.FuserOptions): soft_constraint is the worker's third loop (utils/worker:40-46: after radar_ccw,
# before disable_compensate); use_guess is not a loop of the worker and nests inside all of them
FUSER_GRID_ORDER = GRID_ORDER[:1] + ("soft_constraint",) + GRID_ORDER[1:] + ("use_guess",)
FUSER_AXES = ("soft_constraint", "use_guess")


def fuser_grid(base, base_options=None, **axes):
    """param_grid with the fuser's soft_constraint and use_guess allowed as axes, in the reference's loop order (soft_constraint between
    radar_ccw and compensate, use_guess innermost of the worker's axes; other axes inside those, in the order given). base: a
    capi.Params; base_options: the capi.FuserOptions the axes start from (None: the defaults 0, 1). -> (rows, options): a list of
    capi.Params and a list of capi.FuserOptions of the same length, job 1 first - what replay_grid(frames, rows, options=options)
    takes. Pure Python (no device)."""
    import itertools
    for k in axes:
        if k not in FUSER_AXES and not hasattr(base, k):
            raise AttributeError(k)
    b_soft, b_guess = (0, 1) if base_options is None else (int(base_options.soft_constraint), int(base_options.use_guess))
    names = [k for k in FUSER_GRID_ORDER if k in axes] + [k for k in axes if k not in FUSER_GRID_ORDER]
    rows, options = [], []
    for values in itertools.product(*[list(axes[k]) for k in names]):
        p = capi.Params.from_buffer_copy(base)
        o = capi.FuserOptions(b_soft, b_guess)
        for k, v in zip(names, values):
            setattr(o if k in FUSER_AXES else p, k, v)
        rows.append(p)
        options.append(o)
    return rows, options


def drift_dict(row):
    """one result of capi.DriftPlan.score -> the dict kitti.drift_by_length returns"""
    return {"translation_percent": float(row["translation_percent"]), "rotation_deg_per_100m": float(row["rotation_deg_per_100m"]),
            "segments": int(row["segments"]),
            "by_length": {"length_m": list(kitti.LENGTHS), "translation_percent": [float(v) for v in row["translation_percent_by_length"]],
                          "rotation_deg_per_100m": [float(v) for v in row["rotation_deg_per_100m_by_length"]],
                          "segments": [int(v) for v in row["segments_by_length"]]}}


G2O_INFO = (0, 1, 5)  # rows / columns of the 6x6 information (x, y, z, roll, pitch, yaw) a planar EDGE_SE2 carries: x, y, yaw


def loop_candidates(nodes, min_index_gap=6, max_dist=3.0, max_per_node=None):
    """Pairs of keyframes far apart in the log and close in space - where a back end looks for the constraints the odometry chain does not
    have: (from, to) with from < to, to - from >= min_index_gap and |pose_to - pose_from| <= max_dist (metres, x and y of the node
    poses), per `to` nearest first (ties: the smaller index) and cut at max_per_node, `to` ascending. nodes: KEYFRAME_NODE_DTYPE (or
    anything with a "pose" field) -> int32 [n, 2]. Pure numpy (no device)."""
    xy = np.asarray(nodes["pose"], dtype=np.float64).reshape(-1, 3)[:, :2]
    pairs = []
    for to in range(len(xy)):
        last = to - int(min_index_gap)
        if last < 0:
            continue
        d = np.hypot(xy[:last + 1, 0] - xy[to, 0], xy[:last + 1, 1] - xy[to, 1])
        near = np.flatnonzero(d <= max_dist)
        near = near[np.argsort(d[near], kind="stable")]
        if max_per_node is not None:
            near = near[:int(max_per_node)]
        pairs.extend((int(f), to) for f in near)
    return np.array(pairs, dtype=np.int32).reshape(-1, 2)


def edge_jobs(sequence, pairs, n_side=0, n_nodes=None):
    """The jobs of capi.Odometry.keyframe_edges for (from, to) pairs of one sequence (loop_candidates): `to` is registered against the
    candidate and up to n_side neighbours on each side of it - a small submap around the place revisited - clipped to the log (0 ..
    n_nodes - 1; n_nodes None: up to the candidate's own index + n_side) and never `to` itself. The candidate is from[0] and the keyframe the
    constraint is expressed to (ref = 0); the guess is `to`'s recorded pose. -> KEYFRAME_EDGE_JOB_DTYPE [len(pairs)]. Pure numpy."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    n_side = int(n_side)
    if not 0 <= 2 * n_side + 1 <= capi.KF_EDGE_MAX_FROM:
        raise ValueError("edge_jobs: n_side %d gives more than %d `from` keyframes" % (n_side, capi.KF_EDGE_MAX_FROM))
    out = np.zeros(len(pairs), dtype=capi.KEYFRAME_EDGE_JOB_DTYPE)
    for k, (f, to) in enumerate(pairs):
        f, to = int(f), int(to)
        side = [i for i in range(f - n_side, f + n_side + 1) if i != f and i != to and i >= 0 and (n_nodes is None or i < int(n_nodes))]
        frm = [f] + side
        out[k]["sequence"], out[k]["to"], out[k]["n_from"] = int(sequence), to, len(frm)
        out[k]["from"][:len(frm)] = frm
    return out


def appearance_jobs(sequence, candidates, nodes, n_side=0):
    """The jobs of capi.Odometry.keyframe_edges for the appearance candidates of one sequence (capi.Odometry.keyframe_candidates /
    scancontext.candidates: SC_CANDIDATE_DTYPE; records of other sequences are passed over): as edge_jobs - the candidate is from[0] and
    ref, up to n_side neighbours on each side join it - but with a guess (flag bit 0): `to` is placed ON the candidate, at the recorded
    pose of `from` with the match's yaw added to its angle. The odometry's own pose of `to` is the wrong start exactly when the loop is
    worth closing: it is off by the drift. nodes: the sequence's KEYFRAME_NODE_DTYPE. -> KEYFRAME_EDGE_JOB_DTYPE. Pure numpy."""
    cand = np.asarray(candidates, dtype=capi.SC_CANDIDATE_DTYPE).reshape(-1)
    cand = cand[cand["sequence"] == int(sequence)]
    out = edge_jobs(sequence, np.stack([cand["from"], cand["to"]], axis=1) if len(cand) else np.zeros((0, 2), dtype=np.int64), n_side, len(nodes))
    pose = np.asarray(nodes["pose"], dtype=np.float64).reshape(-1, 3)
    for k, c in enumerate(cand):
        g = pose[int(c["from"])].copy()
        g[2] += float(c["yaw"])
        out[k]["flags"], out[k]["guess_xyt"] = 1, g
    return out


def write_g2o(path, nodes, edges=None):
    """The keyframe graph of one sequence (capi.Odometry.keyframes: KEYFRAME_NODE_DTYPE) as g2o text: `VERTEX_SE2 index x y theta` per
    node and, for every node with a previous one, `EDGE_SE2 index prev dx dy dtheta i11 i12 i13 i22 i23 i33` - the constraint AddToGraph
    stores (odometrykeyframefuser.cpp:435-443: from the new keyframe to the previous one) with the upper triangle of the information's
    (x, y, yaw) block. edges: constraints between any keyframes (capi.Odometry.keyframe_edges: KEYFRAME_EDGE_DTYPE) - those with `success`
    follow as `EDGE_SE2 to from ...`, by the same rule; None: the text is the nodes' alone. Floats are written with repr: read_g2o /
    read_g2o_edges give back the same bits. Pure Python (no device)."""
    with open(path, "w") as f:
        f.write(g2o_text(nodes, edges))


def _g2o_edge(a, b, t_be, information):
    info = np.asarray(information).reshape(6, 6)
    tri = [info[G2O_INFO[i], G2O_INFO[j]] for i in range(3) for j in range(i, 3)]
    return "EDGE_SE2 %d %d %s" % (int(a), int(b), " ".join(repr(float(v)) for v in list(t_be) + tri))


def g2o_text(nodes, edges=None):
    lines = []
    for nd in nodes:
        lines.append("VERTEX_SE2 %d %s" % (int(nd["index"]), " ".join(repr(float(v)) for v in nd["pose"])))
    for nd in nodes:
        if int(nd["prev"]) < 0:
            continue
        lines.append(_g2o_edge(nd["index"], nd["prev"], nd["t_be"], nd["information"]))
    for e in (edges if edges is not None else ()):
        if int(e["success"]):
            lines.append(_g2o_edge(e["to"], e["from"], e["t_be"], e["information"]))
    return "".join(l + "\n" for l in lines)


def _g2o_info(v, information):
    tri = iter(v)
    for i in range(3):
        for j in range(i, 3):
            x = next(tri)
            information[G2O_INFO[i], G2O_INFO[j]] = x
            information[G2O_INFO[j], G2O_INFO[i]] = x


def _g2o_lines(path):
    """-> (vertices [(index, pose)], edges [(a, b, nine floats)], the first `EDGE_SE2 a a-1` of every a: a node's own edge)"""
    verts, edges, own = [], [], {}
    with open(path) as f:
        for line in f:
            w = line.split()
            if not w:
                continue
            if w[0] == "VERTEX_SE2":
                verts.append((int(w[1]), [float(v) for v in w[2:5]]))
            elif w[0] == "EDGE_SE2":
                a, b = int(w[1]), int(w[2])
                if b == a - 1 and a not in own:
                    own[a] = len(edges)
                edges.append((a, b, [float(v) for v in w[3:12]]))
    return verts, edges, own


def read_g2o(path):
    """write_g2o's text -> nodes (KEYFRAME_NODE_DTYPE) in file order: index, pose, prev (-1 without an edge), t_be and the (x, y, yaw)
    block of the information, both triangles; what the text does not carry (sweep, n_cells, motion, the other information entries) is 0.
    A node's own edge is the one to index - 1 (the first such line); the other edges of the file are read_g2o_edges'."""
    verts, edges, own = _g2o_lines(path)
    nodes = np.zeros(len(verts), dtype=capi.KEYFRAME_NODE_DTYPE)
    for k, (idx, pose) in enumerate(verts):
        nodes[k]["index"], nodes[k]["pose"], nodes[k]["prev"] = idx, pose, -1
        if idx in own:
            _, prev, v = edges[own[idx]]
            nodes[k]["prev"], nodes[k]["t_be"] = prev, v[:3]
            _g2o_info(v[3:], nodes[k]["information"])
    return nodes


def read_g2o_edges(path):
    """The edges of write_g2o's text that are no node's own (read_g2o) -> KEYFRAME_EDGE_DTYPE in file order: to, from, t_be and the (x, y,
    yaw) block of the information, both triangles, success = usable = 1; what the text does not carry is 0."""
    _, edges, own = _g2o_lines(path)
    mine = set(own.values())
    rest = [e for k, e in enumerate(edges) if k not in mine]
    out = np.zeros(len(rest), dtype=capi.KEYFRAME_EDGE_DTYPE)
    for k, (a, b, v) in enumerate(rest):
        out[k]["to"], out[k]["from"], out[k]["t_be"], out[k]["success"], out[k]["usable"] = a, b, v[:3], 1, 1
        _g2o_info(v[3:], out[k]["information"])
    return out


def rebase_trajectory(poses, nodes, optimised):
    """The per-sweep trajectory of one sequence carried onto its optimised keyframes: for each sweep s, T'_s = T'_k * T_k^-1 * T_s with k the
    last keyframe whose `sweep` <= s (T_k the node's recorded pose, T'_k its optimised one). poses [n, 3] (x, y, theta), nodes
    KEYFRAME_NODE_DTYPE (or anything with "sweep" and "pose"), optimised [len(nodes), 3] (Odometry.keyframe_optimize) -> [n, 3]. Sweeps in
    front of the first keyframe stay. Headings are not wrapped. Pure numpy (no device)."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    opt = np.asarray(optimised, dtype=np.float64).reshape(-1, 3)
    kp = np.asarray(nodes["pose"], dtype=np.float64).reshape(-1, 3)
    sweep = np.asarray(nodes["sweep"], dtype=np.int64).reshape(-1)
    if len(opt) != len(kp):
        raise ValueError("rebase_trajectory: %d optimised poses for %d nodes" % (len(opt), len(kp)))
    out = poses.copy()
    k = np.searchsorted(sweep, np.arange(len(poses)), side="right") - 1
    has = k >= 0
    k = k[has]
    c, s = np.cos(kp[k, 2]), np.sin(kp[k, 2])
    dx, dy = poses[has, 0] - kp[k, 0], poses[has, 1] - kp[k, 1]
    rx, ry, rt = c * dx + s * dy, -s * dx + c * dy, poses[has, 2] - kp[k, 2]
    c, s = np.cos(opt[k, 2]), np.sin(opt[k, 2])
    out[has] = np.stack([opt[k, 0] + c * rx - s * ry, opt[k, 1] + s * rx + c * ry, opt[k, 2] + rt], axis=1)
    return out


def write_keyframe_clouds(path, clouds, peaks=None):
    """The recorded clouds of one run as one .npz: clouds / peaks are per sequence a list of float32 [n, 3] arrays, one per node
    (capi.Odometry.keyframe_cloud(q, i) / (q, i, peaks=True); peaks None: a run without peaks clouds). Per sequence q the file holds the
    packed points `cloud_q` [N, 3] and `cloud_off_q` [nodes + 1] (node i is cloud_q[off[i]:off[i + 1]]), and `peaks_q` / `peaks_off_q`
    alike. read_keyframe_clouds gives back the same bits. Pure Python (no device)."""
    arrays = {"n_sequences": np.array(len(clouds), dtype=np.int64), "has_peaks": np.array(0 if peaks is None else 1, dtype=np.int64)}
    if peaks is not None and len(peaks) != len(clouds):
        raise ValueError("write_keyframe_clouds: %d sequences of clouds, %d of peaks" % (len(clouds), len(peaks)))
    for name, per_seq in (("cloud", clouds), ("peaks", peaks)):
        if per_seq is None:
            continue
        for q, lst in enumerate(per_seq):
            lst = [np.ascontiguousarray(c, dtype=np.float32).reshape(-1, 3) for c in lst]
            arrays["%s_off_%d" % (name, q)] = np.concatenate([[0], np.cumsum([len(c) for c in lst])]).astype(np.int64)
            arrays["%s_%d" % (name, q)] = np.concatenate(lst, axis=0) if lst else np.zeros((0, 3), dtype=np.float32)
    with open(path, "wb") as f:  # (a file object: np.savez would append .npz to a bare name)
        np.savez(f, **arrays)


def read_keyframe_clouds(path):
    """write_keyframe_clouds' file -> (clouds, peaks): per sequence a list of float32 [n, 3] arrays, one per node; peaks is None for a file
    without peaks clouds."""
    out = []
    with np.load(path) as z:
        for name in ("cloud", "peaks"):
            if name == "peaks" and not int(z["has_peaks"]):
                out.append(None)
                continue
            per_seq = []
            for q in range(int(z["n_sequences"])):
                off, pts = z["%s_off_%d" % (name, q)], z["%s_%d" % (name, q)]
                per_seq.append([np.array(pts[off[i]:off[i + 1]]) for i in range(len(off) - 1)])
            out.append(per_seq)
    return out[0], out[1]


def replay_grid(frames, rows, A=None, R=None, gt=None, device=0, piece=256, context_params=None, options=None, drift_on="host", keyframes=None,
                max_keyframes=None, max_cells=None, max_points=None, edges=None, optimise=None):
    """One recording under len(rows) parameter sets in one batched odometry object: frames uint8 [n, A, R], rows a list of capi.Params that
    agree in the object-wide fields (param_grid of one base does; k_strongest and submap_scan_size may be axes: the context then runs with
    the largest of each, grid_context_params, unless context_params says otherwise; so may cost: rows that differ from the context in cost
    or submap_scan_size run under their own shapes, grid_shapes). The recording is the single source sweep of every sequence: it is
    copied and filtered once per sweep. Rows of filter_type CA-CFAR (cfar_grid) run under their own detectors over that one source
    (Odometry.set_sequence_detectors): the sweep is staged and its prefix sums built once, every distinct detector decided once. options: a capi.FuserOptions for every row or a list of one per row (fuser_grid builds both
    lists); None: the fuser's defaults. -> dict(poses [n, len(rows), 3], records, drift: per row KITTI drift against gt ([n, 4, 4]
    poses) or None). drift_on: "host" - kitti.drift row by row; "device" - all rows in one cfear_drift_host call against a plan of
    gt[:n] (capi.DriftPlan), each row's dict then also holds the per-length table as kitti.drift_by_length returns it.
    keyframes: None, "nodes" or "cells" - record every row's keyframe graph on the device (Odometry.record_keyframes; max_keyframes per row,
    default n: every sweep may fuse; max_cells per row, default 256 * n - 18 KB per sweep and row; a scan of the reference's presets has 150-400
    cells and about every second sweep fuses: size it yourself for a grid of many rows or dense scans, `keyframes_dropped` says when it was too small) and add `keyframes`: a list of
    per-row node arrays (KEYFRAME_NODE_DTYPE), `keyframes_dropped` [rows] and, with "cells", `keyframe_cells`: per row a list of cell
    arrays (KEYFRAME_CELL_DTYPE), one per node. keyframes="clouds": the nodes and their two clouds (capi.KF_CLOUD | capi.KF_PEAKS; max_points per
    row, default n * A * k_strongest of the context - 12 bytes a point: size it yourself for a long recording) -> `keyframe_clouds` and
    `keyframe_peaks`: per row a list of float32 [points, 3] arrays (x, y, intensity), one per node - what write_keyframe_clouds takes.
    edges (with keyframes="cells"): dict(min_index_gap=, max_dist=, n_side=, max_per_node=), each optional - every row's loop_candidates from
    its own nodes, registered as edge_jobs for all rows in ONE Odometry.keyframe_edges call, each row under its own parameters -> `keyframe_edges`:
    per row an array of KEYFRAME_EDGE_DTYPE (what write_g2o takes beside the row's nodes).
    keyframes="cells+clouds": both logs ("cells" and "clouds" together). With it edges=dict(appearance=dict(<capi.ScParams fields>), n_side=) proposes
    the loop pairs by appearance instead - all rows' candidates from ONE Odometry.keyframe_candidates call (Scan-Context descriptors of the
    recorded clouds, no pose involved), registered as appearance_jobs in ONE keyframe_edges call -> `keyframe_candidates` (per row,
    SC_CANDIDATE_DTYPE) beside `keyframe_edges`.
    optimise (with keyframes): a dict of capi.pg_options fields (may be empty) - every row's graph, its chain and with edges= its loop edges,
    optimised in ONE Odometry.keyframe_optimize call -> `keyframe_poses_optimised`: per row [nodes, 3], `optimise_summaries`
    (capi.PG_SUMMARY_DTYPE [rows]), `poses_optimised` [n, rows, 3]: every row's trajectory carried onto its optimised keyframes
    (rebase_trajectory) and, with gt, `drift_optimised`: its drift beside `drift`, scored the same way. None: nothing of this runs."""
    if drift_on not in ("host", "device"):
        raise ValueError("replay_grid: drift_on is 'host' or 'device'")
    if keyframes not in (None, "nodes", "cells", "clouds", "cells+clouds"):
        raise ValueError("replay_grid: keyframes is None, 'nodes', 'cells', 'clouds' or 'cells+clouds'")
    if edges is not None and keyframes not in ("cells", "cells+clouds"):
        raise ValueError("replay_grid: edges need keyframes='cells' (the keyframes are registered from their recorded cells)")
    if edges is not None and "appearance" in edges:
        if keyframes != "cells+clouds":
            raise ValueError("replay_grid: edges by appearance need keyframes='cells+clouds' (the candidates are matched on the recorded clouds)")
        if set(edges) - {"appearance", "n_side"}:
            raise ValueError("replay_grid: edges by appearance take appearance (a dict of capi.ScParams fields) and n_side")
    elif edges is not None and set(edges) - {"min_index_gap", "max_dist", "n_side", "max_per_node"}:
        raise ValueError("replay_grid: edges takes min_index_gap, max_dist, n_side and max_per_node")
    if optimise is not None and keyframes is None:
        raise ValueError("replay_grid: optimise needs keyframes (the graphs are the recorded ones)")
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    n, A, R = frames.shape
    rows = list(rows)
    piece = max(1, int(piece))
    cpar = context_params if context_params is not None else grid_context_params(rows)
    ctx = capi.Context(cpar, A, R, device=device)
    odo = None
    try:
        odo = ctx.odometry(len(rows))
        shapes = grid_shapes(rows, cpar)
        if shapes is not None:
            odo.set_sequence_shapes(shapes)
        if int(cpar.filter_type) == capi.FILTER_CACFAR:  # every row its own detector over the one source (cfar_grid), then the table that carries them
            odo.set_sequence_detectors(grid_detectors(rows), np.zeros(len(rows), dtype=np.int32), 1)
            odo.set_sequence_params(rows)
        else:
            odo.set_sequence_params(rows)
            odo.set_sequence_sources(np.zeros(len(rows), dtype=np.int32), 1)
        if options is not None:
            opts = options if isinstance(options, capi.FuserOptions) else list(options)
            if not isinstance(opts, capi.FuserOptions) and len(opts) != len(rows):
                raise ValueError("replay_grid: %d option sets for %d rows" % (len(opts), len(rows)))
            odo.set_fuser_options(opts)
        if keyframes is not None:
            what = capi.KF_NODES | {"nodes": 0, "cells": capi.KF_CELLS, "clouds": capi.KF_CLOUD | capi.KF_PEAKS,
                                    "cells+clouds": capi.KF_CELLS | capi.KF_CLOUD | capi.KF_PEAKS}[keyframes]
            odo.record_keyframes(what, max_keyframes if max_keyframes is not None else n, max_cells if max_cells is not None else 256 * n,
                                 max_points if max_points is not None else n * A * int(cpar.k_strongest))
        recs = [odo.replay_host(frames[t0:t0 + piece, None]) for t0 in range(0, n, piece)]
        rec = np.concatenate(recs, axis=0)
        poses = np.array(rec["pose"])
        graph = None
        if keyframes is not None:
            graph = {"keyframes": [odo.keyframes(q) for q in range(len(rows))], "keyframes_dropped": odo.keyframe_counts()[1]}
            if keyframes in ("cells", "cells+clouds"):
                graph["keyframe_cells"] = [[odo.keyframe_cells(q, i) for i in range(len(nodes))] for q, nodes in enumerate(graph["keyframes"])]
            if edges is not None and "appearance" in edges:
                graph["keyframe_candidates"], graph["keyframe_edges"] = grid_appearance_edges(odo, graph["keyframes"], edges["appearance"], edges.get("n_side", 0))
            elif edges is not None:
                graph["keyframe_edges"] = grid_edges(odo, graph["keyframes"], **edges)
            if keyframes in ("clouds", "cells+clouds"):
                graph["keyframe_clouds"] = [[odo.keyframe_cloud(q, i) for i in range(len(nodes))] for q, nodes in enumerate(graph["keyframes"])]
                graph["keyframe_peaks"] = [[odo.keyframe_cloud(q, i, peaks=True) for i in range(len(nodes))] for q, nodes in enumerate(graph["keyframes"])]
        rebased = None
        if optimise is not None:
            loops = np.concatenate(graph["keyframe_edges"]) if edges is not None else None
            graph["keyframe_poses_optimised"], graph["optimise_summaries"] = odo.keyframe_optimize(loops, **optimise)
            rebased = np.stack([rebase_trajectory(poses[:, q], graph["keyframes"][q], graph["keyframe_poses_optimised"][q]) for q in range(len(rows))], axis=1)
            graph["poses_optimised"] = rebased
        scored = scored_opt = None
        if gt is not None and drift_on == "device":
            plan = ctx.drift_plan(np.asarray(gt)[:n])
            try:
                scored = plan.score(poses)
                if rebased is not None:
                    scored_opt = plan.score(rebased)
            finally:
                plan.release()
    finally:
        if odo is not None:
            odo.release()
        ctx.close()
    drift = None
    if scored is not None:
        drift = [drift_dict(r) for r in scored]
    elif gt is not None:
        drift = [kitti.drift(np.asarray(gt)[:n], kitti.poses_from_xyt(poses[:, q])) for q in range(len(rows))]
    out = {"poses": poses, "records": rec, "drift": drift}
    if graph is not None:
        out.update(graph)
    if rebased is not None and gt is not None:
        if scored_opt is not None:
            out["drift_optimised"] = [drift_dict(r) for r in scored_opt]
        else:
            out["drift_optimised"] = [kitti.drift(np.asarray(gt)[:n], kitti.poses_from_xyt(rebased[:, q])) for q in range(len(rows))]
    return out


def grid_edges(odo, nodes_per_row, min_index_gap=6, max_dist=3.0, n_side=0, max_per_node=None):
    """The loop candidates of every sequence of `odo` (loop_candidates on nodes_per_row[q]) as edge_jobs, all of them in one
    keyframe_edges call -> per sequence the edges of its candidates, in loop_candidates' order"""
    jobs = [edge_jobs(q, loop_candidates(nodes, min_index_gap, max_dist, max_per_node), n_side, len(nodes)) for q, nodes in enumerate(nodes_per_row)]
    count = [len(j) for j in jobs]
    if sum(count) == 0:
        return [np.zeros(0, dtype=capi.KEYFRAME_EDGE_DTYPE) for _ in jobs]
    got = odo.keyframe_edges(np.concatenate(jobs))
    cuts = np.cumsum([0] + count)
    return [got[cuts[q]:cuts[q + 1]].copy() for q in range(len(jobs))]


def grid_appearance_edges(odo, nodes_per_row, appearance=None, n_side=0):
    """Loop edges by appearance for every sequence of `odo`: the candidates of all sequences from ONE keyframe_candidates call (Scan-Context
    descriptors of the recorded clouds, matched on the device; appearance: a dict of capi.ScParams fields), as appearance_jobs all of them
    in ONE keyframe_edges call -> (per sequence its candidates, SC_CANDIDATE_DTYPE; per sequence the edges of its candidates, in their order)"""
    cand = odo.keyframe_candidates(**(appearance or {}))
    per_row = [cand[cand["sequence"] == q] for q in range(len(nodes_per_row))]
    jobs = [appearance_jobs(q, per_row[q], nodes, n_side) for q, nodes in enumerate(nodes_per_row)]
    count = [len(j) for j in jobs]
    if sum(count) == 0:
        return per_row, [np.zeros(0, dtype=capi.KEYFRAME_EDGE_DTYPE) for _ in jobs]
    got = odo.keyframe_edges(np.concatenate(jobs))
    cuts = np.cumsum([0] + count)
    return per_row, [got[cuts[q]:cuts[q + 1]].copy() for q in range(len(jobs))]


def sweeps(args):
    if args.bag:
        for kind, t, payload in readers.BagReader(args.bag).sweeps_and_gt(args.image_topic, args.gt_topic):
            yield (kind, t, payload if kind == "gt" else readers.polar_image(payload, args.dataset))
    else:
        for path in sorted(glob.glob(os.path.join(args.oxford_png_dir, "*.png"))):
            d = readers.read_oxford_png(path)
            yield ("image", int(d["timestamps"][0]) * 1000, d["polar"])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--bag")
    src.add_argument("--oxford_png_dir")
    ap.add_argument("--dataset", default="oxford")
    ap.add_argument("--image_topic", default="/Navtech/Polar")
    ap.add_argument("--gt_topic", default="/gt")
    ap.add_argument("--est_directory", default=".")
    ap.add_argument("--gt_directory", default=None)
    ap.add_argument("--max_frames", type=int, default=0)
    # defaults of offline_odometry.cpp:155-187
    ap.add_argument("--range-res", dest="range_res", type=float, default=0.0438)
    ap.add_argument("--z-min", dest="z_min", type=float, default=65.0)
    ap.add_argument("--k_strongest", type=int, default=12)
    ap.add_argument("--min_distance", type=float, default=2.5)
    ap.add_argument("--res", type=float, default=3.5)
    ap.add_argument("--submap_scan_size", type=int, default=3)
    ap.add_argument("--weight_intensity", type=int, default=1)
    ap.add_argument("--weight_option", type=int, default=0)
    ap.add_argument("--cost_type", default="P2L", choices=["P2P", "P2L", "P2D"])
    ap.add_argument("--loss_type", default="Huber", choices=["None", "Huber", "Cauchy", "SoftLOne", "Combined", "Tukey"])
    ap.add_argument("--loss_limit", type=float, default=0.1)
    ap.add_argument("--radar_ccw", type=int, default=0)
    ap.add_argument("--disable_compensate", type=int, default=0)
    ap.add_argument("--registered_min_keyframe_dist", type=float, default=1.5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--piece", type=int, default=256, help="sweeps handed to one cfear_odometry_replay_host call (pinned staging buffer)")
    ap.add_argument("--store_graph", default=None, metavar="PATH",
                    help="record the keyframe graph on the device (offline_odometry --store_graph) and write it to PATH as g2o text (write_g2o)")
    ap.add_argument("--max_keyframes", type=int, default=65536, help="with --store_graph: nodes the log holds (later keyframes are dropped and reported)")
    ap.add_argument("--loop_edges", default=None, metavar="GAP,DIST[,SIDE]",
                    help="with --store_graph: also register every keyframe against the keyframes at least GAP nodes earlier and within DIST metres of it "
                         "(loop_candidates; SIDE neighbours on each side of the candidate join it, default 0) in one batch and append the edges to the graph")
    ap.add_argument("--loop_edges_appearance", default=None, metavar="GAP,MAX_DISTANCE[,SIDE]",
                    help="with --store_graph: propose the loop pairs by appearance instead of by pose - Scan-Context descriptors of the recorded clouds, matched "
                         "on the device (Odometry.keyframe_candidates: keyframes at least GAP nodes apart whose descriptor distance is at most MAX_DISTANCE) - "
                         "register them in one batch with the match's yaw as the guess and append the edges to the graph")
    ap.add_argument("--optimize", action="store_true",
                    help="with --store_graph: optimise the graph - the chain and, with --loop_edges, the loop edges - on the device (Odometry.keyframe_optimize) "
                         "and write the optimised vertices; the edges are written as recorded")
    ap.add_argument("--optimize_loss", default="None", choices=["None", "Huber", "Cauchy"], help="with --optimize: the loss on the loop edges")
    ap.add_argument("--optimize_loss_limit", type=float, default=1.0, help="with --optimize_loss: its limit, on the edge's whitened error")
    ap.add_argument("--max_cells", type=int, default=4194304, help="with --loop_edges: cells the log holds, 72 bytes each (later keyframes are dropped and reported)")
    ap.add_argument("--store_clouds", default=None, metavar="PATH",
                    help="with --store_graph: also record every node's motion-compensated filtered and peaks cloud and write them to PATH (.npz, write_keyframe_clouds)")
    ap.add_argument("--max_points", type=int, default=16777216, help="with --store_clouds: points the log holds, 12 bytes each (later keyframes are dropped and reported)")
    ap.add_argument("--trace", action="store_true",
                    help="keep per-sweep poses, Register summaries (outer / inner iteration counts, residuals), keyframe and cell counts in the result")
    args = ap.parse_args(argv)
    if args.store_clouds and not args.store_graph:
        ap.error("--store_clouds needs --store_graph (the clouds belong to the graph's nodes)")
    if args.optimize and not args.store_graph:
        ap.error("--optimize needs --store_graph (the graph that is optimised is the one that is written)")
    loop = None
    if args.loop_edges:
        if not args.store_graph:
            ap.error("--loop_edges needs --store_graph (the edges join the graph's nodes)")
        w = args.loop_edges.split(",")
        if len(w) not in (2, 3):
            ap.error("--loop_edges takes GAP,DIST[,SIDE]")
        loop = dict(min_index_gap=int(w[0]), max_dist=float(w[1]), n_side=int(w[2]) if len(w) == 3 else 0)
    appearance = None
    if args.loop_edges_appearance:
        if not args.store_graph:
            ap.error("--loop_edges_appearance needs --store_graph (the edges join the graph's nodes)")
        if args.loop_edges:
            ap.error("--loop_edges_appearance and --loop_edges propose the same edges in two ways: give one")
        w = args.loop_edges_appearance.split(",")
        if len(w) not in (2, 3):
            ap.error("--loop_edges_appearance takes GAP,MAX_DISTANCE[,SIDE]")
        appearance = dict(appearance=dict(min_index_gap=int(w[0]), max_distance=float(w[1])), n_side=int(w[2]) if len(w) == 3 else 0)
    cost = {"P2P": 0, "P2L": 1, "P2D": 2}[args.cost_type]
    loss = {"None": 0, "Huber": 1, "Cauchy": 2, "SoftLOne": 3, "Combined": 4, "Tukey": 5}[args.loss_type]
    import time
    ctx = odo = buf = None
    est, gts, n, trace = [], [], 0, []
    first_gt = None
    fill = 0
    t_wall0 = time.perf_counter()
    t_dev = 0.0

    def flush():
        # offline_odometry.cpp:103-125 for the sweeps collected so far: one cfear_odometry_replay_host call (no host round trip per
        # sweep; the sweeps sit in pinned memory, so their copies overlap with the kernels of the chunk before)
        nonlocal fill, t_dev
        if fill == 0:
            return
        t0 = time.perf_counter()
        rec = odo.replay_host(buf[:fill])[:, 0]
        t_dev += time.perf_counter() - t0
        for r in rec:
            est.append(np.array(r["pose"]))
            if args.trace:
                no = min(max(int(r["outer_iterations"]), 0), 8)
                trace.append({"outer": int(r["outer_iterations"]), "inner": [int(v) for v in r["inner_iterations"][:no]], "residuals": int(r["num_residuals"]),
                              "final_cost": float(r["final_cost"]), "keyframes": int(r["n_keyframes"]), "cells": int(r["n_cells"])})
        fill = 0

    for kind, t, payload in sweeps(args):
        if kind == "gt":
            x, y, th = payload  # relative to the first ground-truth pose (offline_odometry.cpp:91-92)
            T = kitti.poses_from_xyt([[x, y, th]])[0]
            if first_gt is None:
                first_gt = np.linalg.inv(T)
            gts.append(first_gt @ T)
            continue
        img = payload
        if ctx is None:
            p = capi.default_params(range_res=np.float32(args.range_res), z_min=args.z_min, k_strongest=args.k_strongest, min_distance=args.min_distance,
                                    res=args.res, submap_scan_size=args.submap_scan_size, weight_intensity=args.weight_intensity,
                                    weight_opt=args.weight_option, cost=cost, loss=loss, loss_limit=args.loss_limit, radar_ccw=args.radar_ccw,
                                    compensate=0 if args.disable_compensate else 1, min_keyframe_dist=args.registered_min_keyframe_dist)
            ctx = capi.Context(p, img.shape[0], img.shape[1], device=args.device)
            odo = ctx.odometry(1)
            if args.store_graph:
                odo.record_keyframes(capi.KF_NODES | (capi.KF_CELLS if loop or appearance else 0) |
                                     (capi.KF_CLOUD | capi.KF_PEAKS if args.store_clouds or appearance else 0), args.max_keyframes,
                                     args.max_cells if loop or appearance else 0, args.max_points)
            buf = ctx.pinned((max(1, args.piece), 1, img.shape[0], img.shape[1]))
        buf[fill, 0] = img
        fill += 1
        n += 1
        if fill == buf.shape[0]:
            flush()
        if args.max_frames and n >= args.max_frames:
            break
    if ctx is not None:
        flush()
    t_wall = time.perf_counter() - t_wall0
    if not est:
        raise SystemExit("no radar sweeps found")
    os.makedirs(args.est_directory, exist_ok=True)
    est_T = kitti.poses_from_xyt(np.array(est))
    kitti.write_kitti(os.path.join(args.est_directory, "est_00.txt"), est_T)
    # the rate offline_odometry.cpp:125 prints (frames / second): of the device part alone and of the whole loop incl. reading / decoding
    out = {"frames": n, "final_pose": [float(v) for v in est[-1]], "sweeps_per_s_device": n / t_dev if t_dev > 0 else None,
           "sweeps_per_s_with_reading": n / t_wall if t_wall > 0 else None}
    if gts:
        gdir = args.gt_directory or args.est_directory
        os.makedirs(gdir, exist_ok=True)
        m = min(len(gts), len(est_T))
        kitti.write_kitti(os.path.join(gdir, "gt_00.txt"), gts[:m])
        out["drift"] = kitti.drift(np.array(gts[:m]), est_T[:m])
    if args.store_graph:
        nodes = odo.keyframes(0)
        loop_edges = grid_edges(odo, [nodes], **loop)[0] if loop else None
        if appearance:
            cand, per_row = grid_appearance_edges(odo, [nodes], appearance["appearance"], appearance["n_side"])
            loop_edges = per_row[0]
            out["appearance_candidates"] = int(len(cand[0]))
        if args.optimize:
            opt, sums = odo.keyframe_optimize(loop_edges, loss={"None": 0, "Huber": 1, "Cauchy": 2}[args.optimize_loss], loss_limit=args.optimize_loss_limit)
            nodes = nodes.copy()
            nodes["pose"] = opt[0]
            out["optimize"] = {f: (float(sums[0][f]) if f.endswith("_cost") else int(sums[0][f])) for f in capi.PG_SUMMARY_DTYPE.names if f != "pad_"}
            out["optimize"]["termination"] = capi.PG_TERMINATION[int(sums[0]["termination"])]
        write_g2o(args.store_graph, nodes, loop_edges)
        out["keyframes"] = int(len(nodes))
        if appearance:
            out["loop_edges"] = int(np.count_nonzero(loop_edges["success"]))
        if loop:
            out["loop_candidates"], out["loop_edges"] = int(len(loop_edges)), int(np.count_nonzero(loop_edges["success"]))
        out["keyframes_dropped"] = int(odo.keyframe_counts()[1][0])
        if args.store_clouds:
            write_keyframe_clouds(args.store_clouds, [[odo.keyframe_cloud(0, i) for i in range(len(nodes))]],
                                  [[odo.keyframe_cloud(0, i, peaks=True) for i in range(len(nodes))]])
            nc, npk = odo.keyframe_cloud_sizes(0)
            out["cloud_points"], out["peaks_points"] = int(nc.sum()), int(npk.sum())
    print(json.dumps(out))
    if args.trace:
        out["poses"] = np.array(est)
        out["trace"] = trace
    odo.release()
    ctx.close()
    return out


if __name__ == "__main__":
    main()
