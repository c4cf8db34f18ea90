"""ctypes binding of include/cfear_hip.h (no torch types cross this boundary)."""
import ctypes as C
import os

import numpy as np

from . import build as _build

_LIB = None
CFEAR_MAX_OUTER = 64


class CfearError(RuntimeError):
    pass


class Params(C.Structure):
    """cfear_params (include/cfear_hip.h)."""
    _fields_ = [
        ("z_min", C.c_float), ("range_res", C.c_float), ("min_distance", C.c_float),
        ("k_strongest", C.c_int32),
        ("res", C.c_double), ("downsample_factor", C.c_double),
        ("weight_intensity", C.c_int32), ("cost", C.c_int32), ("loss", C.c_int32),
        ("weight_opt", C.c_int32),
        ("loss_limit", C.c_double), ("covar_scale", C.c_double), ("regularization", C.c_double),
        ("submap_scan_size", C.c_int32), ("compensate", C.c_int32), ("radar_ccw", C.c_int32),
        ("use_keyframe", C.c_int32),
        ("min_keyframe_dist", C.c_double), ("min_keyframe_rot_deg", C.c_double),
        ("max_itr_association", C.c_int32), ("min_itr", C.c_int32),
        ("max_solver_iterations", C.c_int32), ("filter_type", C.c_int32),
        ("assoc_radius", C.c_double),
        ("cfar_window_size", C.c_int32), ("cfar_nb_guard_cells", C.c_int32), ("cfar_false_alarm_rate", C.c_float), ("cfar_max_points", C.c_int32),
        ("cfar_max_distance", C.c_double),
    ]


FILTER_KSTRONG, FILTER_CACFAR = 0, 1


class FuserOptions(C.Structure):
    """cfear_fuser_options (include/cfear_hip.h): the fuser's soft_constraint and use_guess (odometrykeyframefuser.h:94) of a batched
    odometry object or of one of its sequences"""
    _fields_ = [("soft_constraint", C.c_int32), ("use_guess", C.c_int32)]

    def __repr__(self):
        return "FuserOptions(soft_constraint=%d, use_guess=%d)" % (self.soft_constraint, self.use_guess)


class SeqShape(C.Structure):
    """cfear_seq_shape (include/cfear_hip.h): the cost metric and the submap_scan_size of one sequence of a batched odometry object"""
    _fields_ = [("cost", C.c_int32), ("submap_scan_size", C.c_int32)]

    def __repr__(self):
        return "SeqShape(cost=%d, submap_scan_size=%d)" % (self.cost, self.submap_scan_size)


class SeqDetector(C.Structure):
    """cfear_seq_detector (include/cfear_hip.h): the CA-CFAR detector of one cloud of Context.filter_cfar_grid or of one sequence of a
    filter_type CA-CFAR batched odometry object (Odometry.set_sequence_detectors)"""
    _fields_ = [("window_size", C.c_int32), ("nb_guard_cells", C.c_int32), ("false_alarm_rate", C.c_float), ("z_min", C.c_float)]

    def __repr__(self):
        return "SeqDetector(window_size=%d, nb_guard_cells=%d, false_alarm_rate=%g, z_min=%g)" % (
            self.window_size, self.nb_guard_cells, self.false_alarm_rate, self.z_min)


def detector_array(dets):
    """a list of SeqDetector / (window_size, nb_guard_cells, false_alarm_rate, z_min) tuples -> a ctypes array of SeqDetector (handed on as it
    is when it already is one: a caller that repeats a large grid builds it once)"""
    if isinstance(dets, C.Array) and dets._type_ is SeqDetector:
        return dets
    dets = [d if isinstance(d, SeqDetector) else SeqDetector(int(d[0]), int(d[1]), float(d[2]), float(d[3])) for d in dets]
    return (SeqDetector * len(dets))(*dets)


class Cell(C.Structure):
    _fields_ = [
        ("mean", C.c_double * 2), ("cov", C.c_double * 3), ("normal", C.c_double * 2),
        ("orth", C.c_double * 2), ("lambda_min", C.c_double), ("lambda_max", C.c_double),
        ("scale", C.c_double), ("sum_intensity", C.c_double), ("avg_intensity", C.c_double),
        ("nsamples", C.c_int32), ("valid", C.c_int32),
    ]


CELL_DTYPE = np.dtype([
    ("mean", "f8", 2), ("cov", "f8", 3), ("normal", "f8", 2), ("orth", "f8", 2),
    ("lambda_min", "f8"), ("lambda_max", "f8"), ("scale", "f8"), ("sum_intensity", "f8"),
    ("avg_intensity", "f8"), ("nsamples", "i4"), ("valid", "i4")])


class RegSummary(C.Structure):
    _fields_ = [
        ("success", C.c_int32), ("usable", C.c_int32), ("outer_iterations", C.c_int32),
        ("num_residuals", C.c_int32), ("num_residual_blocks", C.c_int32), ("assoc_path", C.c_int32),
        ("final_cost", C.c_double), ("score", C.c_double),
        ("inner_iterations", C.c_int32 * CFEAR_MAX_OUTER), ("termination", C.c_int32 * CFEAR_MAX_OUTER),
        ("outer_cost", C.c_double * CFEAR_MAX_OUTER), ("outer_pose", (C.c_double * 3) * CFEAR_MAX_OUTER),
    ]


# cfear_sweep_record (include/cfear_hip.h): what a caller of pointcloudCallback sees after every sweep of a replay
SWEEP_RECORD_DTYPE = np.dtype([("pose", "f8", 3), ("final_cost", "f8"), ("outer_iterations", "i4"), ("num_residuals", "i4"),
                               ("n_keyframes", "i4"), ("n_cells", "i4"), ("inner_iterations", "i4", 8)])
assert SWEEP_RECORD_DTYPE.itemsize == 80


# cfear_keyframe_node / cfear_keyframe_cell (include/cfear_hip.h): the keyframe graph of the batched routes (AddToGraph,
# odometrykeyframefuser.cpp:428-445): a RadarScan node with its odometry constraint to the previous keyframe, and one of its cells
class KeyframeNode(C.Structure):
    _fields_ = [("index", C.c_int32), ("sweep", C.c_int32), ("n_cells", C.c_int32), ("prev", C.c_int32), ("pose", C.c_double * 3),
                ("motion", C.c_double * 3), ("t_be", C.c_double * 3), ("information", C.c_double * 36)]


class KeyframeCell(C.Structure):
    _fields_ = [("mean", C.c_double * 2), ("normal", C.c_double * 2), ("cov", C.c_double * 3), ("scale", C.c_double),
                ("nsamples", C.c_int32), ("pad_", C.c_int32)]


KEYFRAME_NODE_DTYPE = np.dtype([("index", "i4"), ("sweep", "i4"), ("n_cells", "i4"), ("prev", "i4"), ("pose", "f8", 3), ("motion", "f8", 3),
                                ("t_be", "f8", 3), ("information", "f8", (6, 6))])
KEYFRAME_CELL_DTYPE = np.dtype([("mean", "f8", 2), ("normal", "f8", 2), ("cov", "f8", 3), ("scale", "f8"), ("nsamples", "i4"), ("pad_", "i4")])
assert KEYFRAME_NODE_DTYPE.itemsize == C.sizeof(KeyframeNode) == 376 and KEYFRAME_CELL_DTYPE.itemsize == C.sizeof(KeyframeCell) == 72
KF_EDGE_MAX_FROM = 16  # CFEAR_KF_EDGE_MAX_FROM


# cfear_keyframe_edge_job / cfear_keyframe_edge (include/cfear_hip.h): a constraint between any keyframes of a log - keyframe `to`
# registered against the fixed keyframes `from` (cfear_odometry_keyframe_edges)
class KeyframeEdgeJob(C.Structure):
    _fields_ = [("sequence", C.c_int32), ("to", C.c_int32), ("n_from", C.c_int32), ("ref", C.c_int32), ("flags", C.c_int32), ("pad_", C.c_int32),
                ("from_", C.c_int32 * KF_EDGE_MAX_FROM), ("guess_xyt", C.c_double * 3)]


class KeyframeEdge(C.Structure):
    _fields_ = [("sequence", C.c_int32), ("to", C.c_int32), ("from_", C.c_int32), ("n_from", C.c_int32), ("status", C.c_int32), ("success", C.c_int32),
                ("usable", C.c_int32), ("outer_iterations", C.c_int32), ("num_residuals", C.c_int32), ("num_residual_blocks", C.c_int32),
                ("assoc_path", C.c_int32), ("pad_", C.c_int32), ("pose", C.c_double * 3), ("t_be", C.c_double * 3), ("final_cost", C.c_double),
                ("score", C.c_double), ("information", C.c_double * 36)]


KEYFRAME_EDGE_JOB_DTYPE = np.dtype([("sequence", "i4"), ("to", "i4"), ("n_from", "i4"), ("ref", "i4"), ("flags", "i4"), ("pad_", "i4"),
                                    ("from", "i4", KF_EDGE_MAX_FROM), ("guess_xyt", "f8", 3)])
KEYFRAME_EDGE_DTYPE = np.dtype([("sequence", "i4"), ("to", "i4"), ("from", "i4"), ("n_from", "i4"), ("status", "i4"), ("success", "i4"), ("usable", "i4"),
                                ("outer_iterations", "i4"), ("num_residuals", "i4"), ("num_residual_blocks", "i4"), ("assoc_path", "i4"), ("pad_", "i4"),
                                ("pose", "f8", 3), ("t_be", "f8", 3), ("final_cost", "f8"), ("score", "f8"), ("information", "f8", (6, 6))])
assert KEYFRAME_EDGE_JOB_DTYPE.itemsize == C.sizeof(KeyframeEdgeJob) == 112 and KEYFRAME_EDGE_DTYPE.itemsize == C.sizeof(KeyframeEdge) == 400


def keyframe_edge_jobs(jobs):
    """A job list for Odometry.keyframe_edges as a structured array of KEYFRAME_EDGE_JOB_DTYPE. jobs: such an array (returned as it is,
    contiguous), or a list whose entries are dicts - sequence, to, from (an index or a list of up to 16), and optionally ref (0) and guess
    (x, y, theta; absent or None: `to`'s recorded pose) - or tuples (sequence, to, from[, ref[, guess]]). Pure numpy (no device)."""
    if isinstance(jobs, np.ndarray) and jobs.dtype == KEYFRAME_EDGE_JOB_DTYPE:
        return np.ascontiguousarray(jobs).reshape(-1)
    out = np.zeros(len(jobs), dtype=KEYFRAME_EDGE_JOB_DTYPE)
    for k, j in enumerate(jobs):
        if isinstance(j, dict):
            seq, to, frm, ref, guess = j["sequence"], j["to"], j["from"], j.get("ref", 0), j.get("guess")
        else:
            j = tuple(j)
            seq, to, frm = j[:3]
            ref, guess = (j[3] if len(j) > 3 else 0), (j[4] if len(j) > 4 else None)
        frm = [int(v) for v in np.atleast_1d(frm)]
        if not 1 <= len(frm) <= KF_EDGE_MAX_FROM:
            raise CfearError("keyframe_edge_jobs: job %d names %d `from` keyframes (1 .. %d)" % (k, len(frm), KF_EDGE_MAX_FROM))
        out[k]["sequence"], out[k]["to"], out[k]["n_from"], out[k]["ref"] = int(seq), int(to), len(frm), int(ref)
        out[k]["from"][:len(frm)] = frm
        if guess is not None:
            out[k]["flags"], out[k]["guess_xyt"] = 1, np.asarray(guess, dtype=np.float64).reshape(3)
    return out


# cfear_pg_edge / cfear_pg_options / cfear_pg_summary (include/cfear_hip.h): the batched planar pose-graph optimiser (pose_graph.hip). An
# edge is a g2o `EDGE_SE2 a b ...` line as replay writes it; posegraph.py builds them from nodes and keyframe edges
class PgEdge(C.Structure):
    _fields_ = [("a", C.c_int32), ("b", C.c_int32), ("flags", C.c_int32), ("pad_", C.c_int32), ("z", C.c_double * 3), ("info", C.c_double * 6)]


class PgOptions(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("max_linear_iterations", C.c_int32), ("loss", C.c_int32), ("pad_", C.c_int32),
                ("linear_tolerance", C.c_double), ("function_tolerance", C.c_double), ("parameter_tolerance", C.c_double),
                ("initial_damping", C.c_double), ("loss_limit", C.c_double)]

    def __repr__(self):
        return "PgOptions(%s)" % ", ".join("%s=%r" % (f, getattr(self, f)) for f, _ in self._fields_ if f != "pad_")


class PgSummary(C.Structure):
    _fields_ = [("initial_cost", C.c_double), ("final_cost", C.c_double), ("iterations", C.c_int32), ("accepted", C.c_int32),
                ("linear_iterations", C.c_int32), ("edges_used", C.c_int32), ("edges_skipped", C.c_int32), ("termination", C.c_int32),
                ("status", C.c_int32), ("pad_", C.c_int32)]


PG_EDGE_DTYPE = np.dtype([("a", "i4"), ("b", "i4"), ("flags", "i4"), ("pad_", "i4"), ("z", "f8", 3), ("info", "f8", 6)])
PG_SUMMARY_DTYPE = np.dtype([("initial_cost", "f8"), ("final_cost", "f8"), ("iterations", "i4"), ("accepted", "i4"), ("linear_iterations", "i4"),
                             ("edges_used", "i4"), ("edges_skipped", "i4"), ("termination", "i4"), ("status", "i4"), ("pad_", "i4")])
assert PG_EDGE_DTYPE.itemsize == C.sizeof(PgEdge) == 88 and PG_SUMMARY_DTYPE.itemsize == C.sizeof(PgSummary) == 48 and C.sizeof(PgOptions) == 56
PG_CONVERGED_COST, PG_CONVERGED_STEP, PG_ITERATION_LIMIT, PG_DAMPING_LIMIT, PG_NOTHING_TO_DO = 0, 1, 2, 3, 4  # CFEAR_PG_*
PG_TERMINATION = ("converged on cost", "converged on step", "iteration limit", "damping limit", "nothing to do")
LOSS_NONE, LOSS_HUBER, LOSS_CAUCHY = 0, 1, 2  # CFEAR_LOSS_* the optimiser takes


def pg_options(**kw):
    """cfear_pg_default_options with fields replaced: max_iterations (50), max_linear_iterations (0 = 30 x nodes), linear_tolerance (1e-8),
    function_tolerance (1e-12), parameter_tolerance (1e-10), initial_damping (1e-4), loss (LOSS_NONE), loss_limit (0.1)"""
    o = PgOptions()
    lib().cfear_pg_default_options(C.byref(o))
    for k, v in kw.items():
        if k == "pad_" or not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def pose_graph_cost_host(poses, edges, loss=0, loss_limit=0.1):
    """cfear_pose_graph_cost_host (host only, no device): F of one graph at poses [n, 3] -> (cost, edges used, edges skipped)"""
    x = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    E = np.ascontiguousarray(edges, dtype=PG_EDGE_DTYPE).reshape(-1)
    cost, used, skipped = C.c_double(), C.c_int32(), C.c_int32()
    rc = lib().cfear_pose_graph_cost_host(x.ctypes.data, len(x), E.ctypes.data, len(E), int(loss), float(loss_limit), C.byref(cost), C.byref(used), C.byref(skipped))
    if rc != 0:
        raise CfearError("cfear_pose_graph_cost_host failed rc=%d" % rc)
    return cost.value, used.value, skipped.value


# cfear_sc_params / cfear_sc_candidate (include/cfear_hip.h): Scan-Context descriptors and loop candidates by appearance (scan_context.hip).
# scancontext.py states the definition in numpy
class ScParams(C.Structure):
    _fields_ = [("n_rings", C.c_int32), ("n_sectors", C.c_int32), ("value", C.c_int32), ("source", C.c_int32), ("min_index_gap", C.c_int32),
                ("n_keys", C.c_int32), ("max_per_node", C.c_int32), ("pad_", C.c_int32), ("max_range", C.c_double), ("max_distance", C.c_double)]

    def __repr__(self):
        return "ScParams(%s)" % ", ".join("%s=%r" % (f, getattr(self, f)) for f, _ in self._fields_ if f != "pad_")


class ScCandidate(C.Structure):
    _fields_ = [("sequence", C.c_int32), ("to", C.c_int32), ("from", C.c_int32), ("shift", C.c_int32), ("distance", C.c_double), ("yaw", C.c_double),
                ("key_distance", C.c_uint64)]


SC_CANDIDATE_DTYPE = np.dtype([("sequence", "i4"), ("to", "i4"), ("from", "i4"), ("shift", "i4"), ("distance", "f8"), ("yaw", "f8"), ("key_distance", "u8")])
assert SC_CANDIDATE_DTYPE.itemsize == C.sizeof(ScCandidate) == 40 and C.sizeof(ScParams) == 48
SC_MAX, SC_SUM, SC_COUNT = 0, 1, 2  # CFEAR_SC_MAX / CFEAR_SC_SUM / CFEAR_SC_COUNT
SC_MAX_RINGS, SC_MAX_SECTORS, SC_MAX_KEYS, SC_MAX_PER_NODE, SC_MAX_POINTS = 40, 120, 64, 16, 65536  # CFEAR_SC_MAX_*


def sc_params(**kw):
    """cfear_sc_default_params with fields replaced: n_rings (20), n_sectors (60), max_range (80 m), value (SC_MAX), source (0 = the filtered
    cloud, 1 = the peaks cloud; the log routes), min_index_gap (6), n_keys (10; 0 = exhaustive), max_per_node (1), max_distance (0.4)"""
    p = ScParams()
    lib().cfear_sc_default_params(C.byref(p))
    for k, v in kw.items():
        if k == "pad_" or not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def scan_context_layout(params=None, **kw):
    """cfear_scan_context_layout (host only, no device): the table the kernels read -> (ring_edge2 [n_rings + 1], sector_dir [n_sectors, 2])"""
    p = params if params is not None else sc_params(**kw)
    edge, sdir = np.zeros(max(int(p.n_rings), 0) + 1), np.zeros((max(int(p.n_sectors), 1), 2))
    rc = lib().cfear_scan_context_layout(C.byref(p), edge.ctypes.data, sdir.ctypes.data)
    if rc != 0:
        raise CfearError("cfear_scan_context_layout failed rc=%d (%r)" % (rc, p))
    return edge, sdir


KF_NODES, KF_CELLS = 1, 2  # CFEAR_KF_NODES / CFEAR_KF_CELLS
KF_CLOUD, KF_PEAKS = 4, 8  # CFEAR_KF_CLOUD / CFEAR_KF_PEAKS (cfear_odometry_set_keyframe_clouds)
STATUS_CELLS_LOST, STATUS_POINTS_LOST, STATUS_KEYFRAMES_DROPPED = 1, 2, 4  # the bits of a sequence's word in cfear_odometry_status


class Drift(C.Structure):
    """cfear_drift (include/cfear_hip.h): the KITTI drift of one trajectory with its per-length table (100 ... 800 m)"""
    _fields_ = [("translation_percent", C.c_double), ("rotation_deg_per_100m", C.c_double),
                ("translation_percent_by_length", C.c_double * 8), ("rotation_deg_per_100m_by_length", C.c_double * 8),
                ("segments", C.c_int32), ("segments_by_length", C.c_int32 * 8), ("reserved", C.c_int32)]


DRIFT_DTYPE = np.dtype([("translation_percent", "f8"), ("rotation_deg_per_100m", "f8"), ("translation_percent_by_length", "f8", 8),
                        ("rotation_deg_per_100m_by_length", "f8", 8), ("segments", "i4"), ("segments_by_length", "i4", 8), ("reserved", "i4")])
assert DRIFT_DTYPE.itemsize == C.sizeof(Drift) == 184

class CfarPlan(C.Structure):
    """cfear_cfar_plan (include/cfear_hip.h): the launch plan of the CA-CFAR detector"""
    _fields_ = [("kernel", C.c_int32), ("TB", C.c_int32), ("NW", C.c_int32), ("RS", C.c_int32), ("full", C.c_int32), ("sh", C.c_int32), ("kopen", C.c_int32),
                ("rmin", C.c_int32), ("rmax", C.c_int32), ("cr", C.c_int32 * 4), ("cq", C.c_int32 * 4), ("padl", C.c_int32), ("fill", C.c_int32),
                ("lds_bytes", C.c_int32), ("per_cu", C.c_int32), ("workgroups", C.c_int32)]


CFAR_KERNELS = ("owner", "fast16", "fast32", "general")  # CFEAR_CFAR_KERNEL_*

EXPORTS = [
    "cfear_version", "cfear_default_params", "cfear_create", "cfear_destroy", "cfear_last_error",
    "cfear_set_params", "cfear_synchronize", "cfear_tune", "cfear_kstrongest_launch_shape", "cfear_kstrongest_device", "cfear_kstrongest_host",
    "cfear_rotate_polar", "cfear_rotate_polar_device", "cfear_filter_polar", "cfear_filter_polar_device", "cfear_filter_cfar", "cfear_filter_cfar_device", "cfear_filter_cfar_batch_device", "cfear_filter_cfar_grid_device", "cfear_cfar_launch_plan", "cfear_cloud_upload", "cfear_cloud_size",
    "cfear_cloud_download", "cfear_clouds_download", "cfear_cloud_release", "cfear_compensate", "cfear_compensate_pair", "cfear_scan_create",
    "cfear_scan_from_cells", "cfear_scan_release", "cfear_scan_size", "cfear_scan_download_cells", "cfear_scan_closest",
    "cfear_register", "cfear_register_soft", "cfear_register_time_continuous", "cfear_get_cost", "cfear_cov_by_sampling", "cfear_odometry_create", "cfear_odometry_destroy", "cfear_odometry_reset",
    "cfear_odometry_step_device", "cfear_odometry_step_cloud_device", "cfear_odometry_step_host", "cfear_odometry_poses",
    "cfear_odometry_replay_host", "cfear_odometry_replay_device", "cfear_odometry_replay_host_cov", "cfear_odometry_replay_device_cov",
    "cfear_odometry_set_cov_sampling", "cfear_odometry_cov_samples", "cfear_host_alloc", "cfear_host_free",
    "cfear_surface_dims", "cfear_get_surface", "cfear_odometry_set_surface_recording", "cfear_odometry_surface",
    "cfear_odometry_set_sequence_params", "cfear_odometry_sequence_params", "cfear_odometry_set_sequence_sources",
    "cfear_default_fuser_options", "cfear_odometry_set_fuser_options", "cfear_odometry_fuser_options",
    "cfear_odometry_set_sequence_shapes", "cfear_odometry_sequence_shape",
    "cfear_odometry_set_sequence_detectors", "cfear_odometry_sequence_detector",
    "cfear_odometry_covariances", "cfear_odometry_status", "cfear_odometry_summary", "cfear_odometry_profile", "cfear_odometry_profile_read", "cfear_odometry_profile_read_stages", "cfear_odometry_phase_times", "cfear_time_kstrongest",
    "cfear_keyframe_constraint", "cfear_odometry_set_keyframe_recording", "cfear_odometry_keyframe_counts", "cfear_odometry_keyframe_nodes",
    "cfear_odometry_keyframe_cells", "cfear_odometry_keyframe_scans", "cfear_odometry_keyframe_edges",
    "cfear_odometry_set_keyframe_clouds", "cfear_odometry_keyframe_cloud_sizes", "cfear_odometry_keyframe_cloud", "cfear_odometry_keyframe_clouds",
    "cfear_pg_default_options", "cfear_pose_graph_optimize", "cfear_odometry_keyframe_optimize", "cfear_pose_graph_cost_host",
    "cfear_sc_default_params", "cfear_scan_context_layout", "cfear_scan_context_describe", "cfear_scan_context_match",
    "cfear_odometry_keyframe_descriptors", "cfear_odometry_keyframe_candidates",
    "cfear_drift_segments", "cfear_drift_plan_create", "cfear_drift_plan_release", "cfear_drift_device", "cfear_drift_host",
]


def lib_path():
    return _build.LIB


def lib():
    """Loads libcfear_hip.so; raises if it is not built (no fallback of any kind)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    try:  # PyTorch bundles its own HIP runtime: when both live in one process, torch's must be loaded first
        import torch  # noqa: F401
    except ImportError:
        pass
    path = lib_path()
    if not os.path.exists(path):
        raise CfearError("libcfear_hip.so is not built: run __graft_entry__.build() "
                         "(python -m cfear_radarodometry_code_public_amd.build)")
    L = C.CDLL(path)
    vp, u8p, u32p, f32p, f64p, i32p = (C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
    sig = {
        "cfear_version": (C.c_char_p, []),
        "cfear_default_params": (None, [C.POINTER(Params)]),
        "cfear_create": (C.c_int, [C.POINTER(vp), C.c_int, vp, C.POINTER(Params), C.c_int, C.c_int]),
        "cfear_destroy": (None, [vp]),
        "cfear_last_error": (C.c_char_p, [vp]),
        "cfear_set_params": (C.c_int, [vp, C.POINTER(Params)]),
        "cfear_synchronize": (C.c_int, [vp]),
        "cfear_tune": (C.c_int, [vp, C.c_int, C.c_int]),
        "cfear_kstrongest_launch_shape": (C.c_int, [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "cfear_kstrongest_device": (C.c_int, [vp, u8p, C.c_int, u32p]),
        "cfear_kstrongest_host": (C.c_int, [vp, u8p, C.c_int, u32p]),
        "cfear_rotate_polar": (C.c_int, [vp, u8p, C.c_int, C.c_int, u8p]),
        "cfear_rotate_polar_device": (C.c_int, [vp, u8p, C.c_int, C.c_int, C.c_int, u8p]),
        "cfear_filter_polar": (C.c_int, [vp, u8p, C.POINTER(vp), C.POINTER(vp)]),
        "cfear_filter_polar_device": (C.c_int, [vp, u8p, C.POINTER(vp), C.POINTER(vp)]),
        "cfear_filter_cfar": (C.c_int, [vp, u8p, C.c_int, C.c_int, C.c_float, C.c_double, C.POINTER(vp)]),
        "cfear_filter_cfar_device": (C.c_int, [vp, u8p, C.c_int, C.c_int, C.c_float, C.c_double, C.POINTER(vp)]),
        "cfear_filter_cfar_batch_device": (C.c_int, [vp, u8p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_double, f32p, C.c_int, i32p]),
        "cfear_filter_cfar_grid_device": (C.c_int, [vp, u8p, C.c_int, vp, i32p, C.c_int, C.c_double, f32p, C.c_int, i32p]),
        "cfear_cfar_launch_plan": (C.c_int, [vp, C.c_int, C.c_int, C.c_float, C.c_int, C.POINTER(CfarPlan)]),
        "cfear_cloud_upload": (C.c_int, [vp, f32p, C.c_int, C.POINTER(vp)]),
        "cfear_cloud_size": (C.c_int, [vp, vp, C.POINTER(C.c_int)]),
        "cfear_cloud_download": (C.c_int, [vp, vp, f32p, C.c_int, C.POINTER(C.c_int)]),
        "cfear_clouds_download": (C.c_int, [vp, C.POINTER(vp), C.c_int, C.POINTER(vp), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "cfear_cloud_release": (None, [vp, vp]),
        "cfear_compensate": (C.c_int, [vp, vp, f64p, C.c_int]),
        "cfear_compensate_pair": (C.c_int, [vp, vp, vp, f64p, C.c_int]),
        "cfear_scan_create": (C.c_int, [vp, vp, C.POINTER(vp)]),
        "cfear_scan_from_cells": (C.c_int, [vp, vp, C.c_int, C.POINTER(vp)]),
        "cfear_scan_release": (None, [vp, vp]),
        "cfear_scan_size": (C.c_int, [vp, vp, C.POINTER(C.c_int)]),
        "cfear_scan_download_cells": (C.c_int, [vp, vp, vp, C.c_int, C.POINTER(C.c_int)]),
        "cfear_scan_closest": (C.c_int, [vp, vp, f64p, C.c_int, C.c_double, i32p]),
        "cfear_register": (C.c_int, [vp, C.POINTER(vp), C.c_int, f64p, f64p, C.POINTER(RegSummary)]),
        "cfear_register_soft": (C.c_int, [vp, C.POINTER(vp), C.c_int, f64p, f64p, f64p, C.POINTER(RegSummary)]),
        "cfear_register_time_continuous": (C.c_int, [vp, C.POINTER(vp), C.c_int, f64p, f64p, C.c_int, f64p, f64p, C.POINTER(RegSummary)]),
        "cfear_get_cost": (C.c_int, [vp, C.POINTER(vp), C.c_int, f64p, C.c_int, f64p, f64p, C.c_int, C.POINTER(C.c_int)]),
        "cfear_cov_by_sampling": (C.c_int, [vp, C.POINTER(vp), C.c_int, f64p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double,
                                            C.c_double, C.c_int, f64p, C.POINTER(C.c_int), f64p]),
        "cfear_odometry_create": (C.c_int, [vp, C.c_int, C.POINTER(vp)]),
        "cfear_odometry_destroy": (None, [vp, vp]),
        "cfear_odometry_reset": (C.c_int, [vp, vp]),
        "cfear_odometry_step_device": (C.c_int, [vp, vp, u8p]),
        "cfear_odometry_step_host": (C.c_int, [vp, vp, u8p]),
        "cfear_odometry_step_cloud_device": (C.c_int, [vp, vp, f32p, C.c_int, i32p]),
        "cfear_odometry_poses": (C.c_int, [vp, vp, f64p]),
        "cfear_odometry_covariances": (C.c_int, [vp, vp, f64p]),
        "cfear_odometry_status": (C.c_int, [vp, vp, i32p]),
        "cfear_odometry_replay_host": (C.c_int, [vp, vp, u8p, C.c_int, vp]),
        "cfear_odometry_replay_device": (C.c_int, [vp, vp, u8p, C.c_int, vp]),
        "cfear_odometry_replay_host_cov": (C.c_int, [vp, vp, u8p, C.c_int, vp, vp]),
        "cfear_odometry_replay_device_cov": (C.c_int, [vp, vp, u8p, C.c_int, vp, vp]),
        "cfear_odometry_set_cov_sampling": (C.c_int, [vp, vp, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double]),
        "cfear_odometry_cov_samples": (C.c_int, [vp, vp, C.c_int, f64p, vp]),
        "cfear_surface_dims": (C.c_int, [C.c_double, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "cfear_get_surface": (C.c_int, [vp, C.POINTER(vp), C.c_int, f64p, f64p, C.c_int, C.c_double, C.c_int, f64p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "cfear_odometry_set_surface_recording": (C.c_int, [vp, vp, C.c_int]),
        "cfear_odometry_surface": (C.c_int, [vp, vp, C.c_double, C.c_int, vp, vp, vp, vp]),
        "cfear_odometry_set_sequence_params": (C.c_int, [vp, vp, vp, C.c_int]),
        "cfear_odometry_sequence_params": (C.c_int, [vp, vp, C.c_int, C.POINTER(Params)]),
        "cfear_odometry_set_sequence_sources": (C.c_int, [vp, vp, i32p, C.c_int, C.c_int]),
        "cfear_odometry_set_sequence_shapes": (C.c_int, [vp, vp, vp, C.c_int]),
        "cfear_odometry_sequence_shape": (C.c_int, [vp, vp, C.c_int, C.POINTER(SeqShape)]),
        "cfear_odometry_set_sequence_detectors": (C.c_int, [vp, vp, vp, C.c_int, i32p, C.c_int]),
        "cfear_odometry_sequence_detector": (C.c_int, [vp, vp, C.c_int, C.POINTER(SeqDetector)]),
        "cfear_default_fuser_options": (None, [C.POINTER(FuserOptions)]),
        "cfear_odometry_set_fuser_options": (C.c_int, [vp, vp, vp, C.c_int]),
        "cfear_odometry_fuser_options": (C.c_int, [vp, vp, C.c_int, C.POINTER(FuserOptions)]),
        "cfear_host_alloc": (C.c_int, [vp, C.c_size_t, C.POINTER(vp)]),
        "cfear_host_free": (None, [vp, vp]),
        "cfear_odometry_summary": (C.c_int, [vp, vp, C.c_int, C.POINTER(RegSummary), C.POINTER(C.c_int),
                                             C.POINTER(C.c_int)]),
        "cfear_odometry_profile": (C.c_int, [vp, vp, C.c_int]),
        "cfear_odometry_profile_read": (C.c_int, [vp, vp, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
        "cfear_odometry_profile_read_stages": (C.c_int, [vp, vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]),
        "cfear_odometry_phase_times": (C.c_int, [vp, vp, C.c_int, vp]),
        "cfear_time_kstrongest": (C.c_int, [vp, u8p, C.c_int, u32p, C.c_int, C.c_int, C.POINTER(C.c_double)]),
        "cfear_keyframe_constraint": (C.c_int, [f64p, f64p, f64p, f64p, f64p]),
        "cfear_odometry_set_keyframe_recording": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int]),
        "cfear_odometry_keyframe_counts": (C.c_int, [vp, vp, i32p, i32p]),
        "cfear_odometry_keyframe_nodes": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, C.c_int, C.POINTER(C.c_int)]),
        "cfear_odometry_keyframe_cells": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, C.c_int, C.POINTER(C.c_int)]),
        "cfear_odometry_keyframe_scans": (C.c_int, [vp, vp, C.c_int, i32p, C.c_int, C.POINTER(vp)]),
        "cfear_odometry_keyframe_edges": (C.c_int, [vp, vp, vp, C.c_int, vp, f64p, vp]),
        "cfear_odometry_set_keyframe_clouds": (C.c_int, [vp, vp, C.c_int, C.c_int]),
        "cfear_odometry_keyframe_cloud_sizes": (C.c_int, [vp, vp, C.c_int, C.c_int, i32p, i32p, C.c_int, C.POINTER(C.c_int)]),
        "cfear_odometry_keyframe_cloud": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, f32p, C.c_int, C.POINTER(C.c_int)]),
        "cfear_odometry_keyframe_clouds": (C.c_int, [vp, vp, C.c_int, i32p, C.c_int, C.c_int, C.POINTER(vp)]),
        "cfear_pg_default_options": (None, [C.POINTER(PgOptions)]),
        "cfear_pose_graph_optimize": (C.c_int, [vp, C.c_int, i32p, i32p, vp, i32p, C.POINTER(PgOptions), f64p, vp]),
        "cfear_odometry_keyframe_optimize": (C.c_int, [vp, vp, vp, C.c_int, C.POINTER(PgOptions), f64p, C.c_int, i32p, vp]),
        "cfear_pose_graph_cost_host": (C.c_int, [f64p, C.c_int, vp, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
        "cfear_sc_default_params": (None, [C.POINTER(ScParams)]),
        "cfear_scan_context_layout": (C.c_int, [C.POINTER(ScParams), f64p, f64p]),
        "cfear_scan_context_describe": (C.c_int, [vp, C.POINTER(ScParams), f32p, i32p, C.c_int, u32p, u32p, i32p]),
        "cfear_scan_context_match": (C.c_int, [vp, C.POINTER(ScParams), C.c_int, i32p, u32p, vp, C.c_int, C.POINTER(C.c_int)]),
        "cfear_odometry_keyframe_descriptors": (C.c_int, [vp, vp, C.POINTER(ScParams), C.c_int, C.c_int, u32p, u32p, C.c_int, C.POINTER(C.c_int)]),
        "cfear_odometry_keyframe_candidates": (C.c_int, [vp, vp, C.POINTER(ScParams), vp, C.c_int, C.POINTER(C.c_int)]),
        "cfear_drift_segments": (C.c_int, [f64p, C.c_int, i32p, i32p, i32p, C.c_int, C.POINTER(C.c_int)]),
        "cfear_drift_plan_create": (C.c_int, [vp, f64p, C.c_int, C.POINTER(vp)]),
        "cfear_drift_plan_release": (None, [vp, vp]),
        "cfear_drift_device": (C.c_int, [vp, vp, vp, C.c_size_t, C.c_size_t, C.c_int, C.c_int, vp]),
        "cfear_drift_host": (C.c_int, [vp, vp, vp, C.c_size_t, C.c_size_t, C.c_int, C.c_int, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)  # AttributeError if the ABI is incomplete (tests/test_abi.py checks every export)
        fn.restype = res
        fn.argtypes = args
    _LIB = L
    return L


def surface_dims(res, width, x0=0.0, y0=0.0):
    """cfear_surface_dims (host only, no device): the GetSurface grid (n_scan_normal.cpp:46-63) -> (pixels, values visited along x,
    values visited along y). Raises CfearError for an invalid (rc -1) or too large (rc -3) grid."""
    p, nx, ny = C.c_int(), C.c_int(), C.c_int()
    rc = lib().cfear_surface_dims(float(res), int(width), float(x0), float(y0), C.byref(p), C.byref(nx), C.byref(ny))
    if rc != 0:
        raise CfearError("cfear_surface_dims failed rc=%d" % rc)
    return p.value, nx.value, ny.value


def keyframe_constraint(from_xyt, to_xyt, cov6):
    """cfear_keyframe_constraint (host only, no device): AddToGraph's odometry constraint (odometrykeyframefuser.cpp:435-440) from the
    new keyframe's pose, the previous one's and cov_current [6, 6] -> (t_be (x, y, theta), information [6, 6]). Raises CfearError for a
    non-finite input or a singular covariance."""
    f = np.ascontiguousarray(from_xyt, dtype=np.float64).reshape(3)
    t = np.ascontiguousarray(to_xyt, dtype=np.float64).reshape(3)
    c = np.ascontiguousarray(cov6, dtype=np.float64).reshape(36)
    tbe, info = np.zeros(3), np.zeros(36)
    rc = lib().cfear_keyframe_constraint(f.ctypes.data, t.ctypes.data, c.ctypes.data, tbe.ctypes.data, info.ctypes.data)
    if rc != 0:
        raise CfearError("cfear_keyframe_constraint failed rc=%d" % rc)
    return tbe, info.reshape(6, 6)


def _gt34(gt):
    """ground-truth poses [n, 4, 4] or [n, 3, 4] (or [n, 12]) -> contiguous [n, 12] doubles, the 3x4 row-major form of a KITTI line"""
    g = np.asarray(gt, dtype=np.float64)
    g = g.reshape(len(g), -1, 4)[:, :3, :] if g.ndim == 3 else g.reshape(len(g), 3, 4)
    return np.ascontiguousarray(g).reshape(len(g), 12)


def drift_segments(gt):
    """cfear_drift_segments (host only, no device): the (first, last, length index) triples of the KITTI drift metric for the ground
    truth gt, in the metric's order -> int32 array [m, 3] (kitti.segments is the numpy statement)"""
    g = _gt34(gt)
    m = C.c_int()
    rc = lib().cfear_drift_segments(g.ctypes.data, len(g), None, None, None, 0, C.byref(m))
    if rc not in (0, -6):  # (CFEAR_ERR_CAPACITY with the count is the answer to capacity 0)
        raise CfearError("cfear_drift_segments failed rc=%d" % rc)
    out = np.zeros((3, max(m.value, 1)), dtype=np.int32)
    rc = lib().cfear_drift_segments(g.ctypes.data, len(g), out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, m.value, C.byref(m))
    if rc != 0:
        raise CfearError("cfear_drift_segments failed rc=%d" % rc)
    return np.ascontiguousarray(out[:, :m.value].T)


def default_params(**kw):
    p = Params()
    lib().cfear_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def default_fuser_options(**kw):
    o = FuserOptions()
    lib().cfear_default_fuser_options(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def _addr(a):
    """Device pointer (int), torch tensor (data_ptr) or numpy array -> address."""
    if isinstance(a, int):
        return a
    if hasattr(a, "data_ptr"):
        return a.data_ptr()
    return a.ctypes.data


TUNE_FILTER_OCCUPANCY, TUNE_FILTER_ROWS_PER_WAVE, TUNE_ODOMETRY_OVERLAP, TUNE_REPLAY_PERSISTENT_MAX, TUNE_FILTER_CUS, TUNE_REPEAT_SHORTCUT, TUNE_MAX_CELLS, TUNE_REGISTRATION_ORDER, TUNE_LARGE_SUBMAP_KERNEL, TUNE_NN_TIE_RULE, TUNE_VOXEL_ORDER, TUNE_FILTER_PEAKS = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12
TUNE_DEFAULTS = {TUNE_ODOMETRY_OVERLAP: 0, TUNE_FILTER_CUS: 0, TUNE_MAX_CELLS: 0, TUNE_REGISTRATION_ORDER: 1, TUNE_LARGE_SUBMAP_KERNEL: 0}  # include/cfear_hip.h


class Context:
    """cfear_ctx: one HIP device + stream. `stream` = raw hipStream_t handle (int) or None."""

    def __init__(self, params, A, R, device=0, stream=None):
        self._L = lib()
        self._h = C.c_void_p()
        self.params = params
        self.A, self.R = int(A), int(R)
        self.device = int(device)
        self._tuned = {}
        rc = self._L.cfear_create(C.byref(self._h), int(device), C.c_void_p(stream or 0), C.byref(params),
                                  self.A, self.R)
        if rc != 0:
            self._h = None
            raise CfearError("cfear_create failed rc=%d (is a gfx950 GPU visible?)" % rc)

    def close(self):
        if getattr(self, "_h", None):
            for ptr in list(getattr(self, "_pinned", {}).values()):
                self._L.cfear_host_free(self._h, ptr)
            self._pinned = {}
            self._L.cfear_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise CfearError("%s failed rc=%d: %s" % (what, rc, self._L.cfear_last_error(self._h).decode()))

    @property
    def handle(self):
        return self._h

    def set_params(self, params):
        self._check(self._L.cfear_set_params(self._h, C.byref(params)), "cfear_set_params")
        self.params = params

    def synchronize(self):
        self._check(self._L.cfear_synchronize(self._h), "cfear_synchronize")

    def tune(self, key, value):
        """cfear_tune (include/cfear_hip.h): launch-shape knobs - TUNE_FILTER_OCCUPANCY, TUNE_FILTER_ROWS_PER_WAVE, TUNE_ODOMETRY_OVERLAP,
        TUNE_FILTER_CUS, TUNE_REPLAY_PERSISTENT_MAX, TUNE_REPEAT_SHORTCUT, TUNE_REGISTRATION_ORDER: results do not depend on them -,
        TUNE_FILTER_PEAKS (-1 automatic, 1 / 0: the filter always / never computes the slots' peak flag, bit 25) and
        TUNE_MAX_CELLS, the cell capacity batched odometry objects created afterwards are sized for (an overflow is reported, never silent)"""
        self._check(self._L.cfear_tune(self._h, int(key), int(value)), "cfear_tune")
        # what the library holds after its clamps (csrc/cabi.hip cfear_tune), so that a later restore puts back a value the context really had
        k, v = int(key), int(value)
        clamp = {TUNE_FILTER_ROWS_PER_WAVE: lambda x: max(x, 0), TUNE_ODOMETRY_OVERLAP: lambda x: min(max(x, 0), 8), TUNE_FILTER_CUS: lambda x: max(x, 0),
                 TUNE_REGISTRATION_ORDER: lambda x: int(x != 0), TUNE_MAX_CELLS: lambda x: max(x, 0), TUNE_REPEAT_SHORTCUT: lambda x: int(x != 0),
                 TUNE_VOXEL_ORDER: lambda x: int(x == 1), TUNE_NN_TIE_RULE: lambda x: x if 0 <= x <= 2 else 0, TUNE_LARGE_SUBMAP_KERNEL: lambda x: x if 0 <= x <= 2 else 0,
                 TUNE_REPLAY_PERSISTENT_MAX: lambda x: max(x, 0), TUNE_FILTER_PEAKS: lambda x: -1 if x < 0 else int(x != 0)}
        self._tuned[k] = clamp.get(k, lambda x: x)(v)

    # ---- stage 1 ----
    def kstrongest_launch_shape(self, n_scans):
        """cfear_kstrongest_launch_shape: (rows_per_wave, workgroups, occupancy) of the filter launch for n_scans images under the current knobs"""
        rows, wgs, occ = C.c_int(), C.c_int(), C.c_int()
        self._check(self._L.cfear_kstrongest_launch_shape(self._h, int(n_scans), C.byref(rows), C.byref(wgs), C.byref(occ)), "cfear_kstrongest_launch_shape")
        return rows.value, wgs.value, occ.value

    def kstrongest_host(self, polar):
        polar = np.ascontiguousarray(polar, dtype=np.uint8)
        if polar.ndim == 2:
            polar = polar[None]
        n, A, R = polar.shape
        assert (A, R) == (self.A, self.R)
        out = np.zeros((n, A, self.params.k_strongest), dtype=np.uint32)
        self._check(self._L.cfear_kstrongest_host(self._h, polar.ctypes.data, n, out.ctypes.data), "cfear_kstrongest_host")
        return out

    def kstrongest_device(self, d_polar, n_scans, d_slots):
        self._check(self._L.cfear_kstrongest_device(self._h, _addr(d_polar), int(n_scans), _addr(d_slots)),
                    "cfear_kstrongest_device")

    def time_kstrongest(self, d_polar, n_scans, d_slots, warmup, iters):
        t = C.c_double()
        self._check(self._L.cfear_time_kstrongest(self._h, _addr(d_polar), int(n_scans), _addr(d_slots), int(warmup),
                                                  int(iters), C.byref(t)), "cfear_time_kstrongest")
        return t.value

    def rotate_polar(self, img):
        """radarDriver::Callback (non-Oxford): rows = range -> rows = azimuth (cv::ROTATE_90_COUNTERCLOCKWISE)"""
        img = np.ascontiguousarray(img, dtype=np.uint8)
        out = np.empty((img.shape[1], img.shape[0]), dtype=np.uint8)
        self._check(self._L.cfear_rotate_polar(self._h, img.ctypes.data, img.shape[0], img.shape[1], out.ctypes.data), "cfear_rotate_polar")
        return out

    # ---- stage 1 -> clouds (radarDriver::CallbackOffline) ----
    def filter_polar(self, polar, peaks=True):
        """polar: uint8 [A,R] numpy (host) or a device pointer/torch tensor (device=True path via _addr)."""
        c, cp = C.c_void_p(), C.c_void_p()
        if isinstance(polar, np.ndarray):
            polar = np.ascontiguousarray(polar, dtype=np.uint8)
            assert polar.shape == (self.A, self.R)
            rc = self._L.cfear_filter_polar(self._h, polar.ctypes.data, C.byref(c), C.byref(cp) if peaks else None)
        else:
            rc = self._L.cfear_filter_polar_device(self._h, _addr(polar), C.byref(c), C.byref(cp) if peaks else None)
        self._check(rc, "cfear_filter_polar")
        return Cloud(self, c), (Cloud(self, cp) if peaks else None)

    def filter_cfar(self, polar, window_size=10, nb_guard_cells=20, false_alarm_rate=0.01, max_distance=400.0):
        """radarDriver::Process with filter_type CA-CFAR (defaults of radarDriver::Parameters, radar_driver.h:43-44)."""
        c = C.c_void_p()
        args = (int(window_size), int(nb_guard_cells), C.c_float(false_alarm_rate), C.c_double(max_distance), C.byref(c))
        if isinstance(polar, np.ndarray):
            polar = np.ascontiguousarray(polar, dtype=np.uint8)
            assert polar.shape == (self.A, self.R)
            rc = self._L.cfear_filter_cfar(self._h, polar.ctypes.data, *args)
        else:
            rc = self._L.cfear_filter_cfar_device(self._h, _addr(polar), *args)
        self._check(rc, "cfear_filter_cfar")
        return Cloud(self, c)

    def cfar_launch_plan(self, window_size=10, nb_guard_cells=20, false_alarm_rate=0.01, n_scans=1):
        """cfear_cfar_launch_plan: the detector launch for n_scans images of this context as a dict - kernel (a CFAR_KERNELS name), TB, NW, RS, full, sh,
        kopen, rmin, rmax, cr, cq, padl, fill, lds_bytes, per_cu, workgroups (csrc/cfar_shape.h; host/cfar_shape_check prints the same without a GPU)"""
        p = CfarPlan()
        self._check(self._L.cfear_cfar_launch_plan(self._h, int(window_size), int(nb_guard_cells), C.c_float(false_alarm_rate), int(n_scans), C.byref(p)),
                    "cfear_cfar_launch_plan")
        d = {f: getattr(p, f) for f, _ in CfarPlan._fields_}
        d.update(kernel=CFAR_KERNELS[p.kernel], cr=tuple(p.cr), cq=tuple(p.cq))
        return d

    def filter_cfar_grid(self, d_polar, n_sources, dets, source, d_xyi, capacity, d_counts, max_distance=400.0):
        """Several CA-CFAR detectors over shared device-resident images in one pass (cfear_filter_cfar_grid_device): cloud c is the
        detections of image source[c] (None: image c) under dets[c] (SeqDetector or (window, guard, rate, z_min) tuples) -> d_xyi
        [len(dets), capacity, 3] float32, d_counts [len(dets)] int32 on the device. Asynchronous on the context stream."""
        arr = detector_array(dets)
        src = None if source is None else np.ascontiguousarray(source, dtype=np.int32)
        if src is not None and src.size != len(arr):
            raise ValueError("filter_cfar_grid: %d detectors, %d sources" % (len(arr), src.size))
        self._check(self._L.cfear_filter_cfar_grid_device(self._h, _addr(d_polar), int(n_sources), C.cast(arr, C.c_void_p), src.ctypes.data if src is not None else None,
                                                          len(arr), float(max_distance), _addr(d_xyi), int(capacity), _addr(d_counts)),
                    "cfear_filter_cfar_grid_device")

    def filter_cfar_batch(self, d_polar, n_scans, d_xyi, capacity, d_counts, window_size=10, nb_guard_cells=20, false_alarm_rate=0.01, max_distance=400.0):
        """CA-CFAR over n_scans device-resident sweeps; d_xyi [n_scans, capacity, 3] float32 and d_counts [n_scans] int32 on the device"""
        self._check(self._L.cfear_filter_cfar_batch_device(self._h, _addr(d_polar), int(n_scans), int(window_size), int(nb_guard_cells),
                                                           C.c_float(false_alarm_rate), C.c_double(max_distance), _addr(d_xyi), int(capacity),
                                                           _addr(d_counts)), "cfear_filter_cfar_batch_device")

    def cloud_upload(self, xyi):
        xyi = np.ascontiguousarray(xyi, dtype=np.float32).reshape(-1, 3)
        c = C.c_void_p()
        self._check(self._L.cfear_cloud_upload(self._h, xyi.ctypes.data, xyi.shape[0], C.byref(c)), "cfear_cloud_upload")
        return Cloud(self, c)

    def compensate(self, cloud, motion_xyt, ccw):
        m = np.asarray(motion_xyt, dtype=np.float64).copy()
        self._check(self._L.cfear_compensate(self._h, cloud._h, m.ctypes.data, int(ccw)), "cfear_compensate")

    def compensate_pair(self, cloud, cloud_peaks, motion_xyt, ccw):
        """cfear_compensate_pair: a sweep's two clouds by the same motion in one launch (odometrykeyframefuser.cpp:148-149)"""
        m = np.asarray(motion_xyt, dtype=np.float64).copy()
        self._check(self._L.cfear_compensate_pair(self._h, cloud._h, cloud_peaks._h, m.ctypes.data, int(ccw)), "cfear_compensate_pair")

    # ---- stage 2 (MapPointNormal) ----
    def scan_create(self, cloud):
        s = C.c_void_p()
        self._check(self._L.cfear_scan_create(self._h, cloud._h, C.byref(s)), "cfear_scan_create")
        return Scan(self, s)

    def scan_from_cells(self, cells):
        """cells: numpy array of CELL_DTYPE (raw = true identity cells, transformed copies) -> Scan"""
        cells = np.ascontiguousarray(cells, dtype=CELL_DTYPE)
        s = C.c_void_p()
        self._check(self._L.cfear_scan_from_cells(self._h, cells.ctypes.data, len(cells), C.byref(s)), "cfear_scan_from_cells")
        return Scan(self, s)

    # ---- stage 3 (n_scan_normal_reg::Register) ----
    def register(self, scans, poses):
        n = len(scans)
        arr = (C.c_void_p * n)(*[s._h for s in scans])
        P = np.ascontiguousarray(poses, dtype=np.float64).reshape(n, 3).copy()
        cov = np.zeros(36)
        S = RegSummary()
        self._check(self._L.cfear_register(self._h, arr, n, P.ctypes.data, cov.ctypes.data, C.byref(S)), "cfear_register")
        return bool(S.success), P, cov.reshape(6, 6), S

    def register_soft(self, scans, poses, prior_cov6):
        """Register(..., soft_constraints=true) with reg_cov.back() = prior_cov6"""
        n = len(scans)
        arr = (C.c_void_p * n)(*[s._h for s in scans])
        P = np.ascontiguousarray(poses, dtype=np.float64).reshape(n, 3).copy()
        pc = np.ascontiguousarray(prior_cov6, dtype=np.float64).reshape(36).copy()
        cov = np.zeros(36)
        S = RegSummary()
        self._check(self._L.cfear_register_soft(self._h, arr, n, P.ctypes.data, pc.ctypes.data, cov.ctypes.data, C.byref(S)), "cfear_register_soft")
        return bool(S.success), P, cov.reshape(6, 6), S

    def register_time_continuous(self, scans, poses, velocity, ccw=False, prior_cov6=None):
        """RegisterTimeContinuous(scans, Tsrc, reg_cov, Tvel, soft_constraints, ccw) (n_scan_normal.cpp:67-80): the last scan keeps its
        motion distortion; velocity = (vx, vy, vtheta) over one sweep = Affine3dToVectorXYeZ(Tvel); prior_cov6: reg_cov.back() with
        soft_constraints, None: without. Returns what register returns."""
        n = len(scans)
        arr = (C.c_void_p * n)(*[s._h for s in scans])
        P = np.ascontiguousarray(poses, dtype=np.float64).reshape(n, 3).copy()
        v = np.ascontiguousarray(velocity, dtype=np.float64).reshape(3).copy()
        pc = None if prior_cov6 is None else np.ascontiguousarray(prior_cov6, dtype=np.float64).reshape(36).copy()
        cov = np.zeros(36)
        S = RegSummary()
        self._check(self._L.cfear_register_time_continuous(self._h, arr, n, P.ctypes.data, v.ctypes.data, int(bool(ccw)), None if pc is None else pc.ctypes.data,
                                                           cov.ctypes.data, C.byref(S)), "cfear_register_time_continuous")
        return bool(S.success), P, cov.reshape(6, 6), S

    def get_cost(self, scans, poses, itr=2):
        """n_scan_normal_reg::GetCost -> (score, residuals) or None where the reference returns false."""
        n = len(scans)
        arr = (C.c_void_p * n)(*[s._h for s in scans])
        P = np.ascontiguousarray(poses, dtype=np.float64).reshape(n, 3).copy()
        cap = 2 * (n - 1) * max(scans[-1].size, 1)
        res = np.zeros(cap)
        score, m = C.c_double(), C.c_int()
        rc = self._L.cfear_get_cost(self._h, arr, n, P.ctypes.data, int(itr), C.byref(score), res.ctypes.data, cap, C.byref(m))
        if rc == -4:  # CFEAR_ERR_EMPTY
            return None
        self._check(rc, "cfear_get_cost")
        return score.value, res[:m.value].copy()

    def get_surface(self, scans, poses, res, width, itr=2, prior_cov6=None):
        """n_scan_normal_reg::GetSurface (n_scan_normal.cpp:29-65) -> (pixels, pixels) array, row i = x, column j = y; NaN in the
        cells the reference's loops never reach. prior_cov6: reg_cov.back() with soft_constraints, None: without."""
        n = len(scans)
        arr = (C.c_void_p * n)(*[s._h for s in scans])
        P = np.ascontiguousarray(poses, dtype=np.float64).reshape(n, 3).copy()
        pixels = surface_dims(res, width, P[-1, 0], P[-1, 1])[0]
        out = np.empty((pixels, pixels))
        pc = None if prior_cov6 is None else np.ascontiguousarray(prior_cov6, dtype=np.float64).reshape(36).copy()
        nx, ny = C.c_int(), C.c_int()
        self._check(self._L.cfear_get_surface(self._h, arr, n, P.ctypes.data, None if pc is None else pc.ctypes.data, int(itr), float(res),
                                              int(width), out.ctypes.data, C.byref(nx), C.byref(ny)), "cfear_get_surface")
        return out

    def cov_by_sampling(self, scans, poses, final_cost, num_residuals, itr=2, xy_range=0.4, yaw_range=0.0043625, steps=3, cov_scaler=4.0):
        """approximateCovarianceBySampling -> (success, cov6x6, sampled costs)"""
        n = len(scans)
        arr = (C.c_void_p * n)(*[s._h for s in scans])
        P = np.ascontiguousarray(poses, dtype=np.float64).reshape(n, 3).copy()
        cov, costs, ok = np.zeros(36), np.zeros(steps ** 3), C.c_int()
        self._check(self._L.cfear_cov_by_sampling(self._h, arr, n, P.ctypes.data, int(itr), float(xy_range), float(yaw_range), int(steps),
                                                  float(cov_scaler), float(final_cost), int(num_residuals), cov.ctypes.data, C.byref(ok),
                                                  costs.ctypes.data), "cfear_cov_by_sampling")
        return bool(ok.value), cov.reshape(6, 6), costs

    def pinned(self, shape, dtype=np.uint8):
        """Page-locked host array (cfear_host_alloc): copies from it overlap with kernels. Freed by pinned_free(arr) - arr or any
        view / slice of it - or when the context closes: the array and its views must not be touched after either (the memory is
        gone; NumPy cannot know)."""
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        ptr = C.c_void_p()
        self._check(self._L.cfear_host_alloc(self._h, nbytes, C.byref(ptr)), "cfear_host_alloc")
        buf = (C.c_uint8 * nbytes).from_address(ptr.value)
        arr = np.frombuffer(buf, dtype=dtype).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = ptr.value
        return arr

    def pinned_free(self, arr):
        root = arr
        while isinstance(getattr(root, "base", None), np.ndarray):  # a view / slice: the allocation is its root array's
            root = root.base
        ptr = getattr(self, "_pinned", {}).pop(root.ctypes.data, None)
        if ptr is None:
            raise ValueError("pinned_free: not an array of Context.pinned() of this context (or already freed)")
        if self._h:
            self._L.cfear_host_free(self._h, ptr)

    def drift_plan(self, gt):
        """cfear_drift_plan_create: the segments of the ground truth gt ([n, 4, 4] poses) and what the KITTI drift needs of them, on the
        device -> DriftPlan (score() evaluates batches of trajectories against it)"""
        g = _gt34(gt)
        h = C.c_void_p()
        self._check(self._L.cfear_drift_plan_create(self._h, g.ctypes.data, len(g), C.byref(h)), "cfear_drift_plan_create")
        return DriftPlan(self, h, len(g))

    def pose_graph_optimize(self, poses, edges, fixed=None, options=None, **kw):
        """cfear_pose_graph_optimize: many planar pose graphs in one launch. poses: a list of [n_g, 3] arrays (x, y, theta), one per graph, or one
        such array (a single graph); edges: per graph an array of PG_EDGE_DTYPE (posegraph.problem builds them); fixed: per graph the node
        that is held (None: node 0); options: a PgOptions, or its fields as keywords (pg_options). -> (optimised poses in the shape given,
        summaries: PG_SUMMARY_DTYPE [graphs]). The input arrays are not changed."""
        single = isinstance(poses, np.ndarray) and poses.ndim == 2
        P = [poses] if single else list(poses)
        E = [edges] if single else list(edges)
        if len(P) != len(E) or not P:
            raise CfearError("pose_graph_optimize: %d pose arrays, %d edge arrays" % (len(P), len(E)))
        P = [np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 3) for p in P]
        E = [np.ascontiguousarray(e, dtype=PG_EDGE_DTYPE).reshape(-1) for e in E]
        noff = np.concatenate([[0], np.cumsum([len(p) for p in P])]).astype(np.int32)
        eoff = np.concatenate([[0], np.cumsum([len(e) for e in E])]).astype(np.int32)
        x = np.ascontiguousarray(np.concatenate(P, axis=0))
        ed = np.ascontiguousarray(np.concatenate(E))
        fx = None
        if fixed is not None:
            fx = np.ascontiguousarray(np.atleast_1d(fixed), dtype=np.int32)
            if len(fx) != len(P):
                raise CfearError("pose_graph_optimize: %d fixed nodes for %d graphs" % (len(fx), len(P)))
        opt = options if options is not None else pg_options(**kw)
        sums = np.zeros(len(P), dtype=PG_SUMMARY_DTYPE)
        self._check(self._L.cfear_pose_graph_optimize(self._h, len(P), noff.ctypes.data, eoff.ctypes.data, ed.ctypes.data if len(ed) else None,
                                                      fx.ctypes.data if fx is not None else None, C.byref(opt), x.ctypes.data if len(x) else None,
                                                      sums.ctypes.data), "cfear_pose_graph_optimize")
        out = [x[noff[g]:noff[g + 1]].copy() for g in range(len(P))]
        return (out[0] if single else out), sums

    def scan_context(self, clouds, params=None, **kw):
        """cfear_scan_context_describe: the Scan-Context descriptors of host clouds, a workgroup each in one launch. clouds: a list of [n, 3]
        arrays (x, y, intensity; a cloud may be empty) or one such array; params: a ScParams, or its fields as keywords (sc_params).
        -> (bins uint32 [clouds, n_sectors, n_rings], ring_sums uint32 [clouds, n_rings], dropped int32 [clouds]: the points with a field
        that is not finite); for a single array the three without the leading axis."""
        single = isinstance(clouds, np.ndarray) and clouds.ndim == 2
        cl = [np.ascontiguousarray(c, dtype=np.float32).reshape(-1, 3) for c in ([clouds] if single else list(clouds))]
        p = params if params is not None else sc_params(**kw)
        off = np.concatenate([[0], np.cumsum([len(c) for c in cl])]).astype(np.int32)
        xyi = np.ascontiguousarray(np.concatenate(cl, axis=0)) if cl else np.zeros((0, 3), dtype=np.float32)
        m = len(cl)
        bins = np.zeros((m, max(int(p.n_sectors), 1), max(int(p.n_rings), 1)), dtype=np.uint32)
        ring = np.zeros((m, max(int(p.n_rings), 1)), dtype=np.uint32)
        drop = np.zeros(m, dtype=np.int32)
        self._check(self._L.cfear_scan_context_describe(self._h, C.byref(p), xyi.ctypes.data if len(xyi) else None, off.ctypes.data, m,
                                                        bins.ctypes.data if m else None, ring.ctypes.data if m else None, drop.ctypes.data if m else None),
                    "cfear_scan_context_describe")
        return (bins[0], ring[0], drop[0]) if single else (bins, ring, drop)

    def scan_context_match(self, descriptor_sets, params=None, **kw):
        """cfear_scan_context_match: the loop candidates of sets of descriptors, all sets in one launch. descriptor_sets: a list of uint32
        [n_g, n_sectors, n_rings] arrays (scan_context's bins), one per set, or one such array (a single set). -> SC_CANDIDATE_DTYPE, (set,
        to, distance) ascending; `sequence` is the set."""
        single = isinstance(descriptor_sets, np.ndarray) and descriptor_sets.ndim == 3
        p = params if params is not None else sc_params(**kw)
        shape = (-1, int(p.n_sectors), int(p.n_rings))
        S = [np.ascontiguousarray(d, dtype=np.uint32).reshape(shape) for d in ([descriptor_sets] if single else list(descriptor_sets))]
        off = np.concatenate([[0], np.cumsum([len(d) for d in S])]).astype(np.int32)
        bins = np.ascontiguousarray(np.concatenate(S, axis=0)) if S else np.zeros((0,) + shape[1:], dtype=np.uint32)
        cap = int(off[-1]) * int(p.max_per_node)
        out = np.zeros(max(cap, 1), dtype=SC_CANDIDATE_DTYPE)
        n = C.c_int()
        self._check(self._L.cfear_scan_context_match(self._h, C.byref(p), len(S), off.ctypes.data, bins.ctypes.data if len(bins) else None, out.ctypes.data, cap,
                                                     C.byref(n)), "cfear_scan_context_match")
        return out[:n.value].copy()

    def odometry(self, n_sequences, overlap=None, filter_cus=None, max_cells=None, reg_order=None, large_kernel=None):
        """overlap: None = the context's setting; 0 / False = the three kernels in turn on the context stream; n >= 1 = the filter one
        sweep ahead on a low-priority stream, features / registration of n ranges of the sequences on n high-priority streams.
        The keyword settings apply to THIS object only: the context's own cfear_tune values are put back afterwards (an object
        created later without the keyword does not inherit them)."""
        want = [(TUNE_ODOMETRY_OVERLAP, overlap), (TUNE_FILTER_CUS, filter_cus), (TUNE_REGISTRATION_ORDER, reg_order), (TUNE_MAX_CELLS, max_cells),
                (TUNE_LARGE_SUBMAP_KERNEL, large_kernel)]
        saved = []
        try:
            for key, v in want:
                if v is not None:
                    saved.append((key, self._tuned.get(key, TUNE_DEFAULTS[key])))
                    self.tune(key, int(v))
            return Odometry(self, n_sequences)
        finally:
            for key, v in reversed(saved):
                self.tune(key, v)


class Cloud:
    def __init__(self, ctx, h):
        self._ctx, self._h = ctx, h

    def release(self):
        if self._h and self._ctx._h:
            self._ctx._L.cfear_cloud_release(self._ctx._h, self._h)
        self._h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    @property
    def size(self):
        n = C.c_int()
        self._ctx._check(self._ctx._L.cfear_cloud_size(self._ctx._h, self._h, C.byref(n)), "cfear_cloud_size")
        return n.value

    def download(self):
        n = self.size
        out = np.zeros((max(n, 1), 3), dtype=np.float32)
        m = C.c_int()
        self._ctx._check(self._ctx._L.cfear_cloud_download(self._ctx._h, self._h, out.ctypes.data, n, C.byref(m)),
                         "cfear_cloud_download")
        return out[:n]


class Scan:
    def __init__(self, ctx, h):
        self._ctx, self._h = ctx, h

    def release(self):
        if self._h and self._ctx._h:
            self._ctx._L.cfear_scan_release(self._ctx._h, self._h)
        self._h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    @property
    def size(self):
        n = C.c_int()
        self._ctx._check(self._ctx._L.cfear_scan_size(self._ctx._h, self._h, C.byref(n)), "cfear_scan_size")
        return n.value

    def cells(self):
        n = self.size
        out = np.zeros(max(n, 1), dtype=CELL_DTYPE)
        m = C.c_int()
        self._ctx._check(self._ctx._L.cfear_scan_download_cells(self._ctx._h, self._h, out.ctypes.data, n, C.byref(m)),
                         "cfear_scan_download_cells")
        return out[:n]

    def closest(self, qxy, d):
        q = np.ascontiguousarray(qxy, dtype=np.float64).reshape(-1, 2)
        idx = np.zeros(q.shape[0], dtype=np.int32)
        self._ctx._check(self._ctx._L.cfear_scan_closest(self._ctx._h, self._h, q.ctypes.data, q.shape[0], float(d),
                                                         idx.ctypes.data), "cfear_scan_closest")
        return idx


class DriftPlan:
    """cfear_drift_plan: one ground truth, ready to score batches of trajectories on the device (Context.drift_plan)"""

    def __init__(self, ctx, h, n_gt):
        self._ctx, self._h, self.n_gt = ctx, h, int(n_gt)

    def release(self):
        if self._h and self._ctx._h:
            self._ctx._L.cfear_drift_plan_release(self._ctx._h, self._h)
        self._h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def score(self, poses, n_sweeps=None, n_sequences=None, sweep_stride=None, seq_stride=None, out=None):
        """The KITTI drift of B trajectories -> structured array [B] of DRIFT_DTYPE. poses:
        a numpy float64 array [n, B, 3] of (x, y, theta), or a numpy array [n, B] of SWEEP_RECORD_DTYPE (what replay_host returns): the
        host route (cfear_drift_host; n_sweeps may shorten the trajectories);
        a device tensor or address with n_sweeps, n_sequences and the two strides in bytes (cfear_drift_device; for a buffer of sweep
        records 80 and n_sequences * 80, the defaults; 24 and n_sequences * 24 for packed poses). out: None - the results are copied to
        the host after the context has been synchronised - or a device tensor / address of n_sequences * 184 bytes: the call only
        queues the work on the context stream and returns None."""
        c = self._ctx
        if isinstance(poses, np.ndarray):
            a = poses
            if a.dtype != SWEEP_RECORD_DTYPE:
                a = np.asarray(a, dtype=np.float64)
                if a.ndim == 2:
                    a = a[:, None, :]
                if a.ndim != 3 or a.shape[2] != 3:
                    raise ValueError("DriftPlan.score: poses are [n, B, 3] doubles or [n, B] sweep records")
                a = np.ascontiguousarray(a)
                n, B, seq = a.shape[0], a.shape[1], 24
            else:
                a = np.ascontiguousarray(a if a.ndim == 2 else a[:, None])
                n, B, seq = a.shape[0], a.shape[1], SWEEP_RECORD_DTYPE.itemsize
            n = n if n_sweeps is None else int(n_sweeps)
            if n > a.shape[0]:
                raise ValueError("DriftPlan.score: n_sweeps %d of %d poses" % (n, a.shape[0]))
            if n_sequences is not None and int(n_sequences) != B:
                raise ValueError("DriftPlan.score: n_sequences %d of %d trajectories" % (int(n_sequences), B))
            res = np.zeros(B, dtype=DRIFT_DTYPE)
            c._check(c._L.cfear_drift_host(c._h, self._h, a.ctypes.data, B * seq, seq, n, B, res.ctypes.data), "cfear_drift_host")
            return res
        if n_sweeps is None or n_sequences is None:
            raise ValueError("DriftPlan.score: a device buffer needs n_sweeps and n_sequences")
        B = int(n_sequences)
        seq = SWEEP_RECORD_DTYPE.itemsize if seq_stride is None else int(seq_stride)
        sweep = B * seq if sweep_stride is None else int(sweep_stride)
        if out is not None:
            c._check(c._L.cfear_drift_device(c._h, self._h, _addr(poses), sweep, seq, int(n_sweeps), B, _addr(out)), "cfear_drift_device")
            return None
        import torch
        d_out = torch.empty(B * DRIFT_DTYPE.itemsize, dtype=torch.uint8, device="cuda:%d" % c.device)
        torch.cuda.synchronize(d_out.device)  # (the allocator's stream may still use the memory; the context stream writes it)
        c._check(c._L.cfear_drift_device(c._h, self._h, _addr(poses), sweep, seq, int(n_sweeps), B, d_out.data_ptr()), "cfear_drift_device")
        c.synchronize()
        return d_out.cpu().numpy().view(DRIFT_DTYPE).copy()


class Odometry:
    """Batched OdometryKeyframeFuser: B independent sequences, all state on the device."""

    def __init__(self, ctx, n_sequences):
        self._ctx, self.B = ctx, int(n_sequences)
        self.n_sources = self.B  # input sweeps per step (set_sequence_sources)
        self._h = C.c_void_p()
        ctx._check(ctx._L.cfear_odometry_create(ctx._h, self.B, C.byref(self._h)), "cfear_odometry_create")

    def release(self):
        if self._h and self._ctx._h:
            self._ctx._L.cfear_odometry_destroy(self._ctx._h, self._h)
        self._h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def reset(self):
        self._ctx._check(self._ctx._L.cfear_odometry_reset(self._ctx._h, self._h), "cfear_odometry_reset")

    def step_device(self, d_polar):
        self._ctx._check(self._ctx._L.cfear_odometry_step_device(self._ctx._h, self._h, _addr(d_polar)),
                         "cfear_odometry_step_device")

    def step_cloud_device(self, d_xyi, capacity, d_counts):
        """clouds on the device (raw pointers): [B][capacity][3] floats, [B] int32 counts"""
        self._ctx._check(self._ctx._L.cfear_odometry_step_cloud_device(self._ctx._h, self._h, C.c_void_p(int(d_xyi)), int(capacity), C.c_void_p(int(d_counts))),
                         "cfear_odometry_step_cloud_device")

    def step_host(self, polar):
        polar = np.ascontiguousarray(polar, dtype=np.uint8)
        assert polar.shape == (self.n_sources, self._ctx.A, self._ctx.R), polar.shape
        self._ctx._check(self._ctx._L.cfear_odometry_step_host(self._ctx._h, self._h, polar.ctypes.data),
                         "cfear_odometry_step_host")

    def replay_host(self, frames, records=True, covariances=False):
        """frames: uint8 [n, B, A, R] (or [n, A, R] for one sequence; [n, n_sources, A, R] with a source map), e.g. a view of Context.pinned(). Runs the n sweeps with
        no host round trip in between; -> structured array [n, B] of SWEEP_RECORD_DTYPE (or None). covariances=True: -> (records,
        [n, B, 6, 6] cov_current after every sweep) (cfear_odometry_replay_host_cov)."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        if frames.ndim == 3:
            frames = frames[:, None]
        assert frames.shape[1:] == (self.n_sources, self._ctx.A, self._ctx.R), frames.shape
        n = frames.shape[0]
        rec = np.zeros((n, self.B), dtype=SWEEP_RECORD_DTYPE) if records else None
        if not covariances:
            self._ctx._check(self._ctx._L.cfear_odometry_replay_host(self._ctx._h, self._h, frames.ctypes.data, n,
                                                                     rec.ctypes.data if records else None), "cfear_odometry_replay_host")
            return rec
        cov = np.zeros((n, self.B, 36))
        self._ctx._check(self._ctx._L.cfear_odometry_replay_host_cov(self._ctx._h, self._h, frames.ctypes.data, n, rec.ctypes.data if records else None,
                                                                     cov.ctypes.data), "cfear_odometry_replay_host_cov")
        return rec, cov.reshape(n, self.B, 6, 6)

    def replay_device(self, d_frames, n_sweeps, d_records=None, d_cov=None):
        """d_frames: device pointer / torch tensor of n_sweeps x B x A x R bytes; d_records: device buffer of n_sweeps x B x 80 bytes or
        None; d_cov: device buffer of n_sweeps x B x 36 doubles (cov_current after every sweep) or None. Asynchronous on the context stream."""
        if d_cov is None:
            self._ctx._check(self._ctx._L.cfear_odometry_replay_device(self._ctx._h, self._h, _addr(d_frames), int(n_sweeps),
                                                                       _addr(d_records) if d_records is not None else None), "cfear_odometry_replay_device")
            return
        self._ctx._check(self._ctx._L.cfear_odometry_replay_device_cov(self._ctx._h, self._h, _addr(d_frames), int(n_sweeps),
                                                                       _addr(d_records) if d_records is not None else None, _addr(d_cov)),
                         "cfear_odometry_replay_device_cov")

    def set_sequence_params(self, rows):
        """rows: one Params per sequence (the points of a parameter grid, utils/worker:26-99; replay.param_grid builds them), or None for
        the context's parameters again (cfear_odometry_set_sequence_params). Before the first sweep since creation / reset()."""
        if rows is None:
            self._ctx._check(self._ctx._L.cfear_odometry_set_sequence_params(self._ctx._h, self._h, None, 0), "cfear_odometry_set_sequence_params")
            return
        rows = list(rows)
        arr = (Params * len(rows))(*rows)
        self._ctx._check(self._ctx._L.cfear_odometry_set_sequence_params(self._ctx._h, self._h, C.cast(arr, C.c_void_p), len(rows)),
                         "cfear_odometry_set_sequence_params")

    def sequence_params(self, q):
        """the Params sequence q runs with (cfear_odometry_sequence_params)"""
        p = Params()
        self._ctx._check(self._ctx._L.cfear_odometry_sequence_params(self._ctx._h, self._h, int(q), C.byref(p)), "cfear_odometry_sequence_params")
        return p

    def set_sequence_sources(self, source, n_sources=None):
        """source[q]: the input sweep sequence q reads; afterwards step_host / step_device / the replays take n_sources sweeps per step
        instead of B. None: one sweep per sequence again (cfear_odometry_set_sequence_sources)."""
        if source is None:
            self._ctx._check(self._ctx._L.cfear_odometry_set_sequence_sources(self._ctx._h, self._h, None, 0, 0), "cfear_odometry_set_sequence_sources")
            self.n_sources = self.B
            return
        src = np.ascontiguousarray(source, dtype=np.int32)
        ns = int(n_sources) if n_sources is not None else int(src.max()) + 1
        self._ctx._check(self._ctx._L.cfear_odometry_set_sequence_sources(self._ctx._h, self._h, src.ctypes.data, int(src.size), ns),
                         "cfear_odometry_set_sequence_sources")
        self.n_sources = ns

    def set_sequence_shapes(self, shapes):
        """shapes: one SeqShape (or (cost, submap_scan_size) pair) per sequence - the cost metric and the submap size it runs with, any
        submap_scan_size up to the context's - or None for the context's values again (cfear_odometry_set_sequence_shapes). Before the first
        sweep since creation / reset(), and before a parameter table whose rows carry these values."""
        fn, c = self._ctx._L.cfear_odometry_set_sequence_shapes, self._ctx
        if shapes is None:
            c._check(fn(c._h, self._h, None, 0), "cfear_odometry_set_sequence_shapes")
            return
        shapes = [s if isinstance(s, SeqShape) else SeqShape(int(s[0]), int(s[1])) for s in shapes]
        arr = (SeqShape * len(shapes))(*shapes)
        c._check(fn(c._h, self._h, C.cast(arr, C.c_void_p), len(shapes)), "cfear_odometry_set_sequence_shapes")

    def sequence_shape(self, q):
        """the SeqShape sequence q runs with (cfear_odometry_sequence_shape)"""
        s = SeqShape()
        self._ctx._check(self._ctx._L.cfear_odometry_sequence_shape(self._ctx._h, self._h, int(q), C.byref(s)), "cfear_odometry_sequence_shape")
        return s

    def set_sequence_detectors(self, dets, source=None, n_sources=None):
        """dets: one SeqDetector (or (window_size, nb_guard_cells, false_alarm_rate, z_min) tuple) per sequence of a filter_type CA-CFAR
        object; source[q]: the input sweep sequence q reads (None: one sweep per sequence) - afterwards step_host / step_device / the
        replays take n_sources sweeps per step, staged once each, every distinct (sweep, detector) decided once. dets None: the
        context's detector and one sweep per sequence again (cfear_odometry_set_sequence_detectors). Before the first sweep since
        creation / reset()."""
        fn, c = self._ctx._L.cfear_odometry_set_sequence_detectors, self._ctx
        if dets is None:
            c._check(fn(c._h, self._h, None, 0, None, 0), "cfear_odometry_set_sequence_detectors")
            self.n_sources = self.B
            return
        arr = detector_array(dets)
        if source is None:
            c._check(fn(c._h, self._h, C.cast(arr, C.c_void_p), len(arr), None, 0), "cfear_odometry_set_sequence_detectors")
            self.n_sources = self.B
            return
        src = np.ascontiguousarray(source, dtype=np.int32)
        ns = int(n_sources) if n_sources is not None else int(src.max()) + 1
        if src.size != len(arr):
            raise ValueError("set_sequence_detectors: %d detectors, %d sources" % (len(arr), src.size))
        c._check(fn(c._h, self._h, C.cast(arr, C.c_void_p), len(arr), src.ctypes.data, ns), "cfear_odometry_set_sequence_detectors")
        self.n_sources = ns

    def sequence_detector(self, q):
        """the SeqDetector sequence q runs with (cfear_odometry_sequence_detector)"""
        d = SeqDetector()
        self._ctx._check(self._ctx._L.cfear_odometry_sequence_detector(self._ctx._h, self._h, int(q), C.byref(d)), "cfear_odometry_sequence_detector")
        return d

    def set_fuser_options(self, rows):
        """rows: one FuserOptions for every sequence, a list of one per sequence, or None for the defaults again
        (cfear_odometry_set_fuser_options). Before the first sweep since creation / reset()."""
        fn, c = self._ctx._L.cfear_odometry_set_fuser_options, self._ctx
        if rows is None:
            c._check(fn(c._h, self._h, None, 0), "cfear_odometry_set_fuser_options")
            return
        rows = [rows] if isinstance(rows, FuserOptions) else list(rows)
        arr = (FuserOptions * len(rows))(*rows)
        c._check(fn(c._h, self._h, C.cast(arr, C.c_void_p), len(rows)), "cfear_odometry_set_fuser_options")

    def fuser_options(self, q):
        """the FuserOptions sequence q runs with (cfear_odometry_fuser_options)"""
        o = FuserOptions()
        self._ctx._check(self._ctx._L.cfear_odometry_fuser_options(self._ctx._h, self._h, int(q), C.byref(o)), "cfear_odometry_fuser_options")
        return o

    def set_cov_sampling(self, enable=True, xy_range=0.4, yaw_range=0.0043625, samples_per_axis=3, covariance_scaler=4.0):
        """estimate_cov_by_sampling and its companions (odometrykeyframefuser.h:104-110) for every sequence, from the next sweep on"""
        self._ctx._check(self._ctx._L.cfear_odometry_set_cov_sampling(self._ctx._h, self._h, int(bool(enable)), float(xy_range), float(yaw_range),
                                                                       int(samples_per_axis), float(covariance_scaler)), "cfear_odometry_set_cov_sampling")
        if enable:
            self._cov_m = int(samples_per_axis) ** 3

    def cov_samples(self, sequence):
        """the last sweep's sampled costs of one sequence (samples_per_axis^3, the reference's order) and whether the sampled
        covariance was used -> (costs, sampled)"""
        costs = np.zeros(getattr(self, "_cov_m", 1))
        ok = C.c_int()
        self._ctx._check(self._ctx._L.cfear_odometry_cov_samples(self._ctx._h, self._h, int(sequence), costs.ctypes.data, C.byref(ok)),
                         "cfear_odometry_cov_samples")
        return costs, bool(ok.value)

    def set_surface_recording(self, enable=True):
        """every registration records what it used, for surface() (cfear_odometry_set_surface_recording); off by default"""
        self._ctx._check(self._ctx._L.cfear_odometry_set_surface_recording(self._ctx._h, self._h, int(bool(enable))),
                         "cfear_odometry_set_surface_recording")

    def surface(self, res, width, details=False):
        """GetSurface of every sequence around its last registration -> torch float64 tensor [B, pixels, pixels] on the context's device
        (NaN where nothing was evaluated). details=True: also (n_used [B], itr_used [B], poses_used [B, 64, 3]) as numpy arrays.
        Synchronises the context before returning, so the tensor is ready on any stream."""
        import torch
        pixels = surface_dims(res, width)[0]
        out = torch.empty((self.B, pixels, pixels), dtype=torch.float64, device="cuda:%d" % self._ctx.device)
        torch.cuda.synchronize(out.device)  # (the allocator's stream may still use the memory; the context stream writes it)
        n_used, itr_used = np.zeros(self.B, dtype=np.int32), np.zeros(self.B, dtype=np.int32)
        poses_used = np.zeros((self.B, 64, 3))
        c = self._ctx
        c._check(c._L.cfear_odometry_surface(c._h, self._h, float(res), int(width), out.data_ptr(), n_used.ctypes.data, itr_used.ctypes.data,
                                             poses_used.ctypes.data), "cfear_odometry_surface")
        c._check(c._L.cfear_synchronize(c._h), "cfear_synchronize")
        return (out, n_used, itr_used, poses_used) if details else out

    def profile(self, enable):
        self._ctx._check(self._ctx._L.cfear_odometry_profile(self._ctx._h, self._h, int(enable)), "cfear_odometry_profile")

    def profile_read(self):
        """-> (filter seconds, filter launches)"""
        tf, nf = C.c_double(), C.c_int()
        self._ctx._check(self._ctx._L.cfear_odometry_profile_read(self._ctx._h, self._h, C.byref(tf), C.byref(nf)),
                         "cfear_odometry_profile_read")
        return tf.value, nf.value

    def profile_read_stages(self):
        """-> (features seconds, registration seconds, launches of each)"""
        tf, tr, n = C.c_double(), C.c_double(), C.c_int()
        self._ctx._check(self._ctx._L.cfear_odometry_profile_read_stages(self._ctx._h, self._h, C.byref(tf), C.byref(tr), C.byref(n)),
                         "cfear_odometry_profile_read_stages")
        return tf.value, tr.value, n.value

    def phase_times(self, mode, light=False, workgroups_only=False, controller=False):
        """None: switch to the timed kernel instantiations (light: phase stamps only, without the per-LM-command clock reads that
        halve the speed of the registration kernel; workgroups_only: production kernels, start / end clock per workgroup; controller: slots 0..7 of a sequence hold the
        breakdown of the registration's command loop instead of the feature kernel's stamps); True: read + clear the [B][32] tick table of the steps since the last read;
        False: back to the production kernels."""
        L, c = self._ctx._L, self._ctx
        if mode is None:
            c._check(L.cfear_odometry_phase_times(c._h, self._h, 3 if workgroups_only else (4 if controller else (2 if light else 1)), None), "cfear_odometry_phase_times")
            return None
        if mode is False:
            c._check(L.cfear_odometry_phase_times(c._h, self._h, 0, None), "cfear_odometry_phase_times")
            return None
        buf = np.zeros((self.B, 32), dtype=np.int64)
        c._check(L.cfear_odometry_phase_times(c._h, self._h, -1, buf.ctypes.data), "cfear_odometry_phase_times")
        return buf

    # ---- the keyframe graph (AddToGraph, odometrykeyframefuser.cpp:428-445) ----
    def record_keyframes(self, what=KF_NODES | KF_CELLS, max_keyframes=1024, max_cells=0, max_points=0):
        """cfear_odometry_set_keyframe_recording: what = 0 (off), KF_NODES or KF_NODES | KF_CELLS; the capacities are per sequence (nodes;
        cells summed over its keyframes). Switching on needs an object that has processed no sweep since it was created / reset.
        what | KF_CLOUD (| KF_PEAKS) also records every node's motion-compensated filtered (and peaks) cloud
        (cfear_odometry_set_keyframe_clouds): max_points per sequence, summed over both clouds of all its keyframes."""
        what = int(what)
        if what & KF_PEAKS and not what & KF_CLOUD:
            raise CfearError("record_keyframes: KF_PEAKS needs KF_CLOUD (the peaks cloud is recorded beside the filtered cloud)")
        if what & (KF_CLOUD | KF_PEAKS) and not what & KF_NODES:
            raise CfearError("record_keyframes: KF_CLOUD needs KF_NODES (the clouds belong to recorded nodes)")
        self._ctx._check(self._ctx._L.cfear_odometry_set_keyframe_recording(self._ctx._h, self._h, what & ~(KF_CLOUD | KF_PEAKS), int(max_keyframes),
                                                                            int(max_cells)), "cfear_odometry_set_keyframe_recording")
        if what & KF_CLOUD:
            self.record_keyframe_clouds(what & (KF_CLOUD | KF_PEAKS), max_points)

    def record_keyframe_clouds(self, what=KF_CLOUD | KF_PEAKS, max_points=0):
        """cfear_odometry_set_keyframe_clouds on an object whose node recording is on: what = 0 (off, at any time), KF_CLOUD or KF_CLOUD | KF_PEAKS"""
        self._ctx._check(self._ctx._L.cfear_odometry_set_keyframe_clouds(self._ctx._h, self._h, int(what), int(max_points)), "cfear_odometry_set_keyframe_clouds")

    def keyframe_counts(self):
        """-> (recorded [B], dropped [B]) keyframes per sequence"""
        rec, drop = np.zeros(self.B, dtype=np.int32), np.zeros(self.B, dtype=np.int32)
        self._ctx._check(self._ctx._L.cfear_odometry_keyframe_counts(self._ctx._h, self._h, rec.ctypes.data, drop.ctypes.data), "cfear_odometry_keyframe_counts")
        return rec, drop

    def keyframes(self, q):
        """the recorded nodes of sequence q -> structured array of KEYFRAME_NODE_DTYPE"""
        n = C.c_int()
        self._ctx._check(self._ctx._L.cfear_odometry_keyframe_nodes(self._ctx._h, self._h, int(q), 0, None, 0, C.byref(n)), "cfear_odometry_keyframe_nodes")
        out = np.zeros(max(n.value, 1), dtype=KEYFRAME_NODE_DTYPE)
        self._ctx._check(self._ctx._L.cfear_odometry_keyframe_nodes(self._ctx._h, self._h, int(q), 0, out.ctypes.data, n.value, C.byref(n)), "cfear_odometry_keyframe_nodes")
        return out[:n.value]

    def keyframe_cells(self, q, i):
        """the cells of keyframe i of sequence q, in the scan's order -> structured array of KEYFRAME_CELL_DTYPE"""
        n = C.c_int()
        self._ctx._check(self._ctx._L.cfear_odometry_keyframe_cells(self._ctx._h, self._h, int(q), int(i), None, 0, C.byref(n)), "cfear_odometry_keyframe_cells")
        out = np.zeros(max(n.value, 1), dtype=KEYFRAME_CELL_DTYPE)
        self._ctx._check(self._ctx._L.cfear_odometry_keyframe_cells(self._ctx._h, self._h, int(q), int(i), out.ctypes.data, n.value, C.byref(n)), "cfear_odometry_keyframe_cells")
        return out[:n.value]

    def keyframe_scans(self, q, indices):
        """per-call Scans rebuilt from the recorded keyframes `indices` of sequence q in one launch (cfear_odometry_keyframe_scans): ready for
        Context.register / get_cost; their downloadable cells carry intensities 0. -> list of Scan"""
        idx = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1)
        arr = (C.c_void_p * len(idx))()
        self._ctx._check(self._ctx._L.cfear_odometry_keyframe_scans(self._ctx._h, self._h, int(q), idx.ctypes.data, len(idx), arr), "cfear_odometry_keyframe_scans")
        return [Scan(self._ctx, C.c_void_p(h)) for h in arr]

    def keyframe_edges(self, jobs, details=False):
        """cfear_odometry_keyframe_edges: constraints between any keyframes of the log, all jobs registered in one launch. jobs: a structured
        array of KEYFRAME_EDGE_JOB_DTYPE, or a list of dicts / tuples (keyframe_edge_jobs). -> the edges (KEYFRAME_EDGE_DTYPE), one per job;
        details=True: (edges, cov6 [m, 6, 6], [RegSummary] * m) - every job's covariance and summary as Context.register returns them."""
        J = keyframe_edge_jobs(jobs)
        m = len(J)
        edges = np.zeros(m, dtype=KEYFRAME_EDGE_DTYPE)
        cov = np.zeros((m, 6, 6)) if details else None
        sums = (RegSummary * max(m, 1))() if details else None
        self._ctx._check(self._ctx._L.cfear_odometry_keyframe_edges(self._ctx._h, self._h, J.ctypes.data, m, edges.ctypes.data, cov.ctypes.data if details else None,
                                                                    sums if details else None), "cfear_odometry_keyframe_edges")
        return (edges, cov, [sums[i] for i in range(m)]) if details else edges

    def keyframe_optimize(self, edges=None, options=None, **kw):
        """cfear_odometry_keyframe_optimize: the graphs of the log, one per sequence, optimised in one launch - the chain and the initial
        poses are read from the recorded nodes on the device, edges (KEYFRAME_EDGE_DTYPE, as keyframe_edges returned them; any sequences,
        any order; those without success are left out) join them under the options' loss. options: a PgOptions, or its fields as keywords.
        -> (per sequence an array [n_q, 3] of optimised poses, summaries: PG_SUMMARY_DTYPE [B]). Nothing is written to the log."""
        E = np.zeros(0, dtype=KEYFRAME_EDGE_DTYPE) if edges is None else np.ascontiguousarray(edges, dtype=KEYFRAME_EDGE_DTYPE).reshape(-1)
        opt = options if options is not None else pg_options(**kw)
        off = np.zeros(self.B + 1, dtype=np.int32)
        fn, ctx = self._ctx._L.cfear_odometry_keyframe_optimize, self._ctx
        ep = E.ctypes.data if len(E) else None
        ctx._check(fn(ctx._h, self._h, ep, len(E), C.byref(opt), None, 0, off.ctypes.data, None), "cfear_odometry_keyframe_optimize")
        x = np.zeros((max(int(off[-1]), 1), 3))
        sums = np.zeros(self.B, dtype=PG_SUMMARY_DTYPE)
        ctx._check(fn(ctx._h, self._h, ep, len(E), C.byref(opt), x.ctypes.data, int(off[-1]), off.ctypes.data, sums.ctypes.data), "cfear_odometry_keyframe_optimize")
        return [x[off[q]:off[q + 1]].copy() for q in range(self.B)], sums

    def keyframe_descriptors(self, q, params=None, **kw):
        """cfear_odometry_keyframe_descriptors: the Scan-Context descriptors of every recorded keyframe, from the point log on the device in
        one launch; those of sequence q come back -> (bins uint32 [n, n_sectors, n_rings], ring_sums uint32 [n, n_rings]). params: a ScParams,
        or its fields as keywords (source=1: of the peaks clouds). Needs a log with KF_CLOUD. Nothing is written to the log."""
        p = params if params is not None else sc_params(**kw)
        fn, ctx = self._ctx._L.cfear_odometry_keyframe_descriptors, self._ctx
        n = C.c_int()
        ctx._check(fn(ctx._h, self._h, C.byref(p), int(q), 0, None, None, 0, C.byref(n)), "cfear_odometry_keyframe_descriptors")
        bins = np.zeros((max(n.value, 1), int(p.n_sectors), int(p.n_rings)), dtype=np.uint32)
        ring = np.zeros((max(n.value, 1), int(p.n_rings)), dtype=np.uint32)
        ctx._check(fn(ctx._h, self._h, C.byref(p), int(q), 0, bins.ctypes.data, ring.ctypes.data, n.value, C.byref(n)), "cfear_odometry_keyframe_descriptors")
        return bins[:n.value], ring[:n.value]

    def keyframe_candidates(self, params=None, **kw):
        """cfear_odometry_keyframe_candidates: loop candidates by appearance for every sequence of the object - describe and match on the
        device, no cloud or descriptor comes to the host -> SC_CANDIDATE_DTYPE, (sequence, to, distance) ascending (replay.appearance_jobs
        turns a sequence's into keyframe_edges jobs). Nothing is written to the log."""
        p = params if params is not None else sc_params(**kw)
        fn, ctx = self._ctx._L.cfear_odometry_keyframe_candidates, self._ctx
        cap = int(self.keyframe_counts()[0].sum()) * int(p.max_per_node)
        out = np.zeros(max(cap, 1), dtype=SC_CANDIDATE_DTYPE)
        n = C.c_int()
        ctx._check(fn(ctx._h, self._h, C.byref(p), out.ctypes.data, cap, C.byref(n)), "cfear_odometry_keyframe_candidates")
        return out[:n.value].copy()

    def keyframe_cloud_sizes(self, q):
        """-> (n_cloud [n], n_peaks [n]): points of the filtered and of the peaks cloud of every recorded node of sequence q"""
        n = C.c_int()
        self._ctx._check(self._ctx._L.cfear_odometry_keyframe_cloud_sizes(self._ctx._h, self._h, int(q), 0, None, None, 0, C.byref(n)), "cfear_odometry_keyframe_cloud_sizes")
        nc, npk = np.zeros(max(n.value, 1), dtype=np.int32), np.zeros(max(n.value, 1), dtype=np.int32)
        self._ctx._check(self._ctx._L.cfear_odometry_keyframe_cloud_sizes(self._ctx._h, self._h, int(q), 0, nc.ctypes.data, npk.ctypes.data, n.value, C.byref(n)),
                         "cfear_odometry_keyframe_cloud_sizes")
        return nc[:n.value], npk[:n.value]

    def keyframe_cloud(self, q, i, peaks=False):
        """the filtered (peaks=True: the peaks) cloud of keyframe i of sequence q -> float32 [n, 3]: x, y, intensity"""
        n = C.c_int()
        self._ctx._check(self._ctx._L.cfear_odometry_keyframe_cloud(self._ctx._h, self._h, int(q), int(i), int(bool(peaks)), None, 0, C.byref(n)),
                         "cfear_odometry_keyframe_cloud")
        out = np.zeros((max(n.value, 1), 3), dtype=np.float32)
        self._ctx._check(self._ctx._L.cfear_odometry_keyframe_cloud(self._ctx._h, self._h, int(q), int(i), int(bool(peaks)), out.ctypes.data, n.value, C.byref(n)),
                         "cfear_odometry_keyframe_cloud")
        return out[:n.value]

    def keyframe_clouds(self, q, indices, peaks=False):
        """the recorded clouds of keyframes `indices` of sequence q as device Clouds (cfear_odometry_keyframe_clouds): ready for
        Context.scan_create at any res, Cloud.download. -> list of Cloud"""
        idx = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1)
        arr = (C.c_void_p * len(idx))()
        self._ctx._check(self._ctx._L.cfear_odometry_keyframe_clouds(self._ctx._h, self._h, int(q), idx.ctypes.data, len(idx), int(bool(peaks)), arr),
                         "cfear_odometry_keyframe_clouds")
        return [Cloud(self._ctx, C.c_void_p(h)) for h in arr]

    def poses(self):
        out = np.zeros((self.B, 3))
        self._ctx._check(self._ctx._L.cfear_odometry_poses(self._ctx._h, self._h, out.ctypes.data), "cfear_odometry_poses")
        return out

    def status(self, per_sequence=False):
        """raises CfearError (rc=-6) if a scan of this object was truncated (cfear_odometry_status); per_sequence=True: returns the per-sequence
        flag words instead of raising (bit 0 = STATUS_CELLS_LOST, bit 1 = STATUS_POINTS_LOST, bit 2 = STATUS_KEYFRAMES_DROPPED: the sequence's keyframe
        log is full - no error of the odometry, the call does not raise for it)"""
        if per_sequence:
            out = np.zeros(self.B, dtype=np.int32)
            rc = self._ctx._L.cfear_odometry_status(self._ctx._h, self._h, out.ctypes.data)
            if rc not in (0, -6):  # (0 and CFEAR_ERR_CAPACITY are what the flag words describe; anything else - a HIP error, a failed join - is not)
                self._ctx._check(rc, "cfear_odometry_status")
            return out
        self._ctx._check(self._ctx._L.cfear_odometry_status(self._ctx._h, self._h, None), "cfear_odometry_status")

    def covariances(self):
        """cov_current of every sequence after the last sweep: [B, 6, 6]"""
        out = np.zeros((self.B, 36))
        self._ctx._check(self._ctx._L.cfear_odometry_covariances(self._ctx._h, self._h, out.ctypes.data), "cfear_odometry_covariances")
        return out.reshape(self.B, 6, 6)

    def summary(self, sequence):
        S = RegSummary()
        nc, nk = C.c_int(), C.c_int()
        self._ctx._check(self._ctx._L.cfear_odometry_summary(self._ctx._h, self._h, int(sequence), C.byref(S), C.byref(nc),
                                                             C.byref(nk)), "cfear_odometry_summary")
        return S, nc.value, nk.value
