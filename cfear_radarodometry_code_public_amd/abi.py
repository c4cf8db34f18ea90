"""The image of include/cfear_hip.h in ctypes, stated once: its records (a numpy dtype is derived from the structure, record_dtype), the constants
it defines, the signature of every export, and the loader. tests/test_abi_cpu.py compiles the header and asks it for every size, offset,
constant and argument count stated here. A new ABI entry is: the header, one SIGNATURES row, one Record if it has one, one method in capi.py."""
import ctypes as C
import os

import numpy as np

from . import build as _build

_LIB = None


class CfearError(RuntimeError):
    pass


def _show(v):
    return [_show(x) for x in v] if isinstance(v, C.Array) else v


class Record(C.Structure):
    """a struct of the header: _c_name_ names it there; every field carries the header's name (getattr for `from`)"""

    def __repr__(self):
        return "%s(%s)" % (type(self).__name__, ", ".join("%s=%r" % (f, _show(getattr(self, f))) for f, _ in self._fields_ if f != "pad_"))


# ---- constants (plain assignments; HEADER_CONSTANTS below names the macro or enumerator of each) ----
CFEAR_MAX_OUTER = 64
ERR_INVALID, ERR_HIP, ERR_UNSUPPORTED, ERR_EMPTY, ERR_NOMEM, ERR_CAPACITY = -1, -2, -3, -4, -5, -6
COST_P2P, COST_P2L, COST_P2D = 0, 1, 2
LOSS_NONE, LOSS_HUBER, LOSS_CAUCHY = 0, 1, 2  # the losses the pose-graph optimiser takes
FILTER_KSTRONG, FILTER_CACFAR = 0, 1
TUNE_FILTER_OCCUPANCY, TUNE_FILTER_ROWS_PER_WAVE, TUNE_ODOMETRY_OVERLAP, TUNE_REPLAY_PERSISTENT_MAX, TUNE_FILTER_CUS, TUNE_REPEAT_SHORTCUT = 1, 2, 3, 4, 5, 6
TUNE_MAX_CELLS, TUNE_REGISTRATION_ORDER, TUNE_LARGE_SUBMAP_KERNEL, TUNE_NN_TIE_RULE, TUNE_VOXEL_ORDER, TUNE_FILTER_PEAKS = 7, 8, 9, 10, 11, 12
CFAR_KERNELS = ("owner", "fast16", "fast32", "general")  # CFEAR_CFAR_KERNEL_*
KF_NODES, KF_CELLS = 1, 2
KF_CLOUD, KF_PEAKS = 4, 8  # (cfear_odometry_set_keyframe_clouds)
KF_EDGE_MAX_FROM = 16
PG_CONVERGED_COST, PG_CONVERGED_STEP, PG_ITERATION_LIMIT, PG_DAMPING_LIMIT, PG_NOTHING_TO_DO = 0, 1, 2, 3, 4
SC_MAX, SC_SUM, SC_COUNT = 0, 1, 2
SC_MAX_RINGS, SC_MAX_SECTORS, SC_MAX_KEYS, SC_MAX_PER_NODE, SC_MAX_POINTS = 40, 120, 64, 16, 65536

_PREFIXES = ("ERR_", "COST_", "LOSS_", "FILTER_", "TUNE_", "KF_", "PG_", "SC_")
HEADER_CONSTANTS = {"CFEAR_" + k: v for k, v in list(globals().items()) if k.startswith(_PREFIXES) and isinstance(v, int)}
HEADER_CONSTANTS.update({"CFEAR_CFAR_KERNEL_" + k.upper(): i for i, k in enumerate(CFAR_KERNELS)}, CFEAR_MAX_OUTER=CFEAR_MAX_OUTER)

# (not in the header)
PG_TERMINATION = ("converged on cost", "converged on step", "iteration limit", "damping limit", "nothing to do")
STATUS_CELLS_LOST, STATUS_POINTS_LOST, STATUS_KEYFRAMES_DROPPED = 1, 2, 4  # the bits of a sequence's word in cfear_odometry_status
TUNE_DEFAULTS = {TUNE_ODOMETRY_OVERLAP: 0, TUNE_FILTER_CUS: 0, TUNE_MAX_CELLS: 0, TUNE_REGISTRATION_ORDER: 1, TUNE_LARGE_SUBMAP_KERNEL: 0}  # include/cfear_hip.h


# ---- records ----
class Params(Record):
    _c_name_ = "cfear_params"
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


class FuserOptions(Record):
    """the fuser's soft_constraint and use_guess (odometrykeyframefuser.h:94) of a batched odometry object or of one of its sequences"""
    _c_name_ = "cfear_fuser_options"
    _fields_ = [("soft_constraint", C.c_int32), ("use_guess", C.c_int32)]


class SeqShape(Record):
    """the cost metric and the submap_scan_size of one sequence of a batched odometry object"""
    _c_name_ = "cfear_seq_shape"
    _fields_ = [("cost", C.c_int32), ("submap_scan_size", C.c_int32)]


class SeqDetector(Record):
    """the CA-CFAR detector of one cloud of Context.filter_cfar_grid or of one sequence of a filter_type CA-CFAR batched odometry object
    (Odometry.set_sequence_detectors)"""
    _c_name_ = "cfear_seq_detector"
    _fields_ = [("window_size", C.c_int32), ("nb_guard_cells", C.c_int32), ("false_alarm_rate", C.c_float), ("z_min", C.c_float)]

    def __repr__(self):  # (%g: the floats as they were given, not their float32 neighbours)
        return "SeqDetector(window_size=%d, nb_guard_cells=%d, false_alarm_rate=%g, z_min=%g)" % (
            self.window_size, self.nb_guard_cells, self.false_alarm_rate, self.z_min)


class CfarPlan(Record):
    """the launch plan of the CA-CFAR detector"""
    _c_name_ = "cfear_cfar_plan"
    _fields_ = [("kernel", C.c_int32), ("TB", C.c_int32), ("NW", C.c_int32), ("RS", C.c_int32), ("full", C.c_int32), ("sh", C.c_int32), ("kopen", C.c_int32),
                ("rmin", C.c_int32), ("rmax", C.c_int32), ("cr", C.c_int32 * 4), ("cq", C.c_int32 * 4), ("padl", C.c_int32), ("fill", C.c_int32),
                ("lds_bytes", C.c_int32), ("per_cu", C.c_int32), ("workgroups", C.c_int32)]


class Cell(Record):
    _c_name_ = "cfear_cell"
    _fields_ = [
        ("mean", C.c_double * 2), ("cov", C.c_double * 3), ("normal", C.c_double * 2),
        ("orth", C.c_double * 2), ("lambda_min", C.c_double), ("lambda_max", C.c_double),
        ("scale", C.c_double), ("sum_intensity", C.c_double), ("avg_intensity", C.c_double),
        ("nsamples", C.c_int32), ("valid", C.c_int32),
    ]


class RegSummary(Record):
    _c_name_ = "cfear_reg_summary"
    _fields_ = [
        ("success", C.c_int32), ("usable", C.c_int32), ("outer_iterations", C.c_int32),
        ("num_residuals", C.c_int32), ("num_residual_blocks", C.c_int32), ("assoc_path", C.c_int32),
        ("final_cost", C.c_double), ("score", C.c_double),
        ("inner_iterations", C.c_int32 * CFEAR_MAX_OUTER), ("termination", C.c_int32 * CFEAR_MAX_OUTER),
        ("outer_cost", C.c_double * CFEAR_MAX_OUTER), ("outer_pose", (C.c_double * 3) * CFEAR_MAX_OUTER),
    ]


class SweepRecord(Record):
    """what a caller of pointcloudCallback sees after every sweep of a replay"""
    _c_name_ = "cfear_sweep_record"
    _fields_ = [("pose", C.c_double * 3), ("final_cost", C.c_double), ("outer_iterations", C.c_int32), ("num_residuals", C.c_int32),
                ("n_keyframes", C.c_int32), ("n_cells", C.c_int32), ("inner_iterations", C.c_int32 * 8)]


# the keyframe graph of the batched routes (AddToGraph, odometrykeyframefuser.cpp:428-445): a RadarScan node with its odometry constraint
# to the previous keyframe, and one of its cells
class KeyframeNode(Record):
    _c_name_ = "cfear_keyframe_node"
    _fields_ = [("index", C.c_int32), ("sweep", C.c_int32), ("n_cells", C.c_int32), ("prev", C.c_int32), ("pose", C.c_double * 3),
                ("motion", C.c_double * 3), ("t_be", C.c_double * 3), ("information", (C.c_double * 6) * 6)]


class KeyframeCell(Record):
    _c_name_ = "cfear_keyframe_cell"
    _fields_ = [("mean", C.c_double * 2), ("normal", C.c_double * 2), ("cov", C.c_double * 3), ("scale", C.c_double),
                ("nsamples", C.c_int32), ("pad_", C.c_int32)]


# a constraint between any keyframes of a log - keyframe `to` registered against the fixed keyframes `from` (cfear_odometry_keyframe_edges)
class KeyframeEdgeJob(Record):
    _c_name_ = "cfear_keyframe_edge_job"
    _fields_ = [("sequence", C.c_int32), ("to", C.c_int32), ("n_from", C.c_int32), ("ref", C.c_int32), ("flags", C.c_int32), ("pad_", C.c_int32),
                ("from", C.c_int32 * KF_EDGE_MAX_FROM), ("guess_xyt", C.c_double * 3)]


class KeyframeEdge(Record):
    _c_name_ = "cfear_keyframe_edge"
    _fields_ = [("sequence", C.c_int32), ("to", C.c_int32), ("from", C.c_int32), ("n_from", C.c_int32), ("status", C.c_int32), ("success", C.c_int32),
                ("usable", C.c_int32), ("outer_iterations", C.c_int32), ("num_residuals", C.c_int32), ("num_residual_blocks", C.c_int32),
                ("assoc_path", C.c_int32), ("pad_", C.c_int32), ("pose", C.c_double * 3), ("t_be", C.c_double * 3), ("final_cost", C.c_double),
                ("score", C.c_double), ("information", (C.c_double * 6) * 6)]


# the batched planar pose-graph optimiser (pose_graph.hip). An edge is a g2o `EDGE_SE2 a b ...` line as replay writes it; posegraph.py
# builds them from nodes and keyframe edges
class PgEdge(Record):
    _c_name_ = "cfear_pg_edge"
    _fields_ = [("a", C.c_int32), ("b", C.c_int32), ("flags", C.c_int32), ("pad_", C.c_int32), ("z", C.c_double * 3), ("info", C.c_double * 6)]


class PgOptions(Record):
    _c_name_ = "cfear_pg_options"
    _fields_ = [("max_iterations", C.c_int32), ("max_linear_iterations", C.c_int32), ("loss", C.c_int32), ("pad_", C.c_int32),
                ("linear_tolerance", C.c_double), ("function_tolerance", C.c_double), ("parameter_tolerance", C.c_double),
                ("initial_damping", C.c_double), ("loss_limit", C.c_double)]


class PgSummary(Record):
    _c_name_ = "cfear_pg_summary"
    _fields_ = [("initial_cost", C.c_double), ("final_cost", C.c_double), ("iterations", C.c_int32), ("accepted", C.c_int32),
                ("linear_iterations", C.c_int32), ("edges_used", C.c_int32), ("edges_skipped", C.c_int32), ("termination", C.c_int32),
                ("status", C.c_int32), ("pad_", C.c_int32)]


# Scan-Context descriptors and loop candidates by appearance (scan_context.hip). scancontext.py states the definition in numpy
class ScParams(Record):
    _c_name_ = "cfear_sc_params"
    _fields_ = [("n_rings", C.c_int32), ("n_sectors", C.c_int32), ("value", C.c_int32), ("source", C.c_int32), ("min_index_gap", C.c_int32),
                ("n_keys", C.c_int32), ("max_per_node", C.c_int32), ("pad_", C.c_int32), ("max_range", C.c_double), ("max_distance", C.c_double)]


class ScCandidate(Record):
    _c_name_ = "cfear_sc_candidate"
    _fields_ = [("sequence", C.c_int32), ("to", C.c_int32), ("from", C.c_int32), ("shift", C.c_int32), ("distance", C.c_double), ("yaw", C.c_double),
                ("key_distance", C.c_uint64)]


class Drift(Record):
    """the KITTI drift of one trajectory with its per-length table (100 ... 800 m)"""
    _c_name_ = "cfear_drift"
    _fields_ = [("translation_percent", C.c_double), ("rotation_deg_per_100m", C.c_double),
                ("translation_percent_by_length", C.c_double * 8), ("rotation_deg_per_100m_by_length", C.c_double * 8),
                ("segments", C.c_int32), ("segments_by_length", C.c_int32 * 8), ("reserved", C.c_int32)]


def record_dtype(record):
    """the numpy dtype of a Record: its fields at the structure's offsets (np.dtype(record) nests an array of arrays as a subarray of
    subarrays, which compares unequal to a field of shape (6, 6))"""
    formats = []
    for _, t in record._fields_:
        shape = ()
        while issubclass(t, C.Array):
            shape, t = shape + (t._length_,), t._type_
        formats.append((np.dtype(t), shape))
    names = [f for f, _ in record._fields_]
    return np.dtype(dict(names=names, formats=formats, offsets=[getattr(record, f).offset for f in names], itemsize=C.sizeof(record)))


CELL_DTYPE, SWEEP_RECORD_DTYPE, DRIFT_DTYPE = record_dtype(Cell), record_dtype(SweepRecord), record_dtype(Drift)
KEYFRAME_NODE_DTYPE, KEYFRAME_CELL_DTYPE = record_dtype(KeyframeNode), record_dtype(KeyframeCell)
KEYFRAME_EDGE_JOB_DTYPE, KEYFRAME_EDGE_DTYPE = record_dtype(KeyframeEdgeJob), record_dtype(KeyframeEdge)
PG_EDGE_DTYPE, PG_SUMMARY_DTYPE, SC_CANDIDATE_DTYPE = record_dtype(PgEdge), record_dtype(PgSummary), record_dtype(ScCandidate)

# ---- signatures: (result, arguments) of every export; the pointer names say what is behind a void* ----
_vp = _u8p = _u32p = _f32p = _f64p = _i32p = C.c_void_p
_int, _dbl, _P = C.c_int, C.c_double, C.POINTER
SIGNATURES = {
    "cfear_version": (C.c_char_p, []),
    "cfear_default_params": (None, [_P(Params)]),
    "cfear_create": (_int, [_P(_vp), _int, _vp, _P(Params), _int, _int]),
    "cfear_destroy": (None, [_vp]),
    "cfear_last_error": (C.c_char_p, [_vp]),
    "cfear_set_params": (_int, [_vp, _P(Params)]),
    "cfear_synchronize": (_int, [_vp]),
    "cfear_tune": (_int, [_vp, _int, _int]),
    "cfear_kstrongest_launch_shape": (_int, [_vp, _int, _P(_int), _P(_int), _P(_int)]),
    "cfear_kstrongest_device": (_int, [_vp, _u8p, _int, _u32p]),
    "cfear_kstrongest_host": (_int, [_vp, _u8p, _int, _u32p]),
    "cfear_rotate_polar": (_int, [_vp, _u8p, _int, _int, _u8p]),
    "cfear_rotate_polar_device": (_int, [_vp, _u8p, _int, _int, _int, _u8p]),
    "cfear_filter_polar": (_int, [_vp, _u8p, _P(_vp), _P(_vp)]),
    "cfear_filter_polar_device": (_int, [_vp, _u8p, _P(_vp), _P(_vp)]),
    "cfear_filter_cfar": (_int, [_vp, _u8p, _int, _int, C.c_float, _dbl, _P(_vp)]),
    "cfear_filter_cfar_device": (_int, [_vp, _u8p, _int, _int, C.c_float, _dbl, _P(_vp)]),
    "cfear_filter_cfar_batch_device": (_int, [_vp, _u8p, _int, _int, _int, C.c_float, _dbl, _f32p, _int, _i32p]),
    "cfear_filter_cfar_grid_device": (_int, [_vp, _u8p, _int, _vp, _i32p, _int, _dbl, _f32p, _int, _i32p]),
    "cfear_cfar_launch_plan": (_int, [_vp, _int, _int, C.c_float, _int, _P(CfarPlan)]),
    "cfear_cloud_upload": (_int, [_vp, _f32p, _int, _P(_vp)]),
    "cfear_cloud_size": (_int, [_vp, _vp, _P(_int)]),
    "cfear_cloud_download": (_int, [_vp, _vp, _f32p, _int, _P(_int)]),
    "cfear_clouds_download": (_int, [_vp, _P(_vp), _int, _P(_vp), _P(_int), _P(_int)]),
    "cfear_cloud_release": (None, [_vp, _vp]),
    "cfear_compensate": (_int, [_vp, _vp, _f64p, _int]),
    "cfear_compensate_pair": (_int, [_vp, _vp, _vp, _f64p, _int]),
    "cfear_scan_create": (_int, [_vp, _vp, _P(_vp)]),
    "cfear_scan_from_cells": (_int, [_vp, _vp, _int, _P(_vp)]),
    "cfear_scan_release": (None, [_vp, _vp]),
    "cfear_scan_size": (_int, [_vp, _vp, _P(_int)]),
    "cfear_scan_download_cells": (_int, [_vp, _vp, _vp, _int, _P(_int)]),
    "cfear_scan_closest": (_int, [_vp, _vp, _f64p, _int, _dbl, _i32p]),
    "cfear_register": (_int, [_vp, _P(_vp), _int, _f64p, _f64p, _P(RegSummary)]),
    "cfear_register_soft": (_int, [_vp, _P(_vp), _int, _f64p, _f64p, _f64p, _P(RegSummary)]),
    "cfear_register_time_continuous": (_int, [_vp, _P(_vp), _int, _f64p, _f64p, _int, _f64p, _f64p, _P(RegSummary)]),
    "cfear_get_cost": (_int, [_vp, _P(_vp), _int, _f64p, _int, _f64p, _f64p, _int, _P(_int)]),
    "cfear_cov_by_sampling": (_int, [_vp, _P(_vp), _int, _f64p, _int, _dbl, _dbl, _int, _dbl, _dbl, _int, _f64p, _P(_int), _f64p]),
    "cfear_odometry_create": (_int, [_vp, _int, _P(_vp)]),
    "cfear_odometry_destroy": (None, [_vp, _vp]),
    "cfear_odometry_reset": (_int, [_vp, _vp]),
    "cfear_odometry_step_device": (_int, [_vp, _vp, _u8p]),
    "cfear_odometry_step_host": (_int, [_vp, _vp, _u8p]),
    "cfear_odometry_step_cloud_device": (_int, [_vp, _vp, _f32p, _int, _i32p]),
    "cfear_odometry_poses": (_int, [_vp, _vp, _f64p]),
    "cfear_odometry_covariances": (_int, [_vp, _vp, _f64p]),
    "cfear_odometry_status": (_int, [_vp, _vp, _i32p]),
    "cfear_odometry_replay_host": (_int, [_vp, _vp, _u8p, _int, _vp]),
    "cfear_odometry_replay_device": (_int, [_vp, _vp, _u8p, _int, _vp]),
    "cfear_odometry_replay_host_cov": (_int, [_vp, _vp, _u8p, _int, _vp, _vp]),
    "cfear_odometry_replay_device_cov": (_int, [_vp, _vp, _u8p, _int, _vp, _vp]),
    "cfear_odometry_set_cov_sampling": (_int, [_vp, _vp, _int, _dbl, _dbl, _int, _dbl]),
    "cfear_odometry_cov_samples": (_int, [_vp, _vp, _int, _f64p, _vp]),
    "cfear_surface_dims": (_int, [_dbl, _int, _dbl, _dbl, _P(_int), _P(_int), _P(_int)]),
    "cfear_get_surface": (_int, [_vp, _P(_vp), _int, _f64p, _f64p, _int, _dbl, _int, _f64p, _P(_int), _P(_int)]),
    "cfear_odometry_set_surface_recording": (_int, [_vp, _vp, _int]),
    "cfear_odometry_surface": (_int, [_vp, _vp, _dbl, _int, _vp, _vp, _vp, _vp]),
    "cfear_odometry_set_sequence_params": (_int, [_vp, _vp, _vp, _int]),
    "cfear_odometry_sequence_params": (_int, [_vp, _vp, _int, _P(Params)]),
    "cfear_odometry_set_sequence_sources": (_int, [_vp, _vp, _i32p, _int, _int]),
    "cfear_odometry_set_sequence_shapes": (_int, [_vp, _vp, _vp, _int]),
    "cfear_odometry_sequence_shape": (_int, [_vp, _vp, _int, _P(SeqShape)]),
    "cfear_odometry_set_sequence_detectors": (_int, [_vp, _vp, _vp, _int, _i32p, _int]),
    "cfear_odometry_sequence_detector": (_int, [_vp, _vp, _int, _P(SeqDetector)]),
    "cfear_default_fuser_options": (None, [_P(FuserOptions)]),
    "cfear_odometry_set_fuser_options": (_int, [_vp, _vp, _vp, _int]),
    "cfear_odometry_fuser_options": (_int, [_vp, _vp, _int, _P(FuserOptions)]),
    "cfear_host_alloc": (_int, [_vp, C.c_size_t, _P(_vp)]),
    "cfear_host_free": (None, [_vp, _vp]),
    "cfear_odometry_summary": (_int, [_vp, _vp, _int, _P(RegSummary), _P(_int), _P(_int)]),
    "cfear_odometry_profile": (_int, [_vp, _vp, _int]),
    "cfear_odometry_profile_read": (_int, [_vp, _vp, _P(_dbl), _P(_int)]),
    "cfear_odometry_profile_read_stages": (_int, [_vp, _vp, _P(_dbl), _P(_dbl), _P(_int)]),
    "cfear_odometry_phase_times": (_int, [_vp, _vp, _int, _vp]),
    "cfear_time_kstrongest": (_int, [_vp, _u8p, _int, _u32p, _int, _int, _P(_dbl)]),
    "cfear_keyframe_constraint": (_int, [_f64p, _f64p, _f64p, _f64p, _f64p]),
    "cfear_odometry_set_keyframe_recording": (_int, [_vp, _vp, _int, _int, _int]),
    "cfear_odometry_keyframe_counts": (_int, [_vp, _vp, _i32p, _i32p]),
    "cfear_odometry_keyframe_nodes": (_int, [_vp, _vp, _int, _int, _vp, _int, _P(_int)]),
    "cfear_odometry_keyframe_cells": (_int, [_vp, _vp, _int, _int, _vp, _int, _P(_int)]),
    "cfear_odometry_keyframe_scans": (_int, [_vp, _vp, _int, _i32p, _int, _P(_vp)]),
    "cfear_odometry_keyframe_edges": (_int, [_vp, _vp, _vp, _int, _vp, _f64p, _vp]),
    "cfear_odometry_set_keyframe_clouds": (_int, [_vp, _vp, _int, _int]),
    "cfear_odometry_keyframe_cloud_sizes": (_int, [_vp, _vp, _int, _int, _i32p, _i32p, _int, _P(_int)]),
    "cfear_odometry_keyframe_cloud": (_int, [_vp, _vp, _int, _int, _int, _f32p, _int, _P(_int)]),
    "cfear_odometry_keyframe_clouds": (_int, [_vp, _vp, _int, _i32p, _int, _int, _P(_vp)]),
    "cfear_pg_default_options": (None, [_P(PgOptions)]),
    "cfear_pose_graph_optimize": (_int, [_vp, _int, _i32p, _i32p, _vp, _i32p, _P(PgOptions), _f64p, _vp]),
    "cfear_odometry_keyframe_optimize": (_int, [_vp, _vp, _vp, _int, _P(PgOptions), _f64p, _int, _i32p, _vp]),
    "cfear_pose_graph_cost_host": (_int, [_f64p, _int, _vp, _int, _int, _dbl, _P(_dbl), _P(C.c_int32), _P(C.c_int32)]),
    "cfear_sc_default_params": (None, [_P(ScParams)]),
    "cfear_scan_context_layout": (_int, [_P(ScParams), _f64p, _f64p]),
    "cfear_scan_context_describe": (_int, [_vp, _P(ScParams), _f32p, _i32p, _int, _u32p, _u32p, _i32p]),
    "cfear_scan_context_match": (_int, [_vp, _P(ScParams), _int, _i32p, _u32p, _vp, _int, _P(_int)]),
    "cfear_odometry_keyframe_descriptors": (_int, [_vp, _vp, _P(ScParams), _int, _int, _u32p, _u32p, _int, _P(_int)]),
    "cfear_odometry_keyframe_candidates": (_int, [_vp, _vp, _P(ScParams), _vp, _int, _P(_int)]),
    "cfear_drift_segments": (_int, [_f64p, _int, _i32p, _i32p, _i32p, _int, _P(_int)]),
    "cfear_drift_plan_create": (_int, [_vp, _f64p, _int, _P(_vp)]),
    "cfear_drift_plan_release": (None, [_vp, _vp]),
    "cfear_drift_device": (_int, [_vp, _vp, _vp, C.c_size_t, C.c_size_t, _int, _int, _vp]),
    "cfear_drift_host": (_int, [_vp, _vp, _vp, C.c_size_t, C.c_size_t, _int, _int, _vp]),
}
EXPORTS = list(SIGNATURES)


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
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)  # AttributeError if the ABI is incomplete (tests/test_abi_cpu.py checks every export)
        fn.restype = res
        fn.argtypes = args
    _LIB = L
    return L
