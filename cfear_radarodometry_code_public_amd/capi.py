"""ctypes binding of include/cfear_hip.h (no torch types cross this boundary): the objects and the host-only functions. abi.py holds what
mirrors the header - records, constants, signatures, the loader - and every public name of it is a name of this module too."""
import ctypes as C

import numpy as np

from .abi import *  # noqa: F401,F403


def _with_fields(record, defaults_fn, kw):
    """a record as the library's defaults_fn fills it, with the fields named in kw replaced"""
    r = record()
    getattr(lib(), defaults_fn)(C.byref(r))
    for k, v in kw.items():
        if k == "pad_" or not hasattr(r, k):
            raise AttributeError(k)
        setattr(r, k, v)
    return r


def default_params(**kw):
    return _with_fields(Params, "cfear_default_params", kw)


def default_fuser_options(**kw):
    return _with_fields(FuserOptions, "cfear_default_fuser_options", kw)


def pg_options(**kw):
    """cfear_pg_default_options with fields replaced: max_iterations (50), max_linear_iterations (0 = 30 x nodes), linear_tolerance (1e-8),
    function_tolerance (1e-12), parameter_tolerance (1e-10), initial_damping (1e-4), loss (LOSS_NONE), loss_limit (0.1)"""
    return _with_fields(PgOptions, "cfear_pg_default_options", kw)


def sc_params(**kw):
    """cfear_sc_default_params with fields replaced: n_rings (20), n_sectors (60), max_range (80 m), value (SC_MAX), source (0 = the filtered
    cloud, 1 = the peaks cloud; the log routes), min_index_gap (6), n_keys (10; 0 = exhaustive), max_per_node (1), max_distance (0.4)"""
    return _with_fields(ScParams, "cfear_sc_default_params", kw)


def detector_array(dets):
    """a list of SeqDetector / (window_size, nb_guard_cells, false_alarm_rate, z_min) tuples -> a ctypes array of SeqDetector (handed on as it
    is when it already is one: a caller that repeats a large grid builds it once)"""
    if isinstance(dets, C.Array) and dets._type_ is SeqDetector:
        return dets
    dets = [d if isinstance(d, SeqDetector) else SeqDetector(int(d[0]), int(d[1]), float(d[2]), float(d[3])) for d in dets]
    return (SeqDetector * len(dets))(*dets)


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


def pose_graph_cost_host(poses, edges, loss=0, loss_limit=0.1):
    """cfear_pose_graph_cost_host (host only, no device): F of one graph at poses [n, 3] -> (cost, edges used, edges skipped)"""
    x = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    E = np.ascontiguousarray(edges, dtype=PG_EDGE_DTYPE).reshape(-1)
    cost, used, skipped = C.c_double(), C.c_int32(), C.c_int32()
    rc = lib().cfear_pose_graph_cost_host(x.ctypes.data, len(x), E.ctypes.data, len(E), int(loss), float(loss_limit), C.byref(cost), C.byref(used), C.byref(skipped))
    if rc != 0:
        raise CfearError("cfear_pose_graph_cost_host failed rc=%d" % rc)
    return cost.value, used.value, skipped.value


def scan_context_layout(params=None, **kw):
    """cfear_scan_context_layout (host only, no device): the table the kernels read -> (ring_edge2 [n_rings + 1], sector_dir [n_sectors, 2])"""
    p = params if params is not None else sc_params(**kw)
    edge, sdir = np.zeros(max(int(p.n_rings), 0) + 1), np.zeros((max(int(p.n_sectors), 1), 2))
    rc = lib().cfear_scan_context_layout(C.byref(p), edge.ctypes.data, sdir.ctypes.data)
    if rc != 0:
        raise CfearError("cfear_scan_context_layout failed rc=%d (%r)" % (rc, p))
    return edge, sdir


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


def _count_then_fill(call, head, *outs):
    """The ABI's two-step read, `call(*head, outputs ..., capacity, &n)`: null outputs with capacity 0 answer the count, then arrays of
    that length (allocated with at least one element) are filled. outs: (dtype, trailing shape) of each output -> the list of arrays."""
    n = C.c_int()
    call(*head, *[None] * len(outs), 0, C.byref(n))
    arrs = [np.zeros((max(n.value, 1),) + tuple(shape), dtype=dt) for dt, shape in outs]
    call(*head, *[a.ctypes.data for a in arrs], n.value, C.byref(n))
    return [a[:n.value] for a in arrs]


def _gt34(gt):
    """ground-truth poses [n, 4, 4] or [n, 3, 4] (or [n, 12]) -> contiguous [n, 12] doubles, the 3x4 row-major form of a KITTI line"""
    g = np.asarray(gt, dtype=np.float64)
    g = g.reshape(len(g), -1, 4)[:, :3, :] if g.ndim == 3 else g.reshape(len(g), 3, 4)
    return np.ascontiguousarray(g).reshape(len(g), 12)


def drift_segments(gt):
    """cfear_drift_segments (host only, no device): the (first, last, length index) triples of the KITTI drift metric for the ground
    truth gt, in the metric's order -> int32 array [m, 3] (kitti.segments is the numpy statement)"""
    g = _gt34(gt)

    def call(first, last, length, capacity, m):
        rc = lib().cfear_drift_segments(g.ctypes.data, len(g), first, last, length, capacity, m)
        if rc != 0 and (rc != ERR_CAPACITY or capacity):  # (CFEAR_ERR_CAPACITY with the count is the answer to capacity 0)
            raise CfearError("cfear_drift_segments failed rc=%d" % rc)
    return np.stack(_count_then_fill(call, (), (np.int32, ()), (np.int32, ()), (np.int32, ())), axis=1)


def _addr(a):
    """Device pointer (int), torch tensor (data_ptr) or numpy array -> address."""
    if isinstance(a, int):
        return a
    if hasattr(a, "data_ptr"):
        return a.data_ptr()
    return a.ctypes.data


def _scans_poses(scans, poses):
    """what the registration entries take -> (n, the scans' handles as a C array, a copy of the poses as [n, 3] doubles)"""
    n = len(scans)
    return n, (C.c_void_p * n)(*[s._h for s in scans]), np.ascontiguousarray(poses, dtype=np.float64).reshape(n, 3).copy()


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

    def _call(self, name, *args):
        """the library's `name` on this context; raises CfearError with that name and the library's message unless it returns 0"""
        self._check(getattr(self._L, name)(self._h, *args), name)

    @property
    def handle(self):
        return self._h

    def set_params(self, params):
        self._call("cfear_set_params", C.byref(params))
        self.params = params

    def synchronize(self):
        self._call("cfear_synchronize")

    def tune(self, key, value):
        """cfear_tune (include/cfear_hip.h): launch-shape knobs - TUNE_FILTER_OCCUPANCY, TUNE_FILTER_ROWS_PER_WAVE, TUNE_ODOMETRY_OVERLAP,
        TUNE_FILTER_CUS, TUNE_REPLAY_PERSISTENT_MAX, TUNE_REPEAT_SHORTCUT, TUNE_REGISTRATION_ORDER: results do not depend on them -,
        TUNE_FILTER_PEAKS (-1 automatic, 1 / 0: the filter always / never computes the slots' peak flag, bit 25) and
        TUNE_MAX_CELLS, the cell capacity batched odometry objects created afterwards are sized for (an overflow is reported, never silent)"""
        self._call("cfear_tune", int(key), int(value))
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
        self._call("cfear_kstrongest_launch_shape", int(n_scans), C.byref(rows), C.byref(wgs), C.byref(occ))
        return rows.value, wgs.value, occ.value

    def kstrongest_host(self, polar):
        polar = np.ascontiguousarray(polar, dtype=np.uint8)
        if polar.ndim == 2:
            polar = polar[None]
        n, A, R = polar.shape
        assert (A, R) == (self.A, self.R)
        out = np.zeros((n, A, self.params.k_strongest), dtype=np.uint32)
        self._call("cfear_kstrongest_host", polar.ctypes.data, n, out.ctypes.data)
        return out

    def kstrongest_device(self, d_polar, n_scans, d_slots):
        self._call("cfear_kstrongest_device", _addr(d_polar), int(n_scans), _addr(d_slots))

    def time_kstrongest(self, d_polar, n_scans, d_slots, warmup, iters):
        t = C.c_double()
        self._call("cfear_time_kstrongest", _addr(d_polar), int(n_scans), _addr(d_slots), int(warmup), int(iters), C.byref(t))
        return t.value

    def rotate_polar(self, img):
        """radarDriver::Callback (non-Oxford): rows = range -> rows = azimuth (cv::ROTATE_90_COUNTERCLOCKWISE)"""
        img = np.ascontiguousarray(img, dtype=np.uint8)
        out = np.empty((img.shape[1], img.shape[0]), dtype=np.uint8)
        self._call("cfear_rotate_polar", img.ctypes.data, img.shape[0], img.shape[1], out.ctypes.data)
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
        self._call("cfear_cfar_launch_plan", int(window_size), int(nb_guard_cells), C.c_float(false_alarm_rate), int(n_scans), C.byref(p))
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
        self._call("cfear_filter_cfar_grid_device", _addr(d_polar), int(n_sources), C.cast(arr, C.c_void_p), src.ctypes.data if src is not None else None,
                   len(arr), float(max_distance), _addr(d_xyi), int(capacity), _addr(d_counts))

    def filter_cfar_batch(self, d_polar, n_scans, d_xyi, capacity, d_counts, window_size=10, nb_guard_cells=20, false_alarm_rate=0.01, max_distance=400.0):
        """CA-CFAR over n_scans device-resident sweeps; d_xyi [n_scans, capacity, 3] float32 and d_counts [n_scans] int32 on the device"""
        self._call("cfear_filter_cfar_batch_device", _addr(d_polar), int(n_scans), int(window_size), int(nb_guard_cells), C.c_float(false_alarm_rate),
                   C.c_double(max_distance), _addr(d_xyi), int(capacity), _addr(d_counts))

    def cloud_upload(self, xyi):
        xyi = np.ascontiguousarray(xyi, dtype=np.float32).reshape(-1, 3)
        c = C.c_void_p()
        self._call("cfear_cloud_upload", xyi.ctypes.data, xyi.shape[0], C.byref(c))
        return Cloud(self, c)

    def compensate(self, cloud, motion_xyt, ccw):
        m = np.asarray(motion_xyt, dtype=np.float64).copy()
        self._call("cfear_compensate", cloud._h, m.ctypes.data, int(ccw))

    def compensate_pair(self, cloud, cloud_peaks, motion_xyt, ccw):
        """cfear_compensate_pair: a sweep's two clouds by the same motion in one launch (odometrykeyframefuser.cpp:148-149)"""
        m = np.asarray(motion_xyt, dtype=np.float64).copy()
        self._call("cfear_compensate_pair", cloud._h, cloud_peaks._h, m.ctypes.data, int(ccw))

    # ---- stage 2 (MapPointNormal) ----
    def scan_create(self, cloud):
        s = C.c_void_p()
        self._call("cfear_scan_create", cloud._h, C.byref(s))
        return Scan(self, s)

    def scan_from_cells(self, cells):
        """cells: numpy array of CELL_DTYPE (raw = true identity cells, transformed copies) -> Scan"""
        cells = np.ascontiguousarray(cells, dtype=CELL_DTYPE)
        s = C.c_void_p()
        self._call("cfear_scan_from_cells", cells.ctypes.data, len(cells), C.byref(s))
        return Scan(self, s)

    # ---- stage 3 (n_scan_normal_reg::Register) ----
    def register(self, scans, poses):
        n, arr, P = _scans_poses(scans, poses)
        cov = np.zeros(36)
        S = RegSummary()
        self._call("cfear_register", arr, n, P.ctypes.data, cov.ctypes.data, C.byref(S))
        return bool(S.success), P, cov.reshape(6, 6), S

    def register_soft(self, scans, poses, prior_cov6):
        """Register(..., soft_constraints=true) with reg_cov.back() = prior_cov6"""
        n, arr, P = _scans_poses(scans, poses)
        pc = np.ascontiguousarray(prior_cov6, dtype=np.float64).reshape(36).copy()
        cov = np.zeros(36)
        S = RegSummary()
        self._call("cfear_register_soft", arr, n, P.ctypes.data, pc.ctypes.data, cov.ctypes.data, C.byref(S))
        return bool(S.success), P, cov.reshape(6, 6), S

    def register_time_continuous(self, scans, poses, velocity, ccw=False, prior_cov6=None):
        """RegisterTimeContinuous(scans, Tsrc, reg_cov, Tvel, soft_constraints, ccw) (n_scan_normal.cpp:67-80): the last scan keeps its
        motion distortion; velocity = (vx, vy, vtheta) over one sweep = Affine3dToVectorXYeZ(Tvel); prior_cov6: reg_cov.back() with
        soft_constraints, None: without. Returns what register returns."""
        n, arr, P = _scans_poses(scans, poses)
        v = np.ascontiguousarray(velocity, dtype=np.float64).reshape(3).copy()
        pc = None if prior_cov6 is None else np.ascontiguousarray(prior_cov6, dtype=np.float64).reshape(36).copy()
        cov = np.zeros(36)
        S = RegSummary()
        self._call("cfear_register_time_continuous", arr, n, P.ctypes.data, v.ctypes.data, int(bool(ccw)), None if pc is None else pc.ctypes.data, cov.ctypes.data, C.byref(S))
        return bool(S.success), P, cov.reshape(6, 6), S

    def get_cost(self, scans, poses, itr=2):
        """n_scan_normal_reg::GetCost -> (score, residuals) or None where the reference returns false."""
        n, arr, P = _scans_poses(scans, poses)
        cap = 2 * (n - 1) * max(scans[-1].size, 1)
        res = np.zeros(cap)
        score, m = C.c_double(), C.c_int()
        rc = self._L.cfear_get_cost(self._h, arr, n, P.ctypes.data, int(itr), C.byref(score), res.ctypes.data, cap, C.byref(m))
        if rc == ERR_EMPTY:
            return None
        self._check(rc, "cfear_get_cost")
        return score.value, res[:m.value].copy()

    def get_surface(self, scans, poses, res, width, itr=2, prior_cov6=None):
        """n_scan_normal_reg::GetSurface (n_scan_normal.cpp:29-65) -> (pixels, pixels) array, row i = x, column j = y; NaN in the
        cells the reference's loops never reach. prior_cov6: reg_cov.back() with soft_constraints, None: without."""
        n, arr, P = _scans_poses(scans, poses)
        pixels = surface_dims(res, width, P[-1, 0], P[-1, 1])[0]
        out = np.empty((pixels, pixels))
        pc = None if prior_cov6 is None else np.ascontiguousarray(prior_cov6, dtype=np.float64).reshape(36).copy()
        nx, ny = C.c_int(), C.c_int()
        self._call("cfear_get_surface", arr, n, P.ctypes.data, None if pc is None else pc.ctypes.data, int(itr), float(res), int(width), out.ctypes.data, C.byref(nx), C.byref(ny))
        return out

    def cov_by_sampling(self, scans, poses, final_cost, num_residuals, itr=2, xy_range=0.4, yaw_range=0.0043625, steps=3, cov_scaler=4.0):
        """approximateCovarianceBySampling -> (success, cov6x6, sampled costs)"""
        n, arr, P = _scans_poses(scans, poses)
        cov, costs, ok = np.zeros(36), np.zeros(steps ** 3), C.c_int()
        self._call("cfear_cov_by_sampling", arr, n, P.ctypes.data, int(itr), float(xy_range), float(yaw_range), int(steps), float(cov_scaler),
                   float(final_cost), int(num_residuals), cov.ctypes.data, C.byref(ok), costs.ctypes.data)
        return bool(ok.value), cov.reshape(6, 6), costs

    def pinned(self, shape, dtype=np.uint8):
        """Page-locked host array (cfear_host_alloc): copies from it overlap with kernels. Freed by pinned_free(arr) - arr or any
        view / slice of it - or when the context closes: the array and its views must not be touched after either (the memory is
        gone; NumPy cannot know)."""
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        ptr = C.c_void_p()
        self._call("cfear_host_alloc", nbytes, C.byref(ptr))
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
        self._call("cfear_drift_plan_create", g.ctypes.data, len(g), C.byref(h))
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
        self._call("cfear_pose_graph_optimize", len(P), noff.ctypes.data, eoff.ctypes.data, ed.ctypes.data if len(ed) else None,
                   fx.ctypes.data if fx is not None else None, C.byref(opt), x.ctypes.data if len(x) else None, sums.ctypes.data)
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
        self._call("cfear_scan_context_describe", C.byref(p), xyi.ctypes.data if len(xyi) else None, off.ctypes.data, m,
                   bins.ctypes.data if m else None, ring.ctypes.data if m else None, drop.ctypes.data if m else None)
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
        self._call("cfear_scan_context_match", C.byref(p), len(S), off.ctypes.data, bins.ctypes.data if len(bins) else None, out.ctypes.data, cap, C.byref(n))
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


class _Handle:
    """an object of the library that lives in a context: the context, the handle, and the entry that releases it"""
    _release = None

    def __init__(self, ctx, h):
        self._ctx, self._h = ctx, h

    def release(self):
        if self._h and self._ctx._h:
            getattr(self._ctx._L, self._release)(self._ctx._h, self._h)
        self._h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def _call(self, name, *args):
        """the library's `name` on this object of its context; raises as Context._call does"""
        c = self._ctx
        c._check(getattr(c._L, name)(c._h, self._h, *args), name)

    def _read(self, name, head, *outs):
        return _count_then_fill(lambda *a: self._call(name, *a), head, *outs)


class Cloud(_Handle):
    _release = "cfear_cloud_release"

    @property
    def size(self):
        n = C.c_int()
        self._call("cfear_cloud_size", C.byref(n))
        return n.value

    def download(self):
        n = self.size
        out = np.zeros((max(n, 1), 3), dtype=np.float32)
        m = C.c_int()
        self._call("cfear_cloud_download", out.ctypes.data, n, C.byref(m))
        return out[:n]


class Scan(_Handle):
    _release = "cfear_scan_release"

    @property
    def size(self):
        n = C.c_int()
        self._call("cfear_scan_size", C.byref(n))
        return n.value

    def cells(self):
        n = self.size
        out = np.zeros(max(n, 1), dtype=CELL_DTYPE)
        m = C.c_int()
        self._call("cfear_scan_download_cells", out.ctypes.data, n, C.byref(m))
        return out[:n]

    def closest(self, qxy, d):
        q = np.ascontiguousarray(qxy, dtype=np.float64).reshape(-1, 2)
        idx = np.zeros(q.shape[0], dtype=np.int32)
        self._call("cfear_scan_closest", q.ctypes.data, q.shape[0], float(d), idx.ctypes.data)
        return idx


class DriftPlan(_Handle):
    """cfear_drift_plan: one ground truth, ready to score batches of trajectories on the device (Context.drift_plan)"""
    _release = "cfear_drift_plan_release"

    def __init__(self, ctx, h, n_gt):
        _Handle.__init__(self, ctx, h)
        self.n_gt = int(n_gt)

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
            self._call("cfear_drift_host", a.ctypes.data, B * seq, seq, n, B, res.ctypes.data)
            return res
        if n_sweeps is None or n_sequences is None:
            raise ValueError("DriftPlan.score: a device buffer needs n_sweeps and n_sequences")
        B = int(n_sequences)
        seq = SWEEP_RECORD_DTYPE.itemsize if seq_stride is None else int(seq_stride)
        sweep = B * seq if sweep_stride is None else int(sweep_stride)
        if out is not None:
            self._call("cfear_drift_device", _addr(poses), sweep, seq, int(n_sweeps), B, _addr(out))
            return None
        import torch
        d_out = torch.empty(B * DRIFT_DTYPE.itemsize, dtype=torch.uint8, device="cuda:%d" % c.device)
        torch.cuda.synchronize(d_out.device)  # (the allocator's stream may still use the memory; the context stream writes it)
        self._call("cfear_drift_device", _addr(poses), sweep, seq, int(n_sweeps), B, d_out.data_ptr())
        c.synchronize()
        return d_out.cpu().numpy().view(DRIFT_DTYPE).copy()


class Odometry(_Handle):
    """Batched OdometryKeyframeFuser: B independent sequences, all state on the device."""
    _release = "cfear_odometry_destroy"

    def __init__(self, ctx, n_sequences):
        _Handle.__init__(self, ctx, C.c_void_p())
        self.B = int(n_sequences)
        self.n_sources = self.B  # input sweeps per step (set_sequence_sources)
        ctx._call("cfear_odometry_create", self.B, C.byref(self._h))

    def reset(self):
        self._call("cfear_odometry_reset")

    def step_device(self, d_polar):
        self._call("cfear_odometry_step_device", _addr(d_polar))

    def step_cloud_device(self, d_xyi, capacity, d_counts):
        """clouds on the device (raw pointers): [B][capacity][3] floats, [B] int32 counts"""
        self._call("cfear_odometry_step_cloud_device", C.c_void_p(int(d_xyi)), int(capacity), C.c_void_p(int(d_counts)))

    def step_host(self, polar):
        polar = np.ascontiguousarray(polar, dtype=np.uint8)
        assert polar.shape == (self.n_sources, self._ctx.A, self._ctx.R), polar.shape
        self._call("cfear_odometry_step_host", polar.ctypes.data)

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
            self._call("cfear_odometry_replay_host", frames.ctypes.data, n, rec.ctypes.data if records else None)
            return rec
        cov = np.zeros((n, self.B, 36))
        self._call("cfear_odometry_replay_host_cov", frames.ctypes.data, n, rec.ctypes.data if records else None, cov.ctypes.data)
        return rec, cov.reshape(n, self.B, 6, 6)

    def replay_device(self, d_frames, n_sweeps, d_records=None, d_cov=None):
        """d_frames: device pointer / torch tensor of n_sweeps x B x A x R bytes; d_records: device buffer of n_sweeps x B x 80 bytes or
        None; d_cov: device buffer of n_sweeps x B x 36 doubles (cov_current after every sweep) or None. Asynchronous on the context stream."""
        rec = _addr(d_records) if d_records is not None else None
        if d_cov is None:
            self._call("cfear_odometry_replay_device", _addr(d_frames), int(n_sweeps), rec)
        else:
            self._call("cfear_odometry_replay_device_cov", _addr(d_frames), int(n_sweeps), rec, _addr(d_cov))

    def set_sequence_params(self, rows):
        """rows: one Params per sequence (the points of a parameter grid, utils/worker:26-99; replay.param_grid builds them), or None for
        the context's parameters again (cfear_odometry_set_sequence_params). Before the first sweep since creation / reset()."""
        if rows is None:
            self._call("cfear_odometry_set_sequence_params", None, 0)
            return
        rows = list(rows)
        arr = (Params * len(rows))(*rows)
        self._call("cfear_odometry_set_sequence_params", C.cast(arr, C.c_void_p), len(rows))

    def sequence_params(self, q):
        """the Params sequence q runs with (cfear_odometry_sequence_params)"""
        p = Params()
        self._call("cfear_odometry_sequence_params", int(q), C.byref(p))
        return p

    def set_sequence_sources(self, source, n_sources=None):
        """source[q]: the input sweep sequence q reads; afterwards step_host / step_device / the replays take n_sources sweeps per step
        instead of B. None: one sweep per sequence again (cfear_odometry_set_sequence_sources)."""
        if source is None:
            self._call("cfear_odometry_set_sequence_sources", None, 0, 0)
            self.n_sources = self.B
            return
        src = np.ascontiguousarray(source, dtype=np.int32)
        ns = int(n_sources) if n_sources is not None else int(src.max()) + 1
        self._call("cfear_odometry_set_sequence_sources", src.ctypes.data, int(src.size), ns)
        self.n_sources = ns

    def set_sequence_shapes(self, shapes):
        """shapes: one SeqShape (or (cost, submap_scan_size) pair) per sequence - the cost metric and the submap size it runs with, any
        submap_scan_size up to the context's - or None for the context's values again (cfear_odometry_set_sequence_shapes). Before the first
        sweep since creation / reset(), and before a parameter table whose rows carry these values."""
        if shapes is None:
            self._call("cfear_odometry_set_sequence_shapes", None, 0)
            return
        shapes = [s if isinstance(s, SeqShape) else SeqShape(int(s[0]), int(s[1])) for s in shapes]
        arr = (SeqShape * len(shapes))(*shapes)
        self._call("cfear_odometry_set_sequence_shapes", C.cast(arr, C.c_void_p), len(shapes))

    def sequence_shape(self, q):
        """the SeqShape sequence q runs with (cfear_odometry_sequence_shape)"""
        s = SeqShape()
        self._call("cfear_odometry_sequence_shape", int(q), C.byref(s))
        return s

    def set_sequence_detectors(self, dets, source=None, n_sources=None):
        """dets: one SeqDetector (or (window_size, nb_guard_cells, false_alarm_rate, z_min) tuple) per sequence of a filter_type CA-CFAR
        object; source[q]: the input sweep sequence q reads (None: one sweep per sequence) - afterwards step_host / step_device / the
        replays take n_sources sweeps per step, staged once each, every distinct (sweep, detector) decided once. dets None: the
        context's detector and one sweep per sequence again (cfear_odometry_set_sequence_detectors). Before the first sweep since
        creation / reset()."""
        if dets is None:
            self._call("cfear_odometry_set_sequence_detectors", None, 0, None, 0)
            self.n_sources = self.B
            return
        arr = detector_array(dets)
        if source is None:
            self._call("cfear_odometry_set_sequence_detectors", C.cast(arr, C.c_void_p), len(arr), None, 0)
            self.n_sources = self.B
            return
        src = np.ascontiguousarray(source, dtype=np.int32)
        ns = int(n_sources) if n_sources is not None else int(src.max()) + 1
        if src.size != len(arr):
            raise ValueError("set_sequence_detectors: %d detectors, %d sources" % (len(arr), src.size))
        self._call("cfear_odometry_set_sequence_detectors", C.cast(arr, C.c_void_p), len(arr), src.ctypes.data, ns)
        self.n_sources = ns

    def sequence_detector(self, q):
        """the SeqDetector sequence q runs with (cfear_odometry_sequence_detector)"""
        d = SeqDetector()
        self._call("cfear_odometry_sequence_detector", int(q), C.byref(d))
        return d

    def set_fuser_options(self, rows):
        """rows: one FuserOptions for every sequence, a list of one per sequence, or None for the defaults again
        (cfear_odometry_set_fuser_options). Before the first sweep since creation / reset()."""
        if rows is None:
            self._call("cfear_odometry_set_fuser_options", None, 0)
            return
        rows = [rows] if isinstance(rows, FuserOptions) else list(rows)
        arr = (FuserOptions * len(rows))(*rows)
        self._call("cfear_odometry_set_fuser_options", C.cast(arr, C.c_void_p), len(rows))

    def fuser_options(self, q):
        """the FuserOptions sequence q runs with (cfear_odometry_fuser_options)"""
        o = FuserOptions()
        self._call("cfear_odometry_fuser_options", int(q), C.byref(o))
        return o

    def set_cov_sampling(self, enable=True, xy_range=0.4, yaw_range=0.0043625, samples_per_axis=3, covariance_scaler=4.0):
        """estimate_cov_by_sampling and its companions (odometrykeyframefuser.h:104-110) for every sequence, from the next sweep on"""
        self._call("cfear_odometry_set_cov_sampling", int(bool(enable)), float(xy_range), float(yaw_range), int(samples_per_axis), float(covariance_scaler))
        if enable:
            self._cov_m = int(samples_per_axis) ** 3

    def cov_samples(self, sequence):
        """the last sweep's sampled costs of one sequence (samples_per_axis^3, the reference's order) and whether the sampled
        covariance was used -> (costs, sampled)"""
        costs = np.zeros(getattr(self, "_cov_m", 1))
        ok = C.c_int()
        self._call("cfear_odometry_cov_samples", int(sequence), costs.ctypes.data, C.byref(ok))
        return costs, bool(ok.value)

    def set_surface_recording(self, enable=True):
        """every registration records what it used, for surface() (cfear_odometry_set_surface_recording); off by default"""
        self._call("cfear_odometry_set_surface_recording", int(bool(enable)))

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
        self._call("cfear_odometry_surface", float(res), int(width), out.data_ptr(), n_used.ctypes.data, itr_used.ctypes.data, poses_used.ctypes.data)
        self._ctx.synchronize()
        return (out, n_used, itr_used, poses_used) if details else out

    def profile(self, enable):
        self._call("cfear_odometry_profile", int(enable))

    def profile_read(self):
        """-> (filter seconds, filter launches)"""
        tf, nf = C.c_double(), C.c_int()
        self._call("cfear_odometry_profile_read", C.byref(tf), C.byref(nf))
        return tf.value, nf.value

    def profile_read_stages(self):
        """-> (features seconds, registration seconds, launches of each)"""
        tf, tr, n = C.c_double(), C.c_double(), C.c_int()
        self._call("cfear_odometry_profile_read_stages", C.byref(tf), C.byref(tr), C.byref(n))
        return tf.value, tr.value, n.value

    def phase_times(self, mode, light=False, workgroups_only=False, controller=False):
        """None: switch to the timed kernel instantiations (light: phase stamps only, without the per-LM-command clock reads that
        halve the speed of the registration kernel; workgroups_only: production kernels, start / end clock per workgroup; controller: slots 0..7 of a sequence hold the
        breakdown of the registration's command loop instead of the feature kernel's stamps); True: read + clear the [B][32] tick table of the steps since the last read;
        False: back to the production kernels."""
        if mode is None:
            self._call("cfear_odometry_phase_times", 3 if workgroups_only else (4 if controller else (2 if light else 1)), None)
            return None
        if mode is False:
            self._call("cfear_odometry_phase_times", 0, None)
            return None
        buf = np.zeros((self.B, 32), dtype=np.int64)
        self._call("cfear_odometry_phase_times", -1, buf.ctypes.data)
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
        self._call("cfear_odometry_set_keyframe_recording", what & ~(KF_CLOUD | KF_PEAKS), int(max_keyframes), int(max_cells))
        if what & KF_CLOUD:
            self.record_keyframe_clouds(what & (KF_CLOUD | KF_PEAKS), max_points)

    def record_keyframe_clouds(self, what=KF_CLOUD | KF_PEAKS, max_points=0):
        """cfear_odometry_set_keyframe_clouds on an object whose node recording is on: what = 0 (off, at any time), KF_CLOUD or KF_CLOUD | KF_PEAKS"""
        self._call("cfear_odometry_set_keyframe_clouds", int(what), int(max_points))

    def keyframe_counts(self):
        """-> (recorded [B], dropped [B]) keyframes per sequence"""
        rec, drop = np.zeros(self.B, dtype=np.int32), np.zeros(self.B, dtype=np.int32)
        self._call("cfear_odometry_keyframe_counts", rec.ctypes.data, drop.ctypes.data)
        return rec, drop

    def keyframes(self, q):
        """the recorded nodes of sequence q -> structured array of KEYFRAME_NODE_DTYPE"""
        return self._read("cfear_odometry_keyframe_nodes", (int(q), 0), (KEYFRAME_NODE_DTYPE, ()))[0]

    def keyframe_cells(self, q, i):
        """the cells of keyframe i of sequence q, in the scan's order -> structured array of KEYFRAME_CELL_DTYPE"""
        return self._read("cfear_odometry_keyframe_cells", (int(q), int(i)), (KEYFRAME_CELL_DTYPE, ()))[0]

    def keyframe_scans(self, q, indices):
        """per-call Scans rebuilt from the recorded keyframes `indices` of sequence q in one launch (cfear_odometry_keyframe_scans): ready for
        Context.register / get_cost; their downloadable cells carry intensities 0. -> list of Scan"""
        idx = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1)
        arr = (C.c_void_p * len(idx))()
        self._call("cfear_odometry_keyframe_scans", int(q), idx.ctypes.data, len(idx), arr)
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
        self._call("cfear_odometry_keyframe_edges", J.ctypes.data, m, edges.ctypes.data, cov.ctypes.data if details else None, sums if details else None)
        return (edges, cov, [sums[i] for i in range(m)]) if details else edges

    def keyframe_optimize(self, edges=None, options=None, **kw):
        """cfear_odometry_keyframe_optimize: the graphs of the log, one per sequence, optimised in one launch - the chain and the initial
        poses are read from the recorded nodes on the device, edges (KEYFRAME_EDGE_DTYPE, as keyframe_edges returned them; any sequences,
        any order; those without success are left out) join them under the options' loss. options: a PgOptions, or its fields as keywords.
        -> (per sequence an array [n_q, 3] of optimised poses, summaries: PG_SUMMARY_DTYPE [B]). Nothing is written to the log."""
        E = np.zeros(0, dtype=KEYFRAME_EDGE_DTYPE) if edges is None else np.ascontiguousarray(edges, dtype=KEYFRAME_EDGE_DTYPE).reshape(-1)
        opt = options if options is not None else pg_options(**kw)
        off = np.zeros(self.B + 1, dtype=np.int32)
        ep = E.ctypes.data if len(E) else None
        self._call("cfear_odometry_keyframe_optimize", ep, len(E), C.byref(opt), None, 0, off.ctypes.data, None)
        x = np.zeros((max(int(off[-1]), 1), 3))
        sums = np.zeros(self.B, dtype=PG_SUMMARY_DTYPE)
        self._call("cfear_odometry_keyframe_optimize", ep, len(E), C.byref(opt), x.ctypes.data, int(off[-1]), off.ctypes.data, sums.ctypes.data)
        return [x[off[q]:off[q + 1]].copy() for q in range(self.B)], sums

    def keyframe_descriptors(self, q, params=None, **kw):
        """cfear_odometry_keyframe_descriptors: the Scan-Context descriptors of every recorded keyframe, from the point log on the device in
        one launch; those of sequence q come back -> (bins uint32 [n, n_sectors, n_rings], ring_sums uint32 [n, n_rings]). params: a ScParams,
        or its fields as keywords (source=1: of the peaks clouds). Needs a log with KF_CLOUD. Nothing is written to the log."""
        p = params if params is not None else sc_params(**kw)
        return tuple(self._read("cfear_odometry_keyframe_descriptors", (C.byref(p), int(q), 0),
                                (np.uint32, (int(p.n_sectors), int(p.n_rings))), (np.uint32, (int(p.n_rings),))))

    def keyframe_candidates(self, params=None, **kw):
        """cfear_odometry_keyframe_candidates: loop candidates by appearance for every sequence of the object - describe and match on the
        device, no cloud or descriptor comes to the host -> SC_CANDIDATE_DTYPE, (sequence, to, distance) ascending (replay.appearance_jobs
        turns a sequence's into keyframe_edges jobs). Nothing is written to the log."""
        p = params if params is not None else sc_params(**kw)
        cap = int(self.keyframe_counts()[0].sum()) * int(p.max_per_node)
        out = np.zeros(max(cap, 1), dtype=SC_CANDIDATE_DTYPE)
        n = C.c_int()
        self._call("cfear_odometry_keyframe_candidates", C.byref(p), out.ctypes.data, cap, C.byref(n))
        return out[:n.value].copy()

    def keyframe_cloud_sizes(self, q):
        """-> (n_cloud [n], n_peaks [n]): points of the filtered and of the peaks cloud of every recorded node of sequence q"""
        return tuple(self._read("cfear_odometry_keyframe_cloud_sizes", (int(q), 0), (np.int32, ()), (np.int32, ())))

    def keyframe_cloud(self, q, i, peaks=False):
        """the filtered (peaks=True: the peaks) cloud of keyframe i of sequence q -> float32 [n, 3]: x, y, intensity"""
        return self._read("cfear_odometry_keyframe_cloud", (int(q), int(i), int(bool(peaks))), (np.float32, (3,)))[0]

    def keyframe_clouds(self, q, indices, peaks=False):
        """the recorded clouds of keyframes `indices` of sequence q as device Clouds (cfear_odometry_keyframe_clouds): ready for
        Context.scan_create at any res, Cloud.download. -> list of Cloud"""
        idx = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1)
        arr = (C.c_void_p * len(idx))()
        self._call("cfear_odometry_keyframe_clouds", int(q), idx.ctypes.data, len(idx), int(bool(peaks)), arr)
        return [Cloud(self._ctx, C.c_void_p(h)) for h in arr]

    def poses(self):
        out = np.zeros((self.B, 3))
        self._call("cfear_odometry_poses", out.ctypes.data)
        return out

    def status(self, per_sequence=False):
        """raises CfearError (rc=-6) if a scan of this object was truncated (cfear_odometry_status); per_sequence=True: returns the per-sequence
        flag words instead of raising (bit 0 = STATUS_CELLS_LOST, bit 1 = STATUS_POINTS_LOST, bit 2 = STATUS_KEYFRAMES_DROPPED: the sequence's keyframe
        log is full - no error of the odometry, the call does not raise for it)"""
        if not per_sequence:
            self._call("cfear_odometry_status", None)
            return None
        out = np.zeros(self.B, dtype=np.int32)
        rc = self._ctx._L.cfear_odometry_status(self._ctx._h, self._h, out.ctypes.data)
        if rc not in (0, ERR_CAPACITY):  # (0 and CFEAR_ERR_CAPACITY are what the flag words describe; anything else - a HIP error, a failed join - is not)
            self._ctx._check(rc, "cfear_odometry_status")
        return out

    def covariances(self):
        """cov_current of every sequence after the last sweep: [B, 6, 6]"""
        out = np.zeros((self.B, 36))
        self._call("cfear_odometry_covariances", out.ctypes.data)
        return out.reshape(self.B, 6, 6)

    def summary(self, sequence):
        S = RegSummary()
        nc, nk = C.c_int(), C.c_int()
        self._call("cfear_odometry_summary", int(sequence), C.byref(S), C.byref(nc), C.byref(nk))
        return S, nc.value, nk.value
