/*
 * cfear_hip.h -- C ABI of the MI355X-native CFEAR hot path (libcfear_hip.so).
 *
 * Drop-in boundary for the per-scan path of dan11003/CFEAR_Radarodometry_code_public:
 *   k-strongest filter -> oriented surface points -> scan-to-keyframes registration.
 * Every entry point states the reference interface it replaces (file:line relative to the
 * reference repository). POD only: plain pointers, sizes and opaque handles; no C++/torch types.
 * All functions return 0 (CFEAR_OK) or a negative error code and never exit() (the reference
 * does: pointnormal.cpp:72-75, registration.cpp:24-25). cfear_last_error() gives the text.
 *
 * Threading: one cfear_ctx per caller thread / per sequence (the reference classes are not
 * re-entrant either, registration.h:104-131). All work of a context is ordered on its HIP stream.
 */
#ifndef CFEAR_HIP_H
#define CFEAR_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CFEAR_OK 0
#define CFEAR_ERR_INVALID (-1)     /* bad argument */
#define CFEAR_ERR_HIP (-2)         /* HIP runtime failure */
#define CFEAR_ERR_UNSUPPORTED (-3) /* size outside the compiled kernel range */
#define CFEAR_ERR_EMPTY (-4)       /* empty cloud (reference: exit(0)) */
#define CFEAR_ERR_NOMEM (-5)
#define CFEAR_ERR_CAPACITY (-6)    /* a scan produced more oriented surface points than CFEAR_TUNE_MAX_CELLS allows */

/* registration.h:48-60 */
enum { CFEAR_COST_P2P = 0, CFEAR_COST_P2L = 1, CFEAR_COST_P2D = 2 };
enum { CFEAR_LOSS_NONE = 0, CFEAR_LOSS_HUBER = 1, CFEAR_LOSS_CAUCHY = 2, CFEAR_LOSS_SOFTLONE = 3,
       CFEAR_LOSS_COMBINED = 4, CFEAR_LOSS_TUKEY = 5 };

/* radar_driver.h:24 */
enum { CFEAR_FILTER_KSTRONG = 0, CFEAR_FILTER_CACFAR = 1 };

/* Union of radarDriver::Parameters (radar_driver.h:35-48), OdometryKeyframeFuser::Parameters
 * (odometrykeyframefuser.h:72-114) and the n_scan_normal_reg knobs (n_scan_normal.h:72-81,
 * n_scan_normal.cpp:9, registration.h:117-122) that are on the path. */
typedef struct cfear_params {
  float z_min;        /* radar_driver.h:40 (float, truncated to int at radar_filters.cpp:198) */
  float range_res;    /* radar_driver.h:41 */
  float min_distance; /* radar_driver.h:45 */
  int32_t k_strongest;      /* radar_driver.h:42; 1..64 supported */
  double res;               /* odometrykeyframefuser.h:97 (narrowed to float at pointnormal.h:118) */
  double downsample_factor; /* pointnormal.h:241 */
  int32_t weight_intensity; /* odometrykeyframefuser.h:92 */
  int32_t cost;             /* CFEAR_COST_*  (cost_type string, odometrykeyframefuser.h:86) */
  int32_t loss;             /* CFEAR_LOSS_*  (loss_type_ string, :99) */
  int32_t weight_opt;       /* registration.h:50 */
  double loss_limit;        /* :100 */
  double covar_scale;       /* :101, SetD2dPar n_scan_normal.h:53 */
  double regularization;    /* :102 */
  int32_t submap_scan_size; /* :91 */
  int32_t compensate;       /* :95 */
  int32_t radar_ccw;        /* :95 */
  int32_t use_keyframe;     /* :96 */
  double min_keyframe_dist;    /* :98 */
  double min_keyframe_rot_deg; /* :98 */
  int32_t max_itr_association; /* n_scan_normal.h:75 (8) */
  int32_t min_itr;             /* n_scan_normal.h:75 (3) */
  int32_t max_solver_iterations; /* n_scan_normal.cpp:9 (20) */
  int32_t filter_type;         /* CFEAR_FILTER_* (radarDriver::Parameters::filter_type_, radar_driver.h:24,48): the stage-1 filter of the
                                  batched odometry objects (cfear_odometry_*); the per-call entry points name their filter themselves */
  double assoc_radius;         /* registration.h:122 (2.0) */
  /* filter_type CA-CFAR (radar_driver.cpp:52-56: AzimuthCACFAR(window_size, false_alarm_rate, nb_guard_cells, range_res, z_min,
   * min_distance, 400.0)); z_min is the static threshold there, k_strongest is not used */
  int32_t cfar_window_size;    /* radar_driver.h:43 (10) */
  int32_t cfar_nb_guard_cells; /* radar_driver.h:43 (20) */
  float cfar_false_alarm_rate; /* radar_driver.h:44 (0.01) */
  int32_t cfar_max_points;     /* detections per sweep a batched odometry object is sized for (0 = 32768; a pcl cloud grows, device
                                  memory is sized up front: a sweep with more detections keeps the first ones in (azimuth, range) order
                                  and the reading calls fail with CFEAR_ERR_CAPACITY) */
  double cfar_max_distance;    /* radar_driver.cpp:54 (400.0) */
} cfear_params;

void cfear_default_params(cfear_params* p);

typedef struct cfear_ctx cfear_ctx;

/* One context = one HIP device + stream + scratch. `stream` may be NULL (the context creates its
 * own: note that the handle of a framework's *default* stream is NULL too, and the stream created here is not
 * ordered with that default stream) or an existing hipStream_t passed as void*: device buffers handed to the
 * *_device entry points must be complete on that stream (or synchronized) before the call. A, R = polar image shape the context is sized
 * for (rows = azimuths, cols = range bins; radar_driver.cpp:92-98). */
int cfear_create(cfear_ctx** out, int device, void* stream, const cfear_params* p, int A, int R);
void cfear_destroy(cfear_ctx* ctx);
const char* cfear_last_error(const cfear_ctx* ctx);
int cfear_set_params(cfear_ctx* ctx, const cfear_params* p);
int cfear_synchronize(cfear_ctx* ctx);

/* Launch-shape knobs of a context (tuning; an integration never needs them, tools/ and bench.py do). Results do not depend on
 * them. FILTER_OCCUPANCY: 5..7 filter waves per SIMD (default 7); FILTER_ROWS_PER_WAVE: consecutive azimuths walked by one
 * filter wave (0 = the default: 4, or 6 in launches of 1536 scans and more); ODOMETRY_OVERLAP = n (0..8): batched odometry objects created afterwards run the filter of a sweep
 * on a low-priority stream of their own, one sweep ahead, and the features / registration kernels of n contiguous ranges of
 * the sequences on n high-priority streams (0 = the three kernels strictly in turn on the context stream; DESIGN.md has the
 * measurements). REPLAY_PERSISTENT_MAX (default 256): cfear_odometry_replay_host runs up to this many sequences as persistent
 * workgroups that walk a whole chunk of sweeps in one launch; more sequences (or 0) take the two launches per sweep of the
 * batched step. FILTER_CUS = F (with ODOMETRY_OVERLAP >= 1): the filter stream is created with a compute-unit mask of F units spread
 * evenly over the chip and the odometry streams with the complement (hipExtStreamCreateWithCUMask), so that the HBM-bound filter
 * of sweep t + 1 and the latency-bound odometry kernels of sweep t run side by side without sharing a unit's registers and LDS.
 * REPEAT_SHORTCUT (default 1): an outer registration iteration (n_scan_normal.cpp:102-151) that starts from the pose, radius and
 * keyframes of the previous one - a solve that accepted no step - repeats it bit for bit, so its summary is taken from the
 * previous one instead of associating and solving again; 0 runs it again (the tests compare the two).
 * MAX_CELLS = n (default 0 = A * k_strongest, the number of filtered points: cannot overflow - or 4096 if that is less and
 * submap_scan_size > 7): oriented surface points per scan the batched odometry objects created afterwards are sized for. A sequence's
 * memory is (submap_scan_size + 1) scan blocks of ~12 B per point + 160 B per cell, plus submap_scan_size * cells * 76 B of
 * residual-block scratch: one cell per filtered point is 7 MB at submap_scan_size 4, k 12, but 200 MB at submap_scan_size 50, k 40
 * (launch/oxford_demo:62-71) - where real scans have a few hundred to ~1500 cells; hence the 4096 for the large submaps. A scan that produces more cells than n keeps the first n (ascending voxel index) and the reading
 * calls (poses / covariances / summary / replay_host) return CFEAR_ERR_CAPACITY from then on: never silently.
 * REGISTRATION_ORDER (default 1; 0 = in sequence order): batched odometry objects created afterwards hand their sequences to the registration workgroups
 * longest first - sorted on the device by the work each sequence's registration took in the previous sweep - so that the last
 * round of workgroups of a launch is not left to the slowest ones (results do not depend on it).
 * LARGE_SUBMAP_KERNEL (default 0): with submap_scan_size > 7 the batched step has two registration kernels - the production shape compiled for
 * 64 scans (256 threads, three workgroups per compute unit) and one that gives a registration a whole unit (512 threads, all of its LDS for
 * the residual blocks, every wave evaluating: 2 x faster per registration at fifty keyframes). 0 = the second when the sequences fit the
 * chip at one per unit or the submap has 24 keyframes or more, 1 = always the first, 2 = always the second. Poses agree to the summation order of the evaluation's partial sums.
 * NN_TIE_RULE (default 0) - the one knob here that DOES change results, on purpose: which of several exactly equidistant cells the 1-NN search
 * of GetClosestIdx (pointnormal.cpp:238-254) returns. The reference leaves that to FLANN's kd-tree; 1-5 % of a scan's cells share their float
 * mean with another cell, and the choice moves a registration by up to centimetres on a few percent of the sweeps of a cluttered scene
 * (DESIGN.md section 2). 0 = the lowest cell index (production: a uniform grid search); 1 = the highest (the other end, for sensitivity runs);
 * 2 = what a restatement of flann::KDTreeSingleIndex (leaf size 15, as pcl::KdTreeFLANN builds it) returns - scans and batched odometry objects
 * created afterwards also build that tree (one thread, ~0.1-0.2 ms per scan) and every association walks it pair by pair: a parity mode for
 * comparisons with a build of the reference, several times slower than production. Set it before the scans / objects are created.
 * VOXEL_ORDER (default 0) - the second such knob: the order in which the points of a VoxelGrid voxel are added up for its float centroid
 * (pointnormal.cpp:277-280). PCL sorts (voxel index, point) pairs on the voxel index alone with an UNSTABLE sort, so the order inside a voxel -
 * and the centroid's last bit, which now and then flips a point across the strict d^2 < r^2 of the radius search - belongs to the sort
 * routine: std::sort up to PCL 1.9 (Ubuntu 18.04), boost integer_sort from 1.10. 0 = by point index (production: what a stable sort gives);
 * 1 = exactly what libstdc++'s std::sort leaves, computed on the host by the same call on the same sequence - per-call scans only
 * (cfear_scan_create; batched odometry objects refuse the mode: it costs a host round trip per scan).
 * FILTER_PEAKS (default -1 = automatic): whether the k-strongest filter runs AxialNonMaxSupress and sets the peak flag, bit 25 of a slot. Automatic:
 * every entry that hands slots or a peaks cloud to the caller computes it (cfear_kstrongest_device / _host, cfear_time_kstrongest, cfear_filter_polar*);
 * the filters inside cfear_odometry_step_* / _replay_* do not - their slot buffers are internal and the cloud pass of those routes reads the valid
 * bit, the range and the intensity only, as the reference's odometry never reads cloud_peaks - and leave the bit 0, unless the object records
 * peaks clouds (cfear_odometry_set_keyframe_clouds with CFEAR_KF_PEAKS: its filters compute the flag). 1 = always computed, 0 = never
 * (the per-call entries included: their peak bits are then 0 and a peaks cloud is empty; for A/B timing and tests). Bits 0..24 do not depend on it. */
enum { CFEAR_TUNE_FILTER_OCCUPANCY = 1, CFEAR_TUNE_FILTER_ROWS_PER_WAVE = 2, CFEAR_TUNE_ODOMETRY_OVERLAP = 3,
       CFEAR_TUNE_REPLAY_PERSISTENT_MAX = 4, CFEAR_TUNE_FILTER_CUS = 5, CFEAR_TUNE_REPEAT_SHORTCUT = 6, CFEAR_TUNE_MAX_CELLS = 7,
       CFEAR_TUNE_REGISTRATION_ORDER = 8, CFEAR_TUNE_LARGE_SUBMAP_KERNEL = 9, CFEAR_TUNE_NN_TIE_RULE = 10, CFEAR_TUNE_VOXEL_ORDER = 11,
       CFEAR_TUNE_FILTER_PEAKS = 12 };
int cfear_tune(cfear_ctx* ctx, int key, int value);
/* The launch shape cfear_kstrongest_device / _host and the batched filters use for n_scans images of this context under its FILTER_OCCUPANCY
 * and FILTER_ROWS_PER_WAVE knobs (the launcher calls the same arithmetic; no GPU work). One wave per resident slot (1024 SIMDs x occupancy), each
 * walking rows_per_wave consecutive azimuth rows = min(cap, ceil(n_scans * A / (1024 * occupancy))); the cap is the ROWS_PER_WAVE knob, or 4, or 6
 * from 1536 scans up (400 x 3360: 6 rows at 4608 scans, 4 at 1535, 1 at 5). workgroups = ceil(ceil(n_scans * A / rows_per_wave) / 4). occupancy =
 * workgroups per compute unit the kernel is compiled for: the knob clamped to 5..7 up to R = 4069, 3 up to R = 8165, 2 beyond. Any output may be null. */
int cfear_kstrongest_launch_shape(cfear_ctx* ctx, int n_scans, int* rows_per_wave, int* workgroups, int* occupancy);

/* ---- Stage 1: StructuredKStrongest (radar_filters.cpp:198-298) -----------------------------
 * Packed slot: bits 0..15 range bin | 16..23 intensity | 24 valid | 25 peak (AxialNonMaxSupress).
 * Per azimuth row k slots in ascending (intensity, range) order, unused slots = 0.
 * Bit 25 is set in the slots these entry points return. The internal slot buffers of the batched odometry routes (step, replay) are
 * filtered without the suppression and hold 0 there (cfear_tune FILTER_PEAKS) unless the object records peaks clouds (CFEAR_KF_PEAKS). */
#define CFEAR_SLOT_RANGE(s) ((int)((s) & 0xFFFFu))
#define CFEAR_SLOT_INTENSITY(s) ((int)(((s) >> 16) & 0xFFu))
#define CFEAR_SLOT_VALID(s) ((int)(((s) >> 24) & 1u))
#define CFEAR_SLOT_PEAK(s) ((int)(((s) >> 25) & 1u))

/* Batched filter on device-resident data, asynchronous on the context stream.
 * d_polar: n_scans contiguous A*R uint8 images; d_slots: n_scans*A*k uint32. */
int cfear_kstrongest_device(cfear_ctx* ctx, const uint8_t* d_polar, int n_scans, uint32_t* d_slots);
/* Same with host buffers (H2D, kernel, D2H, synchronous). Replaces FilterKstrongest +
 * AxialNonMaxSupress called from radarDriver::Process (radar_driver.cpp:58-60). */
int cfear_kstrongest_host(cfear_ctx* ctx, const uint8_t* h_polar, int n_scans, uint32_t* h_slots);

/* radarDriver::Callback for the non-Oxford datasets (radar_driver.cpp:74-90): the sensor image has rows = range bins and
 * columns = azimuths; cv::rotate(ROTATE_90_COUNTERCLOCKWISE) (:84) turns it into the rows = azimuth layout of every other
 * call here: out[i][j] = in[j][in_cols - 1 - i], out is in_cols x in_rows. The device variant takes n_images images back to
 * back and is asynchronous on the context stream; in and out must not overlap. */
int cfear_rotate_polar(cfear_ctx* ctx, const uint8_t* h_in, int in_rows, int in_cols, uint8_t* h_out);
int cfear_rotate_polar_device(cfear_ctx* ctx, const uint8_t* d_in, int n_images, int in_rows, int in_cols, uint8_t* d_out);

/* ---- Stage 1/1.5: point clouds -------------------------------------------------------------- */
typedef struct cfear_cloud cfear_cloud; /* pcl::PointCloud<pcl::PointXYZI> on the device */

/* radarDriver::CallbackOffline (radar_driver.cpp:163-176): polar image -> filtered cloud and
 * peaks cloud. h_polar: A*R uint8 host image (rows = azimuth). */
int cfear_filter_polar(cfear_ctx* ctx, const uint8_t* h_polar, cfear_cloud** cloud, cfear_cloud** cloud_peaks);
/* Same from a device-resident image (no copy). */
int cfear_filter_polar_device(cfear_ctx* ctx, const uint8_t* d_polar, cfear_cloud** cloud, cfear_cloud** cloud_peaks);
/* radarDriver::Process with filter_type "CA-CFAR" (radar_driver.cpp:52-56): AzimuthCACFAR(window_size,
 * false_alarm_rate, nb_guard_cells, range_res, z_min, min_distance, max_distance = 400.0)
 * .getFilteredPointCloud (cfar.cpp:27-87) -> filtered cloud, row-major over (azimuth, range bin). range_res, z_min
 * (static threshold) and min_distance come from the context parameters; the defaults of
 * radarDriver::Parameters are window_size 10, nb_guard_cells 20, false_alarm_rate 0.01 (radar_driver.h:43-44).
 * Synchronous (the cloud is sized by the detection count). */
int cfear_filter_cfar(cfear_ctx* ctx, const uint8_t* h_polar, int window_size, int nb_guard_cells, float false_alarm_rate,
                      double max_distance, cfear_cloud** cloud);
int cfear_filter_cfar_device(cfear_ctx* ctx, const uint8_t* d_polar, int window_size, int nb_guard_cells,
                             float false_alarm_rate, double max_distance, cfear_cloud** cloud);
/* The same filter over a batch of device-resident sweeps (n_scans images back to back), asynchronous on the context stream:
 * image i's detections go to d_xyi + i * capacity * 3 (x, y, intensity floats, same order as the per-call version, at most
 * `capacity` of them) and their number - the true count, which may exceed `capacity` - to d_counts[i]. The clouds feed
 * cfear_cloud_upload-style consumers or a caller's own kernels; sizes are known on the device without a host round trip. */
int cfear_filter_cfar_batch_device(cfear_ctx* ctx, const uint8_t* d_polar, int n_scans, int window_size, int nb_guard_cells,
                                   float false_alarm_rate, double max_distance, float* d_xyi, int capacity, int* d_counts);
/* The launch plan of the CA-CFAR detector for n_scans images of this context (4-byte-aligned image base; the launcher calls the same arithmetic,
 * csrc/cfar_shape.h; no GPU work). kernel: which detector takes the configuration - the owner-layout detector, or a round-5 kernel (rows that
 * are no whole dwords, no usable integer scale, more columns than the widest instantiation holds). For the owner-layout detector: TB bins per
 * thread x NW waves ({28,2} below 3584 bins, {20,3} below 3840, {16,4} below 4096, {32,4} below 8192; four waves whenever nb_guard_cells +
 * window_size > 128), RS columns of the transposed prefix array, full = the row is a whole number of threads' segments, sh / kopen the scale of
 * the integer test, window bound c of bin TB t + e at row e + cr[c], column padl + t + cq[c] of rows rmin .. TB + rmax - 1 (guard 10 / window 40
 * at 3360 bins: {28,2}, cr = 6, -10, 10, -6, 48 rows), fill = the row nearly fills the workgroup and a loop writes the columns right of the last
 * thread's, lds_bytes, per_cu persistent workgroups per compute unit, workgroups launched. The owner fields are 0 for a round-5 kernel, whose
 * workgroups are one per row. (The profiling overrides the launcher reads from the environment - CFEAR_CFAR_SHAPE, _PER_CU, _OLD_KERNELS,
 * _GENERAL_KERNEL - are not part of the plan.) */
enum { CFEAR_CFAR_KERNEL_OWNER = 0, CFEAR_CFAR_KERNEL_FAST16 = 1, CFEAR_CFAR_KERNEL_FAST32 = 2, CFEAR_CFAR_KERNEL_GENERAL = 3 };
typedef struct cfear_cfar_plan {
  int32_t kernel;
  int32_t TB, NW, RS, full;
  int32_t sh, kopen;
  int32_t rmin, rmax, cr[4], cq[4];
  int32_t padl, fill;
  int32_t lds_bytes, per_cu, workgroups;
} cfear_cfar_plan;
int cfear_cfar_launch_plan(cfear_ctx* ctx, int window_size, int nb_guard_cells, float false_alarm_rate, int n_scans, cfear_cfar_plan* plan);
/* One CA-CFAR detector of a grid (launch/oxford/eval/params/kstrong_vs_cfar/oxford-cfear-3-ca-cfar sweeps window_size x
 * false_alarm_rate, and guard cells and z_min are loops of the worker too): what AzimuthCACFAR takes besides the object-wide range_res,
 * min_distance and max_distance. */
typedef struct cfear_seq_detector {
  int32_t window_size, nb_guard_cells; /* >= 1, >= 0 */
  float false_alarm_rate;              /* > 0, finite */
  float z_min;                         /* the static threshold (cfar.cpp:45), finite */
} cfear_seq_detector;
/* Several detectors over shared images in one pass: d_polar holds n_sources images back to back, cloud c (of n_clouds) is the detections
 * of image source[c] under dets[c] (source NULL: cloud c reads image c, n_sources must be n_clouds) and goes to d_xyi + c * capacity * 3,
 * its true count to d_counts[c] - bit for bit what cfear_filter_cfar_batch_device gives for that image under a context whose z_min is
 * dets[c].z_min. A source row is staged and its prefix sum of squares built ONCE; every distinct (source, detector) is decided against it
 * once, however many clouds ask for it. Rows of a multiple of 4 bins up to 8192 with nb_guard_cells + window_size <= 2048 take that shared
 * kernel; every other shape cfear_filter_cfar_batch_device accepts runs its detectors once per distinct detector instead, same clouds.
 * CFEAR_ERR_INVALID for a bad detector or source (the message names the cloud and the field). Asynchronous on the context stream (a call
 * whose dets / source differ from the previous call's waits for the stream first: the table on the device is replaced). */
int cfear_filter_cfar_grid_device(cfear_ctx* ctx, const uint8_t* d_polar, int n_sources, const cfear_seq_detector* dets, const int32_t* source,
                                  int n_clouds, double max_distance, float* d_xyi, int capacity, int* d_counts);
/* Upload an existing cloud: xyi = n x (x, y, intensity) floats. */
int cfear_cloud_upload(cfear_ctx* ctx, const float* xyi, int n, cfear_cloud** cloud);
int cfear_cloud_size(cfear_ctx* ctx, const cfear_cloud* cloud, int* n);
int cfear_cloud_download(cfear_ctx* ctx, const cfear_cloud* cloud, float* xyi, int capacity, int* n);
/* m <= 16 clouds to the host with ONE synchronisation (counts and points travel together through pinned staging): what
 * radarDriver::CallbackOffline hands its caller is two clouds (radar_driver.cpp:59-60, 163-176), and Compensate (utils.cpp:96-113)
 * runs on both. xyi[i] receives min(n[i], capacity[i]) points; n[i] is the true count. xyi / capacity may be null (counts only). */
int cfear_clouds_download(cfear_ctx* ctx, const cfear_cloud* const* clouds, int m, float* const* xyi, const int* capacity, int* n);
/* Releasing a cloud or a scan parks its device block in the context for the next handle of a similar size (no hipFree, no
 * synchronisation on the per-sweep path; cfear_destroy gives everything back). Handles must not outlive their context. */
void cfear_cloud_release(cfear_ctx* ctx, cfear_cloud* cloud);
/* Compensate(cloud, Tmotion, ccw) (utils.h:49, utils.cpp:96-113); motion = (tx, ty, theta). In place. */
int cfear_compensate(cfear_ctx* ctx, cfear_cloud* cloud, const double motion_xyt[3], int ccw);
/* ... of the two clouds of one sweep by the same motion in one launch (odometrykeyframefuser.cpp:148-149 compensates cloud and cloud_peaks) */
int cfear_compensate_pair(cfear_ctx* ctx, cfear_cloud* cloud, cfear_cloud* cloud_peaks, const double motion_xyt[3], int ccw);

/* ---- Stage 2: MapPointNormal (pointnormal.h:110-243) ------------------------------------------ */
typedef struct cfear_scan cfear_scan; /* MapNormalPtr: cells + search structure, device resident */

/* One oriented surface point (class cell, pointnormal.h:45-105). */
typedef struct cfear_cell {
  double mean[2];   /* u_ */
  double cov[3];    /* cov_ xx, xy, yy */
  double normal[2]; /* snormal_ */
  double orth[2];   /* orth_normal (sign not defined by the reference) */
  double lambda_min, lambda_max;
  double scale;     /* scale_ (planarity) */
  double sum_intensity, avg_intensity;
  int32_t nsamples; /* Nsamples_ */
  int32_t valid;
} cfear_cell;

/* MapPointNormal(cld, radius = params.res, origin = (0,0), weight_intensity, raw = false)
 * (pointnormal.cpp:65-90 -> ComputeNormals :265-297 -> ComputeSearchTreeFromCells :151-162). */
int cfear_scan_create(cfear_ctx* ctx, const cfear_cloud* cloud, cfear_scan** scan);
/* MapPointNormal over given cells: raw = true (one identity cell per point, pointnormal.cpp:76-82, cell::GetIdentityCell
 * pointnormal.h:58,80-82) and the transformed-copy constructor (pointnormal.cpp:91-110) build the cell list on the host and
 * hand it over here; the device builds the search structure (ComputeSearchTreeFromCells :151-162) and the registration
 * views. Synchronous. */
int cfear_scan_from_cells(cfear_ctx* ctx, const cfear_cell* cells, int n, cfear_scan** scan);
void cfear_scan_release(cfear_ctx* ctx, cfear_scan* scan);
int cfear_scan_size(cfear_ctx* ctx, const cfear_scan* scan, int* n_cells);          /* GetSize() */
int cfear_scan_download_cells(cfear_ctx* ctx, const cfear_scan* scan, cfear_cell* cells, int capacity, int* n);
/* GetClosestIdx(p, d) (pointnormal.cpp:238-254) for nq query points; idx[i] = -1 if none. */
int cfear_scan_closest(cfear_ctx* ctx, const cfear_scan* scan, const double* qxy, int nq, double d, int32_t* idx);

/* ---- Stage 3: n_scan_normal_reg (n_scan_normal.h:27-85) ---------------------------------------- */
#define CFEAR_MAX_OUTER 64
typedef struct cfear_reg_summary {
  int32_t success;          /* Register() return value */
  int32_t usable;           /* solver solution usable (summary_.IsSolutionUsable()) */
  int32_t outer_iterations; /* itr_ as documented at n_scan_normal.cpp:161 */
  int32_t num_residuals;    /* problem_->NumResiduals() of the last problem */
  int32_t num_residual_blocks;
  int32_t assoc_path;       /* diagnostic, no reference counterpart: which association path the last problem build took - 1 = one block of source
                               cells against <= 4 keyframes (matches in registers), 2 = (group of four keyframes, cell) items dealt densely
                               (large submaps, dense scans), 3 = pair ranges per thread (the general path; also every NN_TIE_RULE != 0) */
  double final_cost;        /* summary_.final_cost */
  double score;             /* getScore() */
  int32_t inner_iterations[CFEAR_MAX_OUTER]; /* summary_.iterations.size() per outer iteration */
  int32_t termination[CFEAR_MAX_OUTER];      /* 0 CONVERGENCE, 1 NO_CONVERGENCE, 2 FAILURE */
  double outer_cost[CFEAR_MAX_OUTER];
  double outer_pose[CFEAR_MAX_OUTER][3];
} cfear_reg_summary;

/* bool Register(std::vector<MapNormalPtr>& scans, std::vector<Eigen::Affine3d>& Tsrc,
 *               std::vector<Matrix6d>& reg_cov, bool soft_constraints=false)
 * (n_scan_normal.cpp:82-187). scans[0..n-2] keyframes (fixed), scans[n-1] current.
 * poses_xyt: n x (x, y, theta) in/out; cov6_last: 36 doubles row-major = reg_cov.back(), in/out: a registration that
 * does not produce a usable solution leaves it as passed in, as the reference leaves reg_cov.
 * Returns CFEAR_OK; the reference's bool is summary->success. */
int cfear_register(cfear_ctx* ctx, cfear_scan* const* scans, int n, double* poses_xyt, double* cov6_last,
                   cfear_reg_summary* summary);

/* Register(..., soft_constraints = true) (n_scan_normal.cpp:373-377): adds the Mahalanobis prior
 * mahalanobisDistanceError (n_scan_normal.h:259-290) on the last pose around its initial value, with the information
 * matrix of prior_cov6 = reg_cov.back() as passed in (36 doubles row-major; rows/columns x, y, yaw are used,
 * registration.cpp:123-129) and the weight sqrt(#cells of the last scan). Everything else as cfear_register. */
int cfear_register_soft(cfear_ctx* ctx, cfear_scan* const* scans, int n, double* poses_xyt, const double* prior_cov6,
                        double* cov6_last, cfear_reg_summary* summary);

/* bool RegisterTimeContinuous(std::vector<MapNormalPtr>& scans, std::vector<Eigen::Affine3d>& Tsrc, std::vector<Matrix6d>& reg_cov,
 *                             const Eigen::Affine3d& Tvel, bool soft_constraints=false, bool ccw=false)
 * (n_scan_normal.h:39, n_scan_normal.cpp:67-80): Register of a last scan whose motion distortion has NOT been removed.
 * velocity_xyt = Affine3dToVectorXYeZ(Tvel), the motion over one sweep. Source cell j of the last scan gets the stamp
 * ts_j = GetRelTimeStamp(mean_j, ccw) in (-0.5, 0.5] (utils.h:28-32) and the transform Tcomp_j = vectorToAffine2d(ts_j * velocity);
 * the association - nearest-neighbour query, 30 degree gate, direction similarity and the weights built on it - uses Tcomp_j mean_j
 * and Tcomp_j.linear() normal_j, the P2P residual the corrected mean Tcomp_j mean_j (P2PEfficientContinuousCost), the P2L and
 * P2D residuals the UNCORRECTED mean_j as the reference does (n_scan_normal.cpp:279-300). Outer loop, solver,
 * termination, covariance and summary as cfear_register. prior_cov6: NULL, or the prior of cfear_register_soft. A velocity of
 * zero is cfear_register / cfear_register_soft bit for bit. Returns CFEAR_ERR_INVALID for a null or non-finite velocity. */
int cfear_register_time_continuous(cfear_ctx* ctx, cfear_scan* const* scans, int n, double* poses_xyt, const double velocity_xyt[3], int ccw,
                                   const double* prior_cov6 /* NULL: no soft constraint */, double* cov6_last, cfear_reg_summary* summary);

/* bool GetCost(std::vector<MapNormalPtr>& scans, std::vector<Eigen::Affine3d>& Tsrc, double& score,
 *              std::vector<double>& residuals) (n_scan_normal.cpp:188-213; called by the cost-sampling covariance,
 * odometrykeyframefuser.cpp:305): associations and residual blocks at the given poses, no solve. itr = the object's
 * itr_ (1 = double association radius, n_scan_normal.cpp:222). *score = 1/2 sum rho (ceres::Problem::Evaluate),
 * residuals = the robustified residuals in residual-block order (at most `capacity` are written), *n_residuals =
 * their number. Returns CFEAR_ERR_EMPTY (and *n_residuals = -1) where the reference returns false (<= 1 residuals). */
int cfear_get_cost(cfear_ctx* ctx, cfear_scan* const* scans, int n, const double* poses_xyt, int itr, double* score,
                   double* residuals, int capacity, int* n_residuals);

/* bool OdometryKeyframeFuser::approximateCovarianceBySampling(scans_vek, T_vek, cov_sampled)
 * (odometrykeyframefuser.cpp:261-380): GetCost on samples_per_axis^3 poses around poses_xyt[n-1] (all samples in one
 * launch, one workgroup each), least-squares quadratic, Hessian -> covariance scaled by GetCovarianceScaler
 * (final_cost / (num_residuals - 3) of the preceding Register) and covariance_scaler. Parameters are
 * par.cov_sampling_xy_range (0.4), cov_sampling_yaw_range (0.0043625), cov_sampling_samples_per_axis (3),
 * cov_sampling_covariance_scaler (4.0) (odometrykeyframefuser.h:107-110). *success = the reference's bool; cov6 = 36
 * doubles row-major (written only on success); sample_costs: optional samples_per_axis^3 sampled costs. */
int cfear_cov_by_sampling(cfear_ctx* ctx, cfear_scan* const* scans, int n, const double* poses_xyt, int itr, double xy_range,
                          double yaw_range, int samples_per_axis, double covariance_scaler, double final_cost,
                          int num_residuals, double* cov6, int* success, double* sample_costs);

/* void GetSurface(std::vector<MapNormalPtr>& scans, std::vector<Eigen::Affine3d>& Tsrc, std::vector<Matrix6d>& reg_cov,
 *                 bool soft_constraints, Eigen::MatrixXd& surface, double res, int width) (n_scan_normal.cpp:29-65).
 * The grid: pixels = ceil(2.0 * width / res) + 1 per side (:47); row i walks x, column j walks y, both by the reference's loop
 * `for (v = v0 - width; v <= v0 + width; v = v + res)` accumulated in double from the last pose (x0, y0), so each axis visits
 * pixels or pixels - 1 values depending on the estimate. cfear_surface_dims: pixels and the values visited along x (*nx) and y (*ny);
 * host only (no context, no device). CFEAR_ERR_INVALID for a res that is not finite or <= 0 or a width < 0, CFEAR_ERR_UNSUPPORTED
 * above CFEAR_SURFACE_MAX_SIDE pixels per side. */
#define CFEAR_SURFACE_MAX_SIDE 2048
int cfear_surface_dims(double res, int width, double x0, double y0, int* pixels, int* nx, int* ny);
/* GetSurface itself: every scan fixed but the last (InitFixedBlocks, :32), the problem built ONCE at the round-tripped poses
 * (Affine3dToVectorXYeZ, :35-38) with the object's itr_ (1 = double association radius, :222) - the associations are not rebuilt
 * per pixel, unlike GetCost - then ceres::Problem::Evaluate at every pixel (x, y, yaw of the estimate): 1/2 sum w rho(|r|^2), plus
 * with prior_cov6 (= reg_cov.back(), 36 doubles row-major; NULL = soft_constraints false) the Mahalanobis prior of
 * cfear_register_soft when the problem has more than one residual (:370-377). Nothing is refused for too few residuals (a problem
 * without blocks gives zeros). surface: pixels * pixels doubles, row-major, host memory; cells the reference's loops never reach
 * (which it leaves uninitialised) are NaN. nx, ny (optional): as cfear_surface_dims. Synchronises. */
int cfear_get_surface(cfear_ctx* ctx, cfear_scan* const* scans, int n, const double* poses_xyt, const double* prior_cov6, int itr,
                      double res, int width, double* surface, int* nx, int* ny);

/* ---- Batched odometry: OdometryKeyframeFuser::pointcloudCallback for B independent sequences ---
 * (odometrykeyframefuser.cpp:143-259, :397-411) with the filter of radar_driver.cpp:48-70 in front: k-strongest, or - with
 * cfear_params.filter_type = CFEAR_FILTER_CACFAR at creation - azimuth CA-CFAR (radar_driver.cpp:52-56; the peaks cloud stays empty
 * there and nothing on this path reads it).
 * All state (T_prev, Tmot, keyframe ring) lives on the device; one call = one radar sweep of every
 * sequence. */
typedef struct cfear_odometry cfear_odometry;
int cfear_odometry_create(cfear_ctx* ctx, int n_sequences, cfear_odometry** odo);
void cfear_odometry_destroy(cfear_ctx* ctx, cfear_odometry* odo);
int cfear_odometry_reset(cfear_ctx* ctx, cfear_odometry* odo);
/* d_polar: n_sequences contiguous A*R uint8 sweeps on the device. Asynchronous and stream-ordered for the input: the sweeps
 * must be ready at this point of the context stream, and work given to the context stream afterwards (the next write into
 * d_polar) runs after the filter has read it. With CFEAR_TUNE_ODOMETRY_OVERLAP the kernels run on two internal streams (the
 * filter of sweep t+1 beside the features / registration kernels of sweep t) that the context stream joins for the results only
 * in the reading calls below (poses / summary / profile_read / reset) and in cfear_synchronize(). */
int cfear_odometry_step_device(cfear_ctx* ctx, cfear_odometry* odo, const uint8_t* d_polar);
/* The same step from clouds that are already on the device instead of polar sweeps - whatever produced them (cfear_filter_cfar_batch_device,
 * a caller's own detector): sequence q's cloud is d_xyi + q * capacity * 3 (x, y, intensity floats, as cfear_cloud_upload takes them),
 * its size min(d_counts[q], capacity). What pointcloudCallback does with a cloud follows: Compensate (odometrykeyframefuser.cpp:146-150),
 * MapPointNormal (:161), Register, keyframe logic. capacity must not exceed the points the object's scans are sized for (A * k_strongest,
 * or cfar_max_points with filter_type CA-CFAR). Asynchronous on the context stream; d_xyi / d_counts are read by the first kernel only.
 * With filter_type CA-CFAR, cfear_odometry_step_device / _step_host / _replay_* run AzimuthCACFAR in front of exactly this. */
int cfear_odometry_step_cloud_device(cfear_ctx* ctx, cfear_odometry* odo, const float* d_xyi, int capacity, const int* d_counts);
/* Same from a host buffer (n_sequences * A * R bytes): the sweeps are copied to a staging buffer on the device; the call
 * returns when that copy has completed (h_polar may be reused or freed at once), the kernels run asynchronously as above. */
int cfear_odometry_step_host(cfear_ctx* ctx, cfear_odometry* odo, const uint8_t* h_polar);
/* Tcurrent of every sequence as (x, y, theta); synchronises the stream. */
int cfear_odometry_poses(cfear_ctx* ctx, cfear_odometry* odo, double* poses_xyt);
/* cov_current of every sequence after the last sweep (the Covariance& of the five-argument pointcloudCallback,
 * odometrykeyframefuser.cpp:196,397-411): n_sequences x 36 doubles row-major - the registration covariance of the sweep's
 * Register() (GetCovariance), the identity FormatScans starts from when the registration had no usable solution, zeros before
 * the second sweep - or, with cfear_odometry_set_cov_sampling on, the cost-sampling covariance of the sweep where it succeeded
 * (odometrykeyframefuser.cpp:202-208). Synchronises. */
int cfear_odometry_covariances(cfear_ctx* ctx, cfear_odometry* odo, double* cov6);
/* estimate_cov_by_sampling and its companions (odometrykeyframefuser.h:104-110: cov_sampling_xy_range 0.4, cov_sampling_yaw_range
 * 0.0043625, cov_sampling_samples_per_axis 3, cov_sampling_covariance_scaler 4.0) for every sequence of a batched odometry object, from
 * its next sweep on, on every route of the object (cfear_odometry_step_*, cfear_odometry_replay_*). Off by default (= the behaviour
 * without the call). On: after each sweep's Register and sanity check, GetCost at samples_per_axis^3 poses around the registered pose
 * against the keyframes the registration used (:261-380, as cfear_cov_by_sampling; itr = the sweep's outer iterations), and
 * cov_current becomes the sampled covariance where the fit is convex and num_residuals != 3. Poses, keyframes and records do not
 * change. samples_per_axis 1..8 (CFEAR_ERR_UNSUPPORTED above, CFEAR_ERR_INVALID below 1 or for a range / scaler that is not finite;
 * the object keeps its previous setting). enable = 0 switches it off (the other arguments are not read). cfear_odometry_reset keeps
 * the setting. Synchronises the context stream. */
int cfear_odometry_set_cov_sampling(cfear_ctx* ctx, cfear_odometry* odo, int enable, double xy_range, double yaw_range,
                                    int samples_per_axis, double covariance_scaler);
/* The last sweep's sampled costs of one sequence (samples_per_axis^3 doubles, the reference's sample order :294-296 - what
 * cov_samples_to_file_as_well would dump) and whether the sampled covariance was used (cov_sampled_success; 0 on a sequence's first
 * sweep, which samples nothing). Either pointer may be NULL. CFEAR_ERR_INVALID while sampling is off. Synchronises. */
int cfear_odometry_cov_samples(cfear_ctx* ctx, cfear_odometry* odo, int sequence, double* costs, int* sampled);
/* Cost surfaces of the batched step (GetSurface, n_scan_normal.cpp:29-65, as cfear_get_surface). enable = 1: from the next step on,
 * every registration records the scans, poses and itr_ it used (the record the cost-sampling covariance keeps; the sampling stage
 * itself does not run unless cfear_odometry_set_cov_sampling is on). Off by default; poses, covariances and summaries do not change;
 * cfear_odometry_reset keeps the setting. The replay routes do not record. */
int cfear_odometry_set_surface_recording(cfear_ctx* ctx, cfear_odometry* odo, int enable);
/* One surface per sequence around its last registration: the recorded scans, poses and itr_ - and, for a sequence whose recorded
 * registration ran soft (cfear_odometry_set_fuser_options), the prior the fuser passes: Identity66 around the recorded registered pose,
 * as cfear_get_surface with that prior_cov6 (a sequence without soft_constraint stays prior-free) - with one build launch and one
 * evaluation launch for all sequences. d_surface: caller-owned device buffer of n_sequences *
 * pixels * pixels doubles (pixels: cfear_surface_dims), sequence q's surface row-major at q * pixels * pixels; unvisited cells NaN,
 * and a sequence without a registration in the last step (its first sweep) or no step since the last reset / replay: all NaN.
 * Optional host outputs of what was evaluated: n_used (n_sequences: scans of the problem, 0 = none), itr_used (n_sequences),
 * poses_used (n_sequences * 192 doubles: the (x, y, theta) of up to 64 scans, keyframes then the registered pose) - with
 * cfear_get_surface on the same scans they give the same surface. Reads the records after joining the step (synchronises the
 * context stream once); the launches are stream-ordered on the context stream, the result is valid until the next step or reset.
 * CFEAR_ERR_INVALID while neither the recording nor the cost sampling is on. */
int cfear_odometry_surface(cfear_ctx* ctx, cfear_odometry* odo, double res, int width, double* d_surface, int* n_used, int* itr_used,
                           double* poses_used);
/* ---- Parameter grids in one batch: per-sequence parameters and shared input sweeps. The reference evaluates one recording under many
 * parameter sets by running one offline_odometry process per point of a nested-loop grid (utils/worker:26-99, utils/start_workers:54-57);
 * each process builds its OdometryKeyframeFuser::Parameters (odometrykeyframefuser.h:72-114) from its own arguments. Here the points of
 * the grid are the sequences of one object: each sequence may run under its own parameter set, and several sequences may read the same
 * sweep, with the results of running each parameter set on its own.
 *
 * cfear_odometry_set_sequence_params: rows = n_sequences cfear_params, row q for sequence q (n_rows must be the object's n_sequences);
 * NULL: back to the context's parameters for all sequences. Per sequence: z_min, k_strongest (1 .. the context's, see below), res,
 * weight_intensity, loss, loss_limit, weight_opt, covar_scale, regularization, compensate, use_keyframe, min_keyframe_dist,
 * min_keyframe_rot_deg, max_itr_association, min_itr, max_solver_iterations; cost and submap_scan_size through
 * cfear_odometry_set_sequence_shapes below, whose values a row must then carry. Every other field (cost, submap_scan_size, filter_type, range_res, min_distance, downsample_factor,
 * radar_ccw, assoc_radius, cfar_*; with filter_type CA-CFAR also z_min) sizes memory or selects a kernel and must equal the context's value
 * in every row: otherwise CFEAR_ERR_INVALID with a message that names the row and the field, and nothing is changed. Only on an object
 * that has processed no sweep since cfear_odometry_create / cfear_odometry_reset (CFEAR_ERR_INVALID otherwise); cfear_odometry_reset
 * keeps the table. cfear_set_params on the context afterwards is checked against the table at the next step / replay (CFEAR_ERR_INVALID
 * there if a row no longer agrees in an object-wide field). Every batched route honours the table: the step and replay entry points, the
 * cost-sampling covariance (loss, weights, radius rule of the sampled GetCost) and cfear_odometry_surface (each sequence's loss).
 * Per-sequence z_min: the k-strongest filter runs once per input sweep with the smallest z_min of the rows and each sequence drops the
 * slots below its own - exact, because intensity is the filter's primary sort key (the k strongest above z are the members above z of
 * the k strongest above any z' <= z). The peaks flag of a slot does depend on the kept set; no batched route reads it.
 * Per-sequence k_strongest: the context's k_strongest K is what the filter runs with, once per input sweep, and what sizes the object
 * (the slot buffers, the A * K points of a scan, the default cell capacity); a row may carry any k in 1..K and its sequence then gives,
 * bit for bit, what an object created under a context with that k_strongest and otherwise equal parameters gives. Exact for the same
 * reason: the filter keeps a bearing's C <= K largest (intensity, range) keys ascending in front of the bearing's K slots, and the keys are
 * unique, so the k strongest are slots [max(C - k, 0), C), in the k-filter's own order; a sequence's cloud pass reads that window, and
 * takes the compact or the general feature path by its own A * k. The cost: every row pays the filter pass and the memory of K - make
 * the context's k_strongest the largest of the rows, no larger. A row with k_strongest < 1 or > K: CFEAR_ERR_INVALID (the message names
 * the row and k_strongest); so is a k other than K on a filter_type CA-CFAR object (the detector has no k). While a row's k differs from
 * K, cfear_odometry_step_cloud_device refuses to run (CFEAR_ERR_UNSUPPORTED: a cloud has no slots to take a window of).
 * Synchronises the context stream. */
int cfear_odometry_set_sequence_params(cfear_ctx* ctx, cfear_odometry* odo, const cfear_params* rows, int n_rows);
/* The parameter set sequence q runs with: its row, or the context's parameters without a table. */
int cfear_odometry_sequence_params(cfear_ctx* ctx, cfear_odometry* odo, int sequence, cfear_params* out);
/* source[q] in [0, n_sources): the input sweep sequence q reads (1 <= n_sources <= n_sequences). Afterwards cfear_odometry_step_device /
 * _step_host take n_sources sweeps and the replay entry points n_sweeps x n_sources x A x R bytes instead of n_sequences per sweep: a
 * shared sweep is stored, copied and filtered once. NULL: identity (one sweep per sequence). k-strongest objects only: a CA-CFAR object
 * refuses a map (its sequences share sweeps through cfear_odometry_set_sequence_detectors, whose clouds stay per sequence), and cfear_odometry_step_cloud_device refuses to run while one is set (both CFEAR_ERR_UNSUPPORTED). A source out of
 * range: CFEAR_ERR_INVALID, nothing changed. As the table: only before the first sweep since create / reset; reset keeps it.
 * Synchronises the context stream. */
int cfear_odometry_set_sequence_sources(cfear_ctx* ctx, cfear_odometry* odo, const int32_t* source, int n_sequences, int n_sources);
/* ---- Per-sequence cost metric and submap size: loops 6 and 7 of the evaluation grid (utils/worker:49-52, cost_type and submap_scan_size;
 * params/submap_keyframes/submap_keyframe_cfear-3 is P2P P2L P2D x 1 .. 10) as sequences of one object. Both fields select a kernel, and
 * submap_scan_size sizes memory too, so cfear_odometry_set_sequence_params alone keeps refusing rows that differ from the context in
 * them; they are set by a call of their own. */
typedef struct cfear_seq_shape {
  int32_t cost;             /* CFEAR_COST_P2P / _P2L / _P2D */
  int32_t submap_scan_size; /* 1 .. the context's submap_scan_size */
} cfear_seq_shape;
/* shapes[q]: the cost metric and the submap_scan_size sequence q runs with (n_rows must be the object's n_sequences); NULL: every sequence
 * back to the context's values. The context's submap_scan_size S sizes the object and stays what sizes it - S + 1 scan slots per sequence,
 * the residual-block scratch of S keyframes: a sequence with s <= S keeps a ring of s keyframes in slots 0 .. s of its S + 1 and gives, bit
 * for bit, what the only sequence of an object created under a context with that cost and submap_scan_size gives (where both run the same
 * kernel shape; the 512-thread kernel of large submaps sums an evaluation's partial results in another order than the 256-thread ones).
 * The cost: every sequence pays the slots and the scratch of S - make the context's submap_scan_size the largest of the rows, no larger -
 * and a sweep's registration stage is one launch per (cost, submap of up to 7 keyframes or more) present among the shapes, six at the
 * most, each on the kernel an object of that cost and size runs; shapes that form one group launch once.
 * Once shapes are set, cfear_odometry_set_sequence_params compares row q's cost and submap_scan_size with shapes[q] instead of the
 * context's (a disagreement: CFEAR_ERR_INVALID, row and field named, nothing changed), and cfear_odometry_sequence_params(q) reports
 * shapes[q]'s two values. Setting shapes while a table exists whose rows would then disagree is CFEAR_ERR_INVALID too.
 * CFEAR_ERR_INVALID (row and field named) for a submap_scan_size < 1 or > S or an unknown cost, for n_rows other than n_sequences, and on
 * an object that has processed a sweep since cfear_odometry_create / cfear_odometry_reset; CFEAR_ERR_UNSUPPORTED on an object created with
 * cfear_tune ODOMETRY_OVERLAP streams (their sub-batches are index ranges). Nothing changes on failure. cfear_odometry_reset keeps the
 * shapes. Every batched route honours them - the step entry points (host, device, cloud), both replay shapes, CA-CFAR objects, source
 * maps, per-sequence k_strongest and z_min, the fuser options, the cost-sampling covariance - except cfear_odometry_surface while the
 * shapes differ in COST (CFEAR_ERR_UNSUPPORTED: its evaluation is one launch per cost over all problems); shapes that differ only in
 * submap_scan_size work there. Synchronises the context stream. */
int cfear_odometry_set_sequence_shapes(cfear_ctx* ctx, cfear_odometry* odo, const cfear_seq_shape* shapes, int n_rows);
/* The shape sequence q runs with: shapes[q], or the context's cost and submap_scan_size without shapes. */
int cfear_odometry_sequence_shape(cfear_ctx* ctx, cfear_odometry* odo, int sequence, cfear_seq_shape* out);
/* ---- Per-sequence CA-CFAR detectors over shared sweeps: the detector grid of 4_filter_eval (params/kstrong_vs_cfar/oxford-cfear-3-ca-cfar:
 * window_size x false_alarm_rate, 49 jobs per recording; nb_guard_cells and z_min are loops too) as sequences of one filter_type CA-CFAR
 * object. dets[q]: the detector of sequence q (n_rows must be the object's n_sequences); source[q] in [0, n_sources): the sweep it reads
 * (NULL: one sweep per sequence, n_sources is ignored). NULL dets: back to the context's detector and one sweep per sequence. Afterwards
 * cfear_odometry_step_device / _step_host take n_sources sweeps and the replay entry points n_sweeps x n_sources x A x R bytes (the
 * dword rule of the replay is on n_sources x A x R then); a shared sweep is stored, copied and staged once, its prefix sums are built once
 * and every distinct (source, detector) is decided once (cfear_filter_cfar_grid_device); the clouds stay one per sequence, so the feature
 * and registration kernels and both replay shapes run as before, and sequence q gives bit for bit what the only sequence of a CA-CFAR
 * object under a context with dets[q] (and the row's other values) gives on the same sweeps. cfar_max_points and cfar_max_distance stay
 * the context's. Once set, cfear_odometry_set_sequence_params compares row q's cfar_window_size, cfar_nb_guard_cells,
 * cfar_false_alarm_rate and z_min with dets[q] instead of the context's, and cfear_odometry_sequence_params(q) reports dets[q]'s values;
 * setting detectors while a table exists whose rows would then disagree is CFEAR_ERR_INVALID. cfear_odometry_step_cloud_device refuses to
 * run while detectors with a source map are set (CFEAR_ERR_UNSUPPORTED: it takes one cloud per sequence).
 * CFEAR_ERR_UNSUPPORTED on a k-strongest object. CFEAR_ERR_INVALID (row and field named, nothing changed) for window_size < 1,
 * nb_guard_cells < 0, a false_alarm_rate that is not finite or <= 0, a z_min that is not finite, a source outside [0, n_sources),
 * n_sources outside 1 .. n_sequences, n_rows other than n_sequences, and on an object that has processed a sweep since
 * cfear_odometry_create / cfear_odometry_reset. cfear_odometry_reset keeps the detectors. Composes with shapes, the parameter table, the
 * fuser options, the cost-sampling covariance, both replay shapes and cfear_odometry_status. Synchronises the context stream. */
int cfear_odometry_set_sequence_detectors(cfear_ctx* ctx, cfear_odometry* odo, const cfear_seq_detector* dets, int n_rows, const int32_t* source,
                                          int n_sources);
/* The detector sequence q runs with: dets[q], or the context's cfar_* values and z_min without a call. */
int cfear_odometry_sequence_detector(cfear_ctx* ctx, cfear_odometry* odo, int sequence, cfear_seq_detector* out);
/* ---- The fuser's own switches on the batched routes (OdometryKeyframeFuser::Parameters soft_constraint and use_guess,
 * odometrykeyframefuser.h:94; offline_odometry.cpp:166,273-274; the third loop of the evaluation grid, utils/worker:43), per object or per
 * sequence. They are not in cfear_params (whose layout is fixed); the defaults are what the batched routes did before: 0, 1. */
typedef struct cfear_fuser_options {
  int32_t soft_constraint; /* 1: Register(scans, T, cov, soft_constraints = true) (odometrykeyframefuser.cpp:186): on every sweep that
                            * registers, mahalanobisDistanceError (n_scan_normal.h:259-290) joins the problem after the residual-count
                            * check (n_scan_normal.cpp:370-377) - covariance Identity66 (FormatScans, odometrykeyframefuser.cpp:486-491),
                            * centre the normalised Tguess of the sweep, weight sqrt(cells of the current scan), rebuilt around the same
                            * centre at every outer iteration. As cfear_register_soft: num_residuals counts three more; final_cost,
                            * outer_cost, the termination tests and GetCovariance include the prior, and the summary, the sweep records
                            * and cfear_odometry_covariances report exactly that. The cost sampling (cfear_odometry_set_cov_sampling)
                            * samples GetCost without the prior (n_scan_normal.cpp:202) and scales with the soft Register's final_cost
                            * and num_residuals (GetCovarianceScaler, :435-441). */
  int32_t use_guess;       /* 0: Tguess = T_prev (odometrykeyframefuser.cpp:167-168) instead of T_prev * Tmot (:166): the start of the
                            * registration, the fallback of AccelerationVelocitySanityCheck (:199) and the centre of the prior.
                            * Motion compensation still uses Tmot. */
} cfear_fuser_options;
void cfear_default_fuser_options(cfear_fuser_options* o); /* soft_constraint 0, use_guess 1 */
/* rows: n_rows = 1 (every sequence) or the object's n_sequences (row q for sequence q); NULL: back to the defaults. CFEAR_ERR_INVALID
 * for a value other than 0 or 1 (the message names the row and the field), for any other n_rows, or on an object that has processed a
 * sweep since cfear_odometry_create / cfear_odometry_reset; nothing changes on failure. cfear_odometry_reset keeps the setting. It is
 * independent of the parameter table and the source map and works with or without either, on k-strongest and CA-CFAR objects; every
 * route of the object honours it (cfear_odometry_step_*, cfear_odometry_replay_*, both registration kernels, ODOMETRY_OVERLAP), and the
 * record behind the cost sampling and cfear_odometry_surface notes that the registration ran soft. Synchronises the context stream. */
int cfear_odometry_set_fuser_options(cfear_ctx* ctx, cfear_odometry* odo, const cfear_fuser_options* rows, int n_rows);
/* The options sequence q runs with (the defaults without a call). */
int cfear_odometry_fuser_options(cfear_ctx* ctx, cfear_odometry* odo, int sequence, cfear_fuser_options* out);
/* Has any scan of this object been truncated - more oriented surface points than CFEAR_TUNE_MAX_CELLS, or a cloud with more points than the object
 * holds? Synchronises the context stream; returns CFEAR_OK or CFEAR_ERR_CAPACITY (with the message the reading calls give). For callers of the
 * asynchronous cfear_odometry_replay_device, which read their records on the device and never pass through poses / summary / replay_host.
 * per_sequence (optional, n_sequences words): which sequences - bit 0 = a scan of that sequence lost cells, bit 1 = a cloud of it lost points;
 * the others' results are untouched (the condition is sticky until cfear_odometry_reset, like the return code). Bit 2 = the sequence's
 * keyframe log is full (cfear_odometry_set_keyframe_recording): keyframes were dropped, the odometry itself is untouched and the return
 * code stays CFEAR_OK. Switching the recording off clears the bit; it cannot be set while recording is off. */
int cfear_odometry_status(cfear_ctx* ctx, cfear_odometry* odo, int32_t* per_sequence);
/* Last Register() summary / cell count / keyframe count of one sequence (debug + parity tests). */
int cfear_odometry_summary(cfear_ctx* ctx, cfear_odometry* odo, int sequence, cfear_reg_summary* summary,
                           int* n_cells, int* n_keyframes);

/* ---- Replay of a recording: the loop of offline_odometry.cpp:103-125 (read a sweep, radarDriver::CallbackOffline,
 * OdometryKeyframeFuser::pointcloudCallback, keep the pose) for n_sweeps consecutive sweeps without a host round trip per
 * sweep. h_frames: n_sweeps x n_sequences x A x R bytes (sweep-major: sweep t of every sequence, then sweep t + 1). The sweeps
 * are copied and filtered in chunks on a stream of their own, two chunks in flight (the filter needs nothing but its input,
 * radar_driver.cpp:58), while features -> registration run sweep after sweep on the context stream; what a caller of
 * pointcloudCallback could observe after every sweep is kept on the device and comes back once, at the end. The state of
 * `odo` carries over between calls (and to / from cfear_odometry_step_*): a long recording may be handed over in pieces.
 * Synchronous: returns when the last sweep is done. Copies from pinned memory (cfear_host_alloc) overlap with the kernels;
 * from pageable memory the call still works, each chunk's copy then holds the calling thread. */
typedef struct cfear_sweep_record {
  double pose[3];             /* Tcurrent after the sweep (x, y, theta) */
  double final_cost;          /* summary_.final_cost of the sweep's Register() (0 for the first sweep) */
  int32_t outer_iterations;   /* as cfear_reg_summary */
  int32_t num_residuals;
  int32_t n_keyframes;        /* keyframes after the sweep (odometrykeyframefuser.cpp:470-476) */
  int32_t n_cells;            /* oriented surface points of the sweep's scan */
  int32_t inner_iterations[8];/* summary_.iterations.size() of the first 8 outer iterations */
} cfear_sweep_record;
int cfear_odometry_replay_host(cfear_ctx* ctx, cfear_odometry* odo, const uint8_t* h_frames, int n_sweeps,
                               cfear_sweep_record* records /* n_sweeps x n_sequences, or NULL */);
/* The same for sweeps that are already on the device (n_sweeps x n_sequences x A x R bytes, ready at this point of the context
 * stream), ASYNCHRONOUS: the call returns when everything is queued; d_records (device memory, n_sweeps x n_sequences records, or
 * NULL) is filled by the kernels, the sweeps are read until the last chunk's filter has run - work queued on the context stream
 * afterwards (a copy of d_records, the next write into d_frames) is ordered behind all of it. */
int cfear_odometry_replay_device(cfear_ctx* ctx, cfear_odometry* odo, const uint8_t* d_frames, int n_sweeps,
                                 cfear_sweep_record* d_records);
/* cfear_odometry_replay_host / _device plus cov_current after every sweep: cov6 = n_sweeps x n_sequences x 36 doubles row-major
 * (host memory for _host, device memory for _device, written by the kernels like d_records), or NULL = exactly the calls above. With
 * cost sampling off this is the registration covariance of every sweep (as cfear_odometry_covariances after it); on, the sampled one
 * where the sampling succeeded. */
int cfear_odometry_replay_host_cov(cfear_ctx* ctx, cfear_odometry* odo, const uint8_t* h_frames, int n_sweeps,
                                   cfear_sweep_record* records, double* cov6);
int cfear_odometry_replay_device_cov(cfear_ctx* ctx, cfear_odometry* odo, const uint8_t* d_frames, int n_sweeps,
                                     cfear_sweep_record* d_records, double* d_cov6);
/* Page-locked host memory for the sweeps of a replay (hipHostMalloc / hipHostFree). */
int cfear_host_alloc(cfear_ctx* ctx, size_t bytes, void** out);
void cfear_host_free(cfear_ctx* ctx, void* p);

/* ---- The keyframe graph of the batched routes: what OdometryKeyframeFuser keeps per KEYFRAME. processFrame ends a fused sweep with
 * scan_ = RadarScan(Tcurrent, TprevMot, cloud_peaks, cloud, Pcurrent, t) and AddToGraph(keyframes_, scan_, cov_current)
 * (odometrykeyframefuser.cpp:171-176, 234-248, 428-445): a node (RadarScan, types.h:93-143) with its oriented surface points and one
 * odometry Constraint3d to the previous keyframe (types.h:155-190) whose information matrix is the inverse of the covariance rotated
 * into the new keyframe's frame; offline_odometry --store_graph hands the result to the SLAM system downstream. With recording on, a
 * stage of its own behind the registration stage (and the cost sampling) appends the node - and the scan's cells - of every sequence
 * that fused to that sequence's log on the device: no host round trip per sweep, no change to any other kernel. cloud_nopeaks_ /
 * cloud_peaks_ (types.h:93-143) are recorded by a stage of their own when asked for (cfear_odometry_set_keyframe_clouds below); Tgt and
 * the stamp are not (`sweep` stands in). */
typedef struct cfear_keyframe_node {
  int32_t index;          /* RadarScan::idx_: 0, 1, 2 ... per sequence since cfear_odometry_create / cfear_odometry_reset */
  int32_t sweep;          /* the sweep of the sequence that fused (0-based since create / reset): the stamp's stand-in */
  int32_t n_cells;        /* oriented surface points of the scan (the sweep record's n_cells) */
  int32_t prev;           /* id_end of the odometry constraint: index - 1, or -1 for the first keyframe */
  double pose[3];         /* T (x, y, theta): the sweep record's pose, bit for bit */
  double motion[3];       /* motion_ = TprevMot, what the sweep was compensated with; (0, 0, 0) for the first keyframe (:172) */
  double t_be[3];         /* Constraint3d::t_be = T^-1 * T_prev as (x, y, theta) (:436); zeros when prev < 0 */
  double information[36]; /* Constraint3d::information, row-major over (x, y, z, roll, pitch, yaw) (:437-440); zeros when prev < 0. Where the sweep's
                           * cov_current cannot be inverted (singular or non-finite) the entries are inf / NaN, as Eigen's inverse() leaves them in the
                           * reference: the node is recorded all the same (cfear_keyframe_constraint on the host refuses the same input) */
} cfear_keyframe_node;    /* 376 bytes */
/* One oriented surface point of a recorded keyframe: exactly what the registration reads of a cell (and what cfear_scan_from_cells
 * reads of a cfear_cell) - a scan rebuilt from these is the scan the fuser registered against. */
typedef struct cfear_keyframe_cell {
  double mean[2], normal[2], cov[3], scale;
  int32_t nsamples, pad_;
} cfear_keyframe_cell;    /* 72 bytes */
#define CFEAR_KF_NODES 1
#define CFEAR_KF_CELLS 2
#define CFEAR_KF_CLOUD 4 /* cfear_odometry_set_keyframe_clouds: the motion-compensated filtered cloud of every node (cloud_nopeaks_) */
#define CFEAR_KF_PEAKS 8 /* ... and its motion-compensated peaks cloud (cloud_peaks_); needs CFEAR_KF_CLOUD */
/* The rule of AddToGraph :435-440, host only (no context, no device; the recorder runs the same function): from = the new keyframe's
 * pose, to = the previous one's, cov6 = cov_current of the sweep that fused -> t_be = Tfrom^-1 * Tto as (x, y, theta) and information =
 * C^-1 with C = cov6 whose leading 3x3 block is turned by the rotation of Tfrom^-1 (only that block: the (0,5) / (5,0) terms stay, as in
 * the reference). CFEAR_ERR_INVALID for a null pointer, a non-finite input or a singular C. */
int cfear_keyframe_constraint(const double from_xyt[3], const double to_xyt[3], const double cov6[36], double t_be_xyt[3], double information[36]);
/* what: 0 = off (releases the log; allowed at any time), CFEAR_KF_NODES, or CFEAR_KF_NODES | CFEAR_KF_CELLS. Capacities per sequence:
 * max_keyframes nodes, max_cells cells summed over its keyframes (ignored without CFEAR_KF_CELLS). Switching on: only on an object that
 * has processed no sweep since cfear_odometry_create / cfear_odometry_reset (CFEAR_ERR_INVALID otherwise); cfear_odometry_reset empties
 * the log and keeps the setting. While on, every route of the object records (cfear_odometry_step_*, both replay routes - which then
 * run two launches per sweep, not the persistent kernel -, per-sequence parameters / sources / shapes / detectors / fuser options,
 * cost sampling, ODOMETRY_OVERLAP). A keyframe that does not fit - its node or its cells - is dropped with every later keyframe of
 * that sequence (what is recorded is a gap-free prefix), counted in `dropped`, and sets bit 2 of that sequence's word in
 * cfear_odometry_status; it is not an error of the reading calls. Synchronises the context stream. */
int cfear_odometry_set_keyframe_recording(cfear_ctx* ctx, cfear_odometry* odo, int what, int max_keyframes, int max_cells);
/* Per sequence (n_sequences words each, either may be NULL): keyframes in the log, keyframes dropped. Synchronises the context stream,
 * like cfear_odometry_poses (so do the three calls below). CFEAR_ERR_INVALID while recording is off. */
int cfear_odometry_keyframe_counts(cfear_ctx* ctx, cfear_odometry* odo, int32_t* recorded, int32_t* dropped);
/* Nodes first, first + 1 ... of one sequence: at most `capacity` are written; *n = the nodes the sequence has recorded in all. */
int cfear_odometry_keyframe_nodes(cfear_ctx* ctx, cfear_odometry* odo, int sequence, int first, cfear_keyframe_node* nodes, int capacity, int* n);
/* The cells of keyframe `index` of one sequence, in the scan's order: at most `capacity` are written; *n = the node's n_cells.
 * CFEAR_ERR_INVALID for an index outside the recorded prefix or a log without CFEAR_KF_CELLS. */
int cfear_odometry_keyframe_cells(cfear_ctx* ctx, cfear_odometry* odo, int sequence, int index, cfear_keyframe_cell* cells, int capacity, int* n);
/* m per-call scans rebuilt from recorded keyframes of one sequence, device to device in one launch (a workgroup per scan): float means,
 * the registration views, the search grid and - under cfear_tune NN_TIE_RULE = 2 - the kd-tree, ready for cfear_register /
 * cfear_get_cost. Their cfear_cell records (cfear_scan_download_cells) carry the recorded fields bit for bit, valid = 1, orth =
 * (-normal_y, normal_x), lambda_min / lambda_max = the closed-form eigenvalues of cov, and BOTH INTENSITIES 0 (the log does not keep
 * them). Memory from the context's pool; release each with cfear_scan_release. CFEAR_ERR_INVALID for an index outside the recorded
 * prefix or a log without CFEAR_KF_CELLS, CFEAR_ERR_EMPTY for a keyframe without cells; nothing is created then. Synchronous. */
int cfear_odometry_keyframe_scans(cfear_ctx* ctx, cfear_odometry* odo, int sequence, const int32_t* indices, int m, cfear_scan** scans);
/* The two clouds of a node: scan_ = RadarScan(Tcurrent, TprevMot, cloud_peaks, cloud, ...) (odometrykeyframefuser.cpp:234-248) keeps the
 * motion-compensated filtered cloud (cloud_nopeaks_, :147) and the motion-compensated peaks cloud (cloud_peaks_, :149; types.h:93-143,
 * types.cpp:76-86). what: 0 = off (releases the point log; allowed at any time), CFEAR_KF_CLOUD, or CFEAR_KF_CLOUD | CFEAR_KF_PEAKS;
 * max_points: points per sequence, summed over both clouds of all its keyframes (12 bytes each). Switching on needs node recording
 * (cfear_odometry_set_keyframe_recording with CFEAR_KF_NODES, which also releases the point log whenever it is called) and, like it, an
 * object that has processed no sweep since create / reset; an object whose log cannot fit the device is refused with the per-sequence
 * footprint in the message. While on, a stage in front of the recorder writes, for every sequence that fused:
 *   the filtered cloud - exactly the points the sweep's cells were built from, in the reference's order (row-major over bearing and slot,
 *     after the drop at range <= ceil(min_distance / range_res), radar_filters.cpp:309-337), compensated with the node's `motion`; on the
 *     CA-CFAR / cfear_odometry_step_cloud_device routes the compensated input cloud;
 *   the peaks cloud - the same pass over the slots with the peak bit (getPeaksFilteredPointCloud(peaks = true) + Compensate); such an
 *     object's filter computes the flag (cfear_tune FILTER_PEAKS = 0 forced together with CFEAR_KF_PEAKS is refused, by this call and by the step / replay
 *     entries: CFEAR_ERR_INVALID; not on a CA-CFAR object, which runs no such filter).
 *     Bits 0..24 of the slots do not depend on it: poses, records, nodes and cells are those of an object without clouds, bit for bit.
 *     On the cloud routes the peaks cloud has 0 points, as the reference's (radar_driver.cpp:52-56).
 * A keyframe whose clouds do not fit is dropped whole - node, cells and clouds - with every later one, as for cells (a gap-free prefix,
 * `dropped`, status bit 2); the odometry is untouched. cfear_odometry_reset empties the point log and keeps the setting. With
 * ODOMETRY_OVERLAP streams the slot buffer is released to the next filter behind this stage instead of behind the feature stage. */
int cfear_odometry_set_keyframe_clouds(cfear_ctx* ctx, cfear_odometry* odo, int what, int max_points);
/* Points of the two clouds of nodes first, first + 1 ... of one sequence: at most `capacity` entries of each array (either may be NULL)
 * are written; *n = the nodes recorded. n_peaks is 0 throughout on a log without CFEAR_KF_PEAKS. CFEAR_ERR_INVALID without CFEAR_KF_CLOUD. */
int cfear_odometry_keyframe_cloud_sizes(cfear_ctx* ctx, cfear_odometry* odo, int sequence, int first, int32_t* n_cloud, int32_t* n_peaks, int capacity, int* n);
/* One cloud of keyframe `index` to the host: x, y, intensity per point as cfear_cloud_download; peaks = 0: the filtered cloud, 1: the
 * peaks cloud. At most `capacity` points are written; *n = the cloud's points. CFEAR_ERR_INVALID for an index outside the recorded prefix,
 * a log without CFEAR_KF_CLOUD, or peaks = 1 on a log without CFEAR_KF_PEAKS. */
int cfear_odometry_keyframe_cloud(cfear_ctx* ctx, cfear_odometry* odo, int sequence, int index, int peaks, float* xyi, int capacity, int* n);
/* m clouds of one sequence, device to device, as handles of the context's pool: ready for cfear_scan_create (a map at any res),
 * cfear_cloud_download and cfear_cloud_release. Errors as above; nothing is created then. Synchronous. */
int cfear_odometry_keyframe_clouds(cfear_ctx* ctx, cfear_odometry* odo, int sequence, const int32_t* indices, int m, int peaks, cfear_cloud** clouds);

/* ---- Constraints between ANY keyframes of a log, registered in one batch: the edges a SLAM back end adds to the odometry chain
 * (Constraint3d::type loop_appearance / mini_loop / candidate, types.h:150-190). One job registers keyframe `to` - the "current scan" -
 * against 1 .. CFEAR_KF_EDGE_MAX_FROM keyframes of the same sequence that sit fixed at their recorded node poses: Register(scans =
 * from[0 .. n_from - 1] + [to]) exactly as cfear_register runs it (outer loop, solver, covariance, summary; no prior) under the
 * parameters of the job's sequence - its cfear_params row and its shape's cost where it has them. All jobs run in one launch, a workgroup
 * each; every distinct keyframe of the job list is rebuilt from the log once (as cfear_odometry_keyframe_scans builds it, under
 * cfear_tune NN_TIE_RULE = 2 with its kd-tree) and read by all the jobs that name it. `to` may appear in `from`. */
#define CFEAR_KF_EDGE_MAX_FROM 16
typedef struct cfear_keyframe_edge_job {   /* 112 bytes */
  int32_t sequence;      /* whose log */
  int32_t to;            /* the keyframe that is registered */
  int32_t n_from;        /* 1 .. CFEAR_KF_EDGE_MAX_FROM fixed keyframes it is registered against */
  int32_t ref;           /* position in from[] of the keyframe the constraint is expressed to */
  int32_t flags;         /* bit 0: guess_xyt is given; otherwise the guess is `to`'s recorded pose */
  int32_t pad_;
  int32_t from[CFEAR_KF_EDGE_MAX_FROM];
  double guess_xyt[3];   /* pose of `to` in the frame of the recorded node poses */
} cfear_keyframe_edge_job;
/* The edge of one job, by the rule of a node's own edge: t_be and information = cfear_keyframe_constraint(from = the registered pose of
 * `to`, to = the node pose of from[ref], cov = the registration's covariance, which starts as zeros). A registration without a usable
 * solution leaves the covariance untouched, as cfear_register does: success = 0, t_be and information all zero. A covariance that cannot
 * be inverted leaves inf / NaN, as in the nodes. */
typedef struct cfear_keyframe_edge {       /* 400 bytes */
  int32_t sequence, to, from /* = job.from[job.ref] */, n_from;
  int32_t status;        /* 0, or a CFEAR_ERR_* of this job alone (CFEAR_ERR_UNSUPPORTED: NN_TIE_RULE could not be honoured, as cfear_register reports it) */
  int32_t success, usable, outer_iterations;   /* as cfear_reg_summary */
  int32_t num_residuals, num_residual_blocks, assoc_path, pad_;
  double pose[3];        /* registered pose of `to` (the guess where the registration has no usable solution) */
  double t_be[3];
  double final_cost, score;
  double information[36];
} cfear_keyframe_edge;
/* m jobs -> edges[m]; cov6 (m x 36 doubles) and summaries (m) receive every job's covariance and cfear_reg_summary, either may be NULL.
 * Checked on the host before anything is launched, each refusal naming job and field: CFEAR_ERR_INVALID for a sequence out of range, an
 * index outside the recorded prefix, n_from outside 1 .. CFEAR_KF_EDGE_MAX_FROM, ref outside 0 .. n_from - 1, a guess that is not finite
 * or a log without CFEAR_KF_CELLS; CFEAR_ERR_EMPTY for a keyframe without cells. No edge is written then. Working memory (the scans, and
 * per job match arrays of max(n_from, 4) x cells(to) pairs) comes from the context's pool and is back there on return. Synchronous;
 * drains the streams the reading calls drain; writes nothing to the log or the object. */
int cfear_odometry_keyframe_edges(cfear_ctx* ctx, cfear_odometry* odo, const cfear_keyframe_edge_job* jobs, int m, cfear_keyframe_edge* edges,
                                  double* cov6, cfear_reg_summary* summaries);

/* ---- KITTI drift of a batch's trajectories on the device: the metric of include/cfear_hip/kitti_metric.hpp (kitti_drift,
 * kitti_drift_by_length; what the reference's evaluation worker computes per job, launch/oxford/eval/utils/worker:94-98) for every
 * sequence of a batch at once. Segments: a start every 10 poses, lengths 100 ... 800 m, `last` = the first pose whose cumulative 3-D
 * path length exceeds dist[first] + len; per segment e = des^-1 * dgt with dgt = gt[first]^-1 * gt[last] (general inverse: 6-decimal
 * text poses are not exactly orthonormal) and des the same for the planar estimate (x, y, theta); r = acos(clamp(0.5 (trace(e_R) - 1))),
 * t = |e_t|, the segment contributes r / len and t / len. The totals are the means over all segments, the by-length tables the same
 * means over the segments of one length (0 for a length without a segment, as the totals are 0 without any). A non-finite pose makes
 * the totals of ITS row NaN, and the by-length entries of the lengths it touches, exactly as the host metric (its clamp keeps a NaN);
 * no other row changes. */
typedef struct cfear_drift {                 /* 184 bytes */
  double  translation_percent;
  double  rotation_deg_per_100m;
  double  translation_percent_by_length[8];   /* 100, 200 ... 800 m */
  double  rotation_deg_per_100m_by_length[8];
  int32_t segments;
  int32_t segments_by_length[8];
  int32_t reserved;                           /* 0 */
} cfear_drift;
typedef struct cfear_drift_plan cfear_drift_plan; /* the segments of one ground truth and their dgt, device resident */

/* The segment list of kitti_drift for n_gt ground-truth poses (gt34: 3x4 row-major, 12 doubles per pose), in its order: start-major,
 * then length; length_index 0..7 = 100 ... 800 m. Host only (no context, no device). At most `capacity` segments are written (the arrays
 * may be NULL with capacity 0); *n_segments is the number there are, and the return value CFEAR_ERR_CAPACITY if that is more than
 * `capacity`. CFEAR_ERR_INVALID for a null gt34 / n_segments, n_gt < 1 or a non-finite entry. */
int cfear_drift_segments(const double* gt34, int n_gt, int32_t* first, int32_t* last, int32_t* length_index, int capacity, int* n_segments);
/* The plan of one ground truth: its segment table, dgt and 1 / len per segment on the device. The segments of a replay of
 * n < n_gt sweeps are exactly the plan's segments with last < n (dist is a prefix sum, last a first crossing), so one plan scores any
 * shorter replay. CFEAR_ERR_INVALID (the message names the argument) for a null pointer, n_gt < 1 or a non-finite entry. Synchronous. */
int cfear_drift_plan_create(cfear_ctx* ctx, const double* gt34, int n_gt, cfear_drift_plan** plan);
void cfear_drift_plan_release(cfear_ctx* ctx, cfear_drift_plan* plan);
/* Scores n_sequences trajectories of n_sweeps poses against the plan over n = min(n_sweeps, n_gt) poses (n < 2 or no fitting segment:
 * zeros). The pose of sweep t of sequence q is the 3 doubles (x, y, theta) at d_poses + t * sweep_stride + q * seq_stride (bytes): for a
 * buffer of cfear_sweep_record as cfear_odometry_replay_device fills it, seq_stride = sizeof(cfear_sweep_record) and sweep_stride =
 * n_sequences * sizeof(cfear_sweep_record); packed poses have 24 and n_sequences * 24. d_out: n_sequences results in device memory. The
 * input is only read. Asynchronous on the context stream - behind a preceding cfear_odometry_replay_device with no synchronisation in
 * between. A row's result is a function of the plan, n_sweeps and that row's poses alone: bit-identical whatever the batch around it,
 * the strides, or the call. CFEAR_ERR_INVALID (the message names the argument) for a null pointer, a d_poses or a stride that is not a
 * multiple of 8, seq_stride < 24, n_sequences < 1 or n_sweeps < 0. */
int cfear_drift_device(cfear_ctx* ctx, const cfear_drift_plan* plan, const void* d_poses, size_t sweep_stride, size_t seq_stride,
                       int n_sweeps, int n_sequences, cfear_drift* d_out);
/* The same from / to host memory (stages through the context; synchronises). */
int cfear_drift_host(cfear_ctx* ctx, const cfear_drift_plan* plan, const void* h_poses, size_t sweep_stride, size_t seq_stride,
                     int n_sweeps, int n_sequences, cfear_drift* h_out);

/* ---- Optimising the keyframe graph on the device: batched SE(2) pose graphs (pose_graph.hip). Many independent graphs in one call and
 * one launch, a workgroup per graph with the whole Levenberg-Marquardt loop on the device. A graph is a set of nodes (x, y, theta) and
 * edges; one edge is exactly a g2o `EDGE_SE2 a b ...` line as this project writes it (replay._g2o_edge): for a node's own edge a is the
 * node's index and b its `prev`, for a cfear_keyframe_edge a is `to` and b is `from`. The error of an edge is expressed in the frame of
 * a, where the recorded information lives (cfear_keyframe_constraint turns the covariance by the rotation of Tfrom^-1; the form of
 * Ceres' pose_graph_2d):
 *   e_xy = R(theta_a)^T (t_b - t_a) - z_xy,  e_th = wrap(theta_b - theta_a - z_th) to [-pi, pi),  F = 1/2 sum_e rho_e(e^T Omega e)
 * with analytic Jacobians (csrc/pose_graph_dev.h: one function for the host and the device). rho is the identity on edges without
 * flag bit 0; on edges with it the options' loss (CFEAR_LOSS_NONE, CFEAR_LOSS_HUBER or CFEAR_LOSS_CAUCHY with loss_limit, Ceres'
 * definitions on the squared norm; any other CFEAR_LOSS_*: CFEAR_ERR_UNSUPPORTED), applied as iteratively reweighted least squares: the
 * edge's Omega is scaled by rho'(s) at the linearisation point, the reported cost uses rho(s).
 * The solver: (H + lambda diag(H)) p = -g (diag(H) clamped from below at 1e-6) by conjugate gradients under a block-Jacobi preconditioner
 * (the inverse of every node's damped 3x3 block); H is never assembled. A step is accepted when the robust cost falls, then lambda <-
 * max(lambda / 3, 1e-12); otherwise lambda <- min(4 lambda, 1e8). It stops on an accepted step with F - F_new <= function_tolerance * F,
 * on max|p| < parameter_tolerance (the step is not applied), at the iteration limit, or on a rejected step at the damping limit; CG stops
 * at |r| <= linear_tolerance * |g| or at its iteration limit. All sums run in a fixed order and there are no floating-point atomics: a
 * graph's poses and summary are bit-identical from run to run and whatever batch the graph is solved in.
 * Rules:
 *   - an edge whose z or info is not finite is skipped and counted in edges_skipped (node records carry inf / NaN information by design);
 *     the result is that of the graph without it, bit for bit;
 *   - a == b, or an index outside the edge's graph, is CFEAR_ERR_INVALID: the refusal names graph, edge and field, is made on the host
 *     before anything is launched, and no output is written;
 *   - the fixed node keeps its bits; a graph with no usable edge keeps all its poses bit for bit and reports CFEAR_PG_NOTHING_TO_DO;
 *   - a component that the fixed node does not reach is held by the damping alone (its blocks stay regular): it moves only as far as its
 *     own edges disagree; theta is not wrapped by the update (the error wraps);
 *   - an empty graph (0 nodes) in a batch is allowed. */
typedef struct cfear_pg_edge {       /* 88 bytes */
  int32_t a, b;          /* node indices inside the edge's graph */
  int32_t flags;         /* bit 0: the edge is robustified (the options' loss) */
  int32_t pad_;
  double z[3];           /* the measurement T_a^-1 * T_b as (x, y, theta) */
  double info[6];        /* upper triangle of the 3x3 information over (x, y, yaw): xx, xy, xt, yy, yt, tt (replay._g2o_edge's order) */
} cfear_pg_edge;
typedef struct cfear_pg_options {    /* 56 bytes */
  int32_t max_iterations;         /* 50: Levenberg-Marquardt iterations, accepted or not */
  int32_t max_linear_iterations;  /* 0: 30 x the graph's nodes; CG iterations per solve */
  int32_t loss;                   /* CFEAR_LOSS_NONE (default), CFEAR_LOSS_HUBER or CFEAR_LOSS_CAUCHY: on edges with flag bit 0 */
  int32_t pad_;
  double linear_tolerance;        /* 1e-8 */
  double function_tolerance;      /* 1e-12 */
  double parameter_tolerance;     /* 1e-10 */
  double initial_damping;         /* 1e-4 */
  double loss_limit;              /* 0.1 */
} cfear_pg_options;
enum { CFEAR_PG_CONVERGED_COST = 0, CFEAR_PG_CONVERGED_STEP = 1, CFEAR_PG_ITERATION_LIMIT = 2, CFEAR_PG_DAMPING_LIMIT = 3,
       CFEAR_PG_NOTHING_TO_DO = 4 };
typedef struct cfear_pg_summary {    /* 48 bytes, one per graph */
  double initial_cost, final_cost;  /* F at the poses given and at the poses returned */
  int32_t iterations;               /* Levenberg-Marquardt iterations run */
  int32_t accepted;                 /* ... of which accepted */
  int32_t linear_iterations;        /* CG iterations, summed over the solves */
  int32_t edges_used, edges_skipped;
  int32_t termination;              /* CFEAR_PG_* */
  int32_t status;                   /* 0 */
  int32_t pad_;
} cfear_pg_summary;
void cfear_pg_default_options(cfear_pg_options* options);
/* n_graphs graphs: graph g owns nodes node_offsets[g] .. node_offsets[g + 1] - 1 of poses_xyt (3 doubles each, in / out) and edges
 * edge_offsets[g] .. edge_offsets[g + 1] - 1, whose a / b count from the graph's first node. fixed: per graph the node that is held (NULL:
 * node 0 of every graph). options NULL: the defaults. Host pointers; synchronous; the working memory (30 doubles per node, 16 per edge,
 * the adjacency lists) comes from the context's pool and is back there on return. The graphs are handed to the workgroups largest
 * first; no result depends on that. CFEAR_ERR_INVALID (graph, edge and field named; nothing written) for offsets that do not ascend from
 * 0, a fixed node or an edge index out of range, a == b, or options that are not finite / negative; CFEAR_ERR_UNSUPPORTED for a loss
 * other than the three above. */
int cfear_pose_graph_optimize(cfear_ctx* ctx, int n_graphs, const int32_t* node_offsets, const int32_t* edge_offsets, const cfear_pg_edge* edges,
                              const int32_t* fixed, const cfear_pg_options* options, double* poses_xyt, cfear_pg_summary* summaries);
/* The graphs of an object's keyframe log, one per sequence, optimised in the same launch: the chain edges (a node's t_be / information
 * to `prev`, flag bit 0 clear) and the initial poses are read from the recorded nodes on the device - no download -, the caller adds m
 * records as cfear_odometry_keyframe_edges returned them, of any sequences in any order (they keep their order inside a sequence and
 * carry flag bit 0); those with success == 0 or status != 0 are left out. Node 0 of every sequence is held. pose_offsets: n_sequences + 1
 * words, sequence q's poses are poses_out[3 * pose_offsets[q] .. 3 * pose_offsets[q + 1]); capacity: the poses poses_out holds (too few:
 * CFEAR_ERR_CAPACITY with the offsets written, nothing else); poses_out and summaries NULL with capacity 0: the offsets alone. The result is
 * cfear_pose_graph_optimize's on the downloaded nodes and edges, bit for bit. Nothing is written to the log or the object: a replay
 * continued afterwards is byte-identical. CFEAR_ERR_INVALID while recording is off, for an edge whose sequence, to or from lies outside
 * the log, or to == from (the message names the edge and the field). Synchronous; drains the streams the reading calls drain. */
int cfear_odometry_keyframe_optimize(cfear_ctx* ctx, cfear_odometry* odo, const cfear_keyframe_edge* edges, int m, const cfear_pg_options* options,
                                     double* poses_out, int capacity, int32_t* pose_offsets, cfear_pg_summary* summaries);
/* F of one graph at given poses, host only (no context, no device), through the functions the kernel runs (pose_graph_dev.h); the edges
 * that are not finite are skipped and counted. used / skipped may be NULL. CFEAR_ERR_INVALID for a null pointer, an index out of range
 * or a == b; CFEAR_ERR_UNSUPPORTED for a loss other than NONE / HUBER / CAUCHY. */
int cfear_pose_graph_cost_host(const double* poses_xyt, int n_nodes, const cfear_pg_edge* edges, int n_edges, int loss, double loss_limit,
                               double* cost, int32_t* used, int32_t* skipped);

/* ---- Loop candidates by appearance: Scan-Context descriptors and their matching on the device (scan_context.hip; Kim & Kim, IROS 2018).
 * A descriptor is a polar image of a cloud in the sensor frame, bins[sector][ring] (uint32, n_sectors x n_rings, ring fastest), and its
 * ring key ring_sum[ring] = the sum of bins over the sectors.
 * Layout: ring_edge2[i] = (i * max_range / n_rings)^2 for i = 0 .. n_rings and sector_dir[j] = (cos, sin)(2 pi j / n_sectors), in double,
 *   the entries on the four axes exact. The table is computed once on the host (cfear_scan_context_layout); the kernels read it and take
 *   no cosine themselves.
 * Bin of a point (x, y, intensity), float32 widened to double, products and sums not contracted:
 *   - a point with a field that is not finite is skipped and counted in `dropped`; v = clamp(trunc(intensity), 0, 255);
 *   - r2 = x * x + y * y; r2 >= ring_edge2[n_rings]: out of range, skipped, not counted;
 *   - ring = #{ i in 1 .. n_rings - 1 : r2 >= ring_edge2[i] };
 *   - sector = 0 at x == 0 and y == 0; otherwise with cross_j = dir_j.x * y - dir_j.y * x: in the upper half plane (y > 0, or y == 0 and
 *     x >= 0) #{ j >= 1, 2j < n_sectors : cross_j >= 0 }, in the lower #{ j >= 1 : 2j <= n_sectors } + #{ j : 2j > n_sectors, cross_j >= 0 }.
 *   bins holds per bin the maximum of v, the sum of v, or the number of points (value). All integers: exact and free of any order. A
 *   cloud has at most CFEAR_SC_MAX_POINTS points, so every sum stays below 2^24.
 * Key distance (stage 1): K(a, b) = sum over rings of (ring_sum_a - ring_sum_b)^2 in 64 bits, exact; ties go to the smaller index.
 * Distance (stage 2): column j of a descriptor is bins[j][.]. For a shift s in 0 .. n_sectors - 1
 *     d(s) = 1 - (1 / n) sum_j cos(a_j, b_((j + s) mod n_sectors))  over the n columns j where both columns are nonzero, 1 when n = 0;
 *   distance = min_s d(s), shift = the smallest s that reaches it, yaw = shift * 2 pi / n_sectors in (-pi, pi]. a is `to`, b is `from`,
 *   and theta_to ~ theta_from + yaw. The device evaluates d in float32 in a fixed order (csrc/scan_context_dev.h): rings ascending with
 *   fused multiply-adds, columns ascending; a pair's distance is bit-identical whatever batch it is matched in and within
 *   (n_rings + n_sectors + 8) * 2^-24 of the float64 value.
 * Candidates of a set of N descriptors (one sequence's keyframes in log order): for every `to` the eligible `from` are 0 .. to -
 *   min_index_gap; stage 1 keeps the n_keys with the smallest K (all of them for n_keys = 0 or when fewer are eligible); stage 2 takes
 *   the distance of each; the max_per_node smallest distances <= max_distance are handed back, ties to the smaller `from`. Order of the
 *   output: set ascending, `to` ascending, then distance. */
#define CFEAR_SC_MAX 0   /* a bin holds the largest v of its points */
#define CFEAR_SC_SUM 1   /* ... their sum */
#define CFEAR_SC_COUNT 2 /* ... their number */
#define CFEAR_SC_MAX_RINGS 40
#define CFEAR_SC_MAX_SECTORS 120
#define CFEAR_SC_MAX_KEYS 64
#define CFEAR_SC_MAX_PER_NODE 16
#define CFEAR_SC_MAX_POINTS 65536
typedef struct cfear_sc_params {     /* 48 bytes */
  int32_t n_rings;        /* 1 .. 40, 20 */
  int32_t n_sectors;      /* 1 .. 120, 60 */
  int32_t value;          /* CFEAR_SC_MAX (default), CFEAR_SC_SUM or CFEAR_SC_COUNT */
  int32_t source;         /* the log routes: 0 = the filtered cloud of a keyframe (default), 1 = its peaks cloud */
  int32_t min_index_gap;  /* >= 1, 6 */
  int32_t n_keys;         /* 0 = every eligible keyframe goes to stage 2, else 1 .. 64; 10 */
  int32_t max_per_node;   /* 1 .. 16, 1 */
  int32_t pad_;
  double max_range;       /* metres, finite and > 0; 80 */
  double max_distance;    /* in (0, 1]; 0.4 */
} cfear_sc_params;
typedef struct cfear_sc_candidate {  /* 40 bytes */
  int32_t sequence;       /* the set */
  int32_t to, from;       /* positions in the set, from <= to - min_index_gap */
  int32_t shift;
  double distance, yaw;
  uint64_t key_distance;
} cfear_sc_candidate;
void cfear_sc_default_params(cfear_sc_params* params);
/* The layout table of params (n_rings, n_sectors, max_range), host only: ring_edge2[n_rings + 1], sector_dir[n_sectors][2]. CFEAR_ERR_INVALID
 * for a null pointer or a field out of range. */
int cfear_scan_context_layout(const cfear_sc_params* params, double* ring_edge2, double* sector_dir);
/* Descriptors of n_clouds caller clouds in host memory, a workgroup each in one launch: cloud c is points point_offsets[c] ..
 * point_offsets[c + 1] - 1 of xyi (x, y, intensity; point_offsets[0] = 0, ascending; a cloud may be empty). bins: n_clouds x n_sectors x
 * n_rings, ring_sums: n_clouds x n_rings, dropped: n_clouds (the last two may be NULL). params NULL: the defaults. CFEAR_ERR_INVALID, the
 * field - or the cloud - named and nothing written, for a parameter out of range, offsets that do not ascend from 0 or a cloud of more
 * than CFEAR_SC_MAX_POINTS points. Synchronous; working memory from the context's pool. */
int cfear_scan_context_describe(cfear_ctx* ctx, const cfear_sc_params* params, const float* xyi, const int32_t* point_offsets, int n_clouds, uint32_t* bins,
                                uint32_t* ring_sums, int32_t* dropped);
/* The candidates of n_sets sets of caller descriptors in one launch: set g owns descriptors set_offsets[g] .. set_offsets[g + 1] - 1 of
 * bins (as cfear_scan_context_describe wrote them; set_offsets[0] = 0, ascending, a set may be empty). *n: the candidates there are;
 * more than `capacity`: CFEAR_ERR_CAPACITY and nothing is written to `candidates` (NULL with capacity 0: the count alone). The
 * candidates of a set do not depend on the other sets of the call. Synchronous. */
int cfear_scan_context_match(cfear_ctx* ctx, const cfear_sc_params* params, int n_sets, const int32_t* set_offsets, const uint32_t* bins,
                             cfear_sc_candidate* candidates, int capacity, int* n);
/* The descriptors of every recorded keyframe of every sequence of the object, from the point log on the device in one launch (params.source:
 * the filtered or the peaks cloud); those of keyframes first .. of `sequence` are handed back, at most `capacity` (bins / ring_sums as
 * above, either may be NULL); *n: the keyframes the sequence has recorded. Needs a log with CFEAR_KF_CLOUD, and CFEAR_KF_PEAKS for
 * source = 1 (CFEAR_ERR_INVALID otherwise). Nothing is written to the log or the object: a replay continued afterwards is byte-identical.
 * Synchronous; drains the streams the reading calls drain. */
int cfear_odometry_keyframe_descriptors(cfear_ctx* ctx, cfear_odometry* odo, const cfear_sc_params* params, int sequence, int first, uint32_t* bins,
                                        uint32_t* ring_sums, int capacity, int* n);
/* Describe and match in one go: a set per sequence, its recorded keyframes in log order; clouds and descriptors stay on the device.
 * candidates / capacity / n as cfear_scan_context_match, `sequence` of a record is the sequence. The result is
 * cfear_scan_context_match's on the descriptors cfear_odometry_keyframe_descriptors hands back, byte for byte. The same conditions, and
 * as little written to the log. */
int cfear_odometry_keyframe_candidates(cfear_ctx* ctx, cfear_odometry* odo, const cfear_sc_params* params, cfear_sc_candidate* candidates, int capacity,
                                       int* n);

/* Filter-kernel timing with HIP events (bench.py roofline leg): enable, run steps, read. filter_seconds is the sum
 * of the durations of the filter launches, each measured on the stream it ran on. The events come from a pool created
 * when profiling is enabled (and grown in blocks), not one hipEventCreate per launch. */
int cfear_odometry_profile(cfear_ctx* ctx, cfear_odometry* odo, int enable);
int cfear_odometry_profile_read(cfear_ctx* ctx, cfear_odometry* odo, double* filter_seconds, int* filter_launches);
/* The same for the two kernels behind the filter (stages 1.5-2: cloud + compensation + oriented surface points;
 * stage 3 + caller: registration and keyframe logic), summed over the profiled launches. */
int cfear_odometry_profile_read_stages(cfear_ctx* ctx, cfear_odometry* odo, double* features_seconds, double* registration_seconds,
                                       int* launches);

/* Per-workgroup phase timestamps (tuning / bench.py's workgroup-time percentiles): enable = 1 switches the odometry steps
 * to the timed instantiations of the features and registration kernels (thread 0 of every workgroup stores wall_clock64()
 * ticks of 10 ns: slots 0..13 features phases, 14..28 registration phases, 29..31 accumulated evaluation / controller
 * ticks and evaluation count - these three need clock reads around every LM command and halve the speed of the
 * registration kernel; enable = 2 leaves them out: phase stamps only, still the timed instantiations; enable = 3 keeps the
 * PRODUCTION kernels and only records every workgroup's start and end clock in slots 0, 1 and 14, 15 - what bench.py's
 * workgroup-time percentiles use; enable = 4: timed instantiations, and slots 0..7 hold - instead of the first feature
 * stamps - the breakdown of the registration's command loop over its evaluation commands: ticks waiting at the command
 * barrier, executing the command, waiting at the result barrier, the command count, ticks in the controller's state
 * function (which includes the trust-region step that follows it), in trust-region steps taken on their own, in the
 * publishing function and in the end-of-solve function); with host_ticks != NULL the [n_sequences][32] table of the steps since the last read is
 * copied out (synchronises) and cleared. enable = 0 frees the table: back to the production kernels. */
int cfear_odometry_phase_times(cfear_ctx* ctx, cfear_odometry* odo, int enable, long long* host_ticks);

/* Timing hook used by bench.py: seconds of the filter kernel measured with HIP events on the
 * context stream over `iters` launches (after `warmup`). */
int cfear_time_kstrongest(cfear_ctx* ctx, const uint8_t* d_polar, int n_scans, uint32_t* d_slots,
                          int warmup, int iters, double* avg_seconds);

const char* cfear_version(void);

#ifdef __cplusplus
}
#endif
#endif
