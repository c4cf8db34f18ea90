// common.h -- shared host-side definitions of libcfear_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/cfear_hip.h"

#define CFEAR_WAVE 64

struct cfear_ctx;
static inline int cfear_fail(cfear_ctx* c, int code, const char* what, hipError_t e = hipSuccess);

// The owner of one hipMalloc allocation of size() elements: everything an object or the context keeps on the device (the blocks of clouds and
// scans come from the context's pool instead, see below). It frees when it is released, grown or destroyed, and hipFree waits for the whole
// device - but when a buffer MAY go is the caller's to know: it drains the streams that can still read the buffer first.
template <typename T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& b) noexcept : p_(b.p_), n_(b.n_) { b.p_ = nullptr; b.n_ = 0; }
  DevBuf& operator=(DevBuf&& b) noexcept {
    if (this != &b) { release(); p_ = b.p_; n_ = b.n_; b.p_ = nullptr; b.n_ = 0; }
    return *this;
  }
  ~DevBuf() { release(); }
  operator T*() const { return p_; }
  size_t size() const { return n_; }
  void release() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr; n_ = 0;
  }
  // room for `count` elements: nothing to do when they fit, a new (with `zero`: zero-filled) allocation otherwise - the old contents are gone.
  // A failure leaves the buffer empty and is reported as `what`.
  int ensure(cfear_ctx* ctx, size_t count, const char* what, bool zero = false) {
    if (count <= n_) return CFEAR_OK;
    release();
    if (hipMalloc(&p_, sizeof(T) * count) != hipSuccess) { p_ = nullptr; return cfear_fail(ctx, CFEAR_ERR_NOMEM, what); }
    n_ = count;
    const hipError_t e = zero ? hipMemset(p_, 0, sizeof(T) * count) : hipSuccess;
    if (e != hipSuccess) { release(); return cfear_fail(ctx, CFEAR_ERR_HIP, what, e); }
    return CFEAR_OK;
  }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};

// The owners of the other three things the runtime hands out, of DevBuf's shape: move-only, converting to the raw handle, gone with their
// owner. As with DevBuf, WHEN one may go is the caller's to know: the work that uses it is drained first.
// An event, created with the caller's flags (hipEventDefault: a timing event).
class Event {
 public:
  Event() = default;
  Event(Event&& b) noexcept : e_(b.e_) { b.e_ = nullptr; }
  Event& operator=(Event&& b) noexcept {
    if (this != &b) { release(); e_ = b.e_; b.e_ = nullptr; }
    return *this;
  }
  ~Event() { release(); }
  operator hipEvent_t() const { return e_; }
  void release() {
    if (e_) (void)hipEventDestroy(e_);
    e_ = nullptr;
  }
  hipError_t create(unsigned flags) {
    release();
    const hipError_t e = flags == hipEventDefault ? hipEventCreate(&e_) : hipEventCreateWithFlags(&e_, flags);
    if (e != hipSuccess) e_ = nullptr;
    return e;
  }
  // created on first use; a failure leaves it empty and is reported as `what` with the runtime's text
  int ensure(cfear_ctx* ctx, unsigned flags, const char* what) {
    if (e_) return CFEAR_OK;
    const hipError_t e = create(flags);
    return e == hipSuccess ? CFEAR_OK : cfear_fail(ctx, CFEAR_ERR_HIP, what, e);
  }

 private:
  hipEvent_t e_ = nullptr;
};

// A stream, made in one of the three ways this library makes them. It knows nothing of cfear_ctx::aux_streams: who creates a stream the
// context is to wait for adds it there, and takes it out again before the owner goes.
class Stream {
 public:
  Stream() = default;
  Stream(Stream&& b) noexcept : s_(b.s_) { b.s_ = nullptr; }
  Stream& operator=(Stream&& b) noexcept {
    if (this != &b) { release(); s_ = b.s_; b.s_ = nullptr; }
    return *this;
  }
  ~Stream() { release(); }
  operator hipStream_t() const { return s_; }
  void release() {
    if (s_) (void)hipStreamDestroy(s_);
    s_ = nullptr;
  }
  hipError_t create(unsigned flags) { release(); return made(hipStreamCreateWithFlags(&s_, flags)); }
  hipError_t create_with_priority(unsigned flags, int priority) { release(); return made(hipStreamCreateWithPriority(&s_, flags, priority)); }
  hipError_t create_with_cu_mask(const std::vector<uint32_t>& mask) { release(); return made(hipExtStreamCreateWithCUMask(&s_, (uint32_t)mask.size(), mask.data())); }

 private:
  hipError_t made(hipError_t e) {
    if (e != hipSuccess) s_ = nullptr;
    return e;
  }
  hipStream_t s_ = nullptr;
};

// DevBuf's twin for pinned host memory (hipHostMalloc): ensure() grows and never shrinks, the old contents are gone, and the caller has
// drained what may still read or write the old block.
template <typename T>
class PinnedBuf {
 public:
  PinnedBuf() = default;
  PinnedBuf(PinnedBuf&& b) noexcept : p_(b.p_), n_(b.n_) { b.p_ = nullptr; b.n_ = 0; }
  PinnedBuf& operator=(PinnedBuf&& b) noexcept {
    if (this != &b) { release(); p_ = b.p_; n_ = b.n_; b.p_ = nullptr; b.n_ = 0; }
    return *this;
  }
  ~PinnedBuf() { release(); }
  operator T*() const { return p_; }
  size_t size() const { return n_; }
  void release() {
    if (p_) (void)hipHostFree(p_);
    p_ = nullptr; n_ = 0;
  }
  int ensure(cfear_ctx* ctx, size_t count, const char* what) {
    if (count <= n_) return CFEAR_OK;
    release();
    if (hipHostMalloc(reinterpret_cast<void**>(&p_), sizeof(T) * count, hipHostMallocDefault) != hipSuccess) { p_ = nullptr; return cfear_fail(ctx, CFEAR_ERR_NOMEM, what); }
    n_ = count;
    return CFEAR_OK;
  }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};

// Members are destroyed last first: the pinned blocks and the events, then the context's own stream, then the device buffers above them.
struct cfear_ctx {
  int device = 0;
  hipStream_t stream = nullptr;  // the caller's, or own_stream (below)
  cfear_params par;
  int A = 0, R = 0;
  std::string err;
  // per-azimuth (cos, sin) of theta=(b+1)/A*2pi computed on the host with libm so that the
  // polar->Cartesian conversion (radar_filters.cpp:317-330) is bit-identical to a CPU run.
  DevBuf<double> d_trig;  // [A][2]
  // staging for the host entry points (these and the three below grow and never shrink)
  DevBuf<uint8_t> d_polar;
  DevBuf<uint32_t> d_slots;
  DevBuf<unsigned char> d_scratch;  // scratch for the per-call feature / registration kernels
  DevBuf<int> d_cfar_rows;          // row counts / bases of cfear_filter_cfar_batch_device
  struct cfear_cfar_grid* cfar_grid = nullptr;  // the plan and tables of the last cfear_filter_cfar_grid_device call (kept while the next call's dets / source equal them)
  DevBuf<double> d_drift;           // per-block partial sums of cfear_drift_device (drift.hip)
  // streams of the batched odometry objects of this context (cfear_synchronize waits for them too)
  std::vector<hipStream_t> aux_streams;
  // launch-shape knobs (cfear_tune): filter occupancy variant (5..7 waves per SIMD), rows walked per filter wave,
  // whether a batched odometry object created from now on runs its filter one sweep ahead on a stream of its own
  int tune_k1_occ = 7, tune_k1_rows = 0 /* 0 = by launch size: 4, or 6 from 1536 scans up */, tune_odo_overlap = 0;
  int tune_k1_peaks = -1;  // FILTER_PEAKS: -1 = the filter computes the peak flag where a caller can see the slots or a peaks cloud, 1 = always, 0 = never
  int tune_filter_cus = 0;  // with ODOMETRY_OVERLAP: compute units reserved for the filter stream (CU-masked streams); 0 = no masks
  int tune_reg_order = 1;  // batched odometry objects created afterwards launch their registration workgroups longest first (keys: the previous sweep's work)
  int tune_max_cells = 0;  // batched odometry: oriented surface points per scan the scan blocks / match scratch are sized for (0 = A * k: every filtered point)
  int tune_large_kernel = 0;  // batched odometry, submap_scan_size > 7: 0 = the 512-thread kernel of register_step_large.hip when the sequences fit the chip at one per compute unit, 1 = never, 2 = always
  int tune_voxel_order = 0;  // per-call scans: 0 = a voxel's points summed in index order (production: the stable order), 1 = in the order libstdc++'s std::sort leaves them (PCL <= 1.9)
  int tune_nn_tie = 0;  // which of several exactly equidistant cells GetClosestIdx returns: 0 lowest index (production), 1 highest, 2 FLANN's kd-tree order (parity mode, slow)
  int tune_repeat_shortcut = 1;  // registration: an outer iteration that would repeat the previous one bit for bit is not recomputed (0: it is - tests)
  int tune_replay_persistent_max = 256;  // cfear_odometry_replay_host: up to this many sequences run as persistent workgroups (replay.hip)
  // Device blocks handed back by cfear_cloud_release / cfear_scan_release, reused by the next allocation of a similar size (round 6): the
  // per-call route (radarDriver -> Compensate -> MapPointNormal -> Register, include/cfear_hip/cfear_host.hpp) creates and drops two clouds
  // and a scan per sweep, and hipMalloc / hipFree (the latter a device-wide synchronisation) cost more than its kernels. Reuse is
  // stream-ordered: every per-call entry point works on ctx->stream (a context with odometry objects on streams of their own keeps the
  // synchronising release).
  std::vector<std::pair<size_t, void*>> pool;
  size_t pool_bytes = 0;
  std::vector<std::pair<size_t, void*>> hpool;  // ... and the pinned host blocks of the clouds' mirrors
  Stream own_stream;  // the stream of a context that was given none (a caller's stream is never destroyed)
  Event ev0, ev1;     // cfear_time_kstrongest (timing events)
  // pinned host staging of the per-call entry points: downloads that complete with ONE synchronisation, registration arguments in one copy
  PinnedBuf<unsigned char> h_stage;
  // pinned staging of one polar image for callers that hand over pageable memory (cfear_upload_image), and the event after its last copy
  PinnedBuf<unsigned char> h_img;
  Event ev_img;
  bool ev_img_pending = false;
};

static inline int cfear_fail(cfear_ctx* c, int code, const char* what, hipError_t e) {
  if (c) {
    char buf[512];
    if (e != hipSuccess)
      snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
    else
      snprintf(buf, sizeof(buf), "%s", what);
    c->err = buf;
  }
  return code;
}

#define CFEAR_HIP_CHECK(ctx, call)                                            \
  do {                                                                        \
    hipError_t _e = (call);                                                   \
    if (_e != hipSuccess) return cfear_fail((ctx), CFEAR_ERR_HIP, #call, _e); \
  } while (0)

// a step that reports through cfear_fail itself: hand its code on
#define CFEAR_TRY(expr)                   \
  do {                                    \
    const int _rc = (expr);               \
    if (_rc != CFEAR_OK) return _rc;      \
  } while (0)

struct cfear_cloud {  // pcl::PointCloud<pcl::PointXYZI> on the device: one block, the count in its first 16 bytes
  int cap = 0;
  float* d_xyi = nullptr;  // [cap][3] x, y, intensity (= block + 16)
  int* d_n = nullptr;      // point count (= block)
  void* block = nullptr;
  size_t bytes = 0;
  // Host mirror (round 6): a pinned, device-visible copy of the block that the kernels producing or changing the cloud on the per-call route write as
  // well - cfear_clouds_download then is a wait and a memcpy, no copy command (kernel + D2H + wait 21 us, kernel writing host memory + wait 13 us:
  // profiles/r06_sync_latency.txt; the per-call route downloads four clouds a sweep). mirror_valid: the mirror holds what the device block holds.
  unsigned char* h_block = nullptr;
  size_t h_bytes = 0;
  bool mirror_valid = false;
  int* h_n() const { return reinterpret_cast<int*>(h_block); }
  float* h_xyi() const { return reinterpret_cast<float*>(h_block + 16); }
};

// cabi.hip
extern "C" __attribute__((visibility("hidden"))) int cfear_ensure_staging(cfear_ctx* ctx, int n_scans);
extern "C" __attribute__((visibility("hidden"))) int cfear_pool_alloc(cfear_ctx* ctx, size_t bytes, void** out, size_t* got);
extern "C" __attribute__((visibility("hidden"))) void cfear_pool_free(cfear_ctx* ctx, void* p, size_t bytes);
extern "C" __attribute__((visibility("hidden"))) int cfear_ensure_hstage(cfear_ctx* ctx, size_t bytes);
extern "C" __attribute__((visibility("hidden"))) void* cfear_hpool_alloc(cfear_ctx* ctx, size_t bytes, size_t* got);  // null: no mirror (not an error)
extern "C" __attribute__((visibility("hidden"))) void cfear_hpool_free(cfear_ctx* ctx, void* p, size_t bytes);
extern "C" __attribute__((visibility("hidden"))) int cfear_upload_image(cfear_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
// one axis of a cost surface around v0: the coordinates of the cells the reference's loop visits into out[0 .. pixels) (null: only counted); their number
extern "C" __attribute__((visibility("hidden"))) int cfear_surface_axis(double v0, double res, int width, int pixels, double* out);
static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// percall.hip: the per-call API (its kernels are pipeline.hip's, behind pipeline_launch.h). What other units need of it: a cloud ...
extern "C" __attribute__((visibility("hidden"))) int cfear_cloud_alloc(cfear_ctx* ctx, int cap, cfear_cloud** out);
// ... and a blank per-call scan of cap_points points and cap_cells cells (their cfear_cell records included; with_kd: and the kd-tree's arrays):
// the handle, its block of the context's pool (*d_block) and in *hdr the header that belongs at the block's front. n_cells: what
// cfear_scan_size answers without a round trip (-1: not known before the scan is built). With cfear_scan_release all another unit needs of a scan.
namespace cfear_dev { struct ScanDev; }
extern "C" __attribute__((visibility("hidden"))) int cfear_scan_alloc(cfear_ctx* ctx, int cap_points, int cap_cells, bool with_kd, int n_cells, cfear_scan** out,
                                                                      cfear_dev::ScanDev** d_block, cfear_dev::ScanDev* hdr);
// ... and the bytes of its block (what a call that builds scans of its own reports to the tools)
extern "C" __attribute__((visibility("hidden"))) size_t cfear_scan_bytes(const cfear_scan* s);
// kstrongest.hip
__attribute__((visibility("hidden"))) int cfear_launch_kstrongest(cfear_ctx* ctx, const uint8_t* d_polar, int n_scans, uint32_t* d_slots, hipStream_t stream,
                                                                   bool peaks /* false: slots nobody reads bit 25 of (the batched odometry routes) - written 0, no suppression */,
                                                                   int u_zmin_override = -1 /* >= 0: this threshold instead of the context's z_min */);

// cfar.hip
__attribute__((visibility("hidden"))) int cfear_launch_cfar_batch(cfear_ctx* ctx, const uint8_t* d_polar, int n_scans, int window_size, int nb_guard_cells,
                                                                  float false_alarm_rate, double max_distance, float* d_xyi, int capacity, int* d_counts,
                                                                  int* d_rows /* cfear_cfar_scratch_ints(ctx, n_scans) ints */, hipStream_t stream);
__attribute__((visibility("hidden"))) size_t cfear_cfar_scratch_ints(const cfear_ctx* ctx, size_t n_scans);
// ... several detectors over shared source images (cfar_grid.h): the plan of a (dets, source) pair and its tables on the device. `what`
// prefixes the message of a refused value (CFEAR_ERR_INVALID: the cloud and the field named). The streams that read a grid are idle when
// it is destroyed.
struct cfear_cfar_grid;
__attribute__((visibility("hidden"))) int cfear_cfar_grid_create(cfear_ctx* ctx, const cfear_seq_detector* dets, const int32_t* source, int n_clouds, int n_sources,
                                                                 const char* what, cfear_cfar_grid** out);
__attribute__((visibility("hidden"))) void cfear_cfar_grid_destroy(cfear_cfar_grid* g);
__attribute__((visibility("hidden"))) size_t cfear_cfar_grid_scratch_ints(const cfear_ctx* ctx, const cfear_cfar_grid* g, size_t n_steps);
// n_steps sweeps of g's n_sources images each -> n_steps x n_clouds clouds (step-major) of `capacity` points each and their true counts
__attribute__((visibility("hidden"))) int cfear_launch_cfar_grid(cfear_ctx* ctx, const cfear_cfar_grid* g, const uint8_t* d_polar, int n_steps, double max_distance,
                                                                 float* d_xyi, int capacity, int* d_counts,
                                                                 int* d_rows /* cfear_cfar_grid_scratch_ints(ctx, g, n_steps) ints */, hipStream_t stream);

// scans (keyframes + current) the batched registration kernels of register_step.hip are compiled for: pipeline.hip launches them
// when submap_scan_size + 1 fits, its own 64-scan instantiation otherwise
#define CFEAR_STEP_SMALL_SCANS 8
