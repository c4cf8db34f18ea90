// percall.hip -- the per-call C API: clouds, scans, Register / RegisterTimeContinuous, GetCost, GetSurface and the cost-sampling covariance.
// Host code only: the kernels are pipeline.hip's, run through its launch functions (pipeline_launch.h); the layouts of a scan block and of
// the context scratch are scan_layout.h's; the sample design and the fit of the covariance are cov_design.h's. Interface contract +
// reference citations: include/cfear_hip.h.
#include <math.h>
#include <cmath>
#include <stdlib.h>

#include <algorithm>
#include <new>

#include "scan_layout.h"
#include "pipeline_launch.h"
#include "cov_sampling_dev.h"
#include "cov_design.h"

// cfear_tune NN_TIE_RULE = 2 needs scans that were built in that mode: anything else would answer by the production rule without saying so
static int check_tie_rule_scans(cfear_ctx* ctx, cfear_scan* const* scans, int n, const char* what) {
  if (ctx->tune_nn_tie != 2) return CFEAR_OK;
  for (int i = 0; i < n; i++)
    if (scans[i] && !scans[i]->with_kd) {
      char msg[256];
      snprintf(msg, sizeof(msg), "%s: scan %d was created before cfear_tune NN_TIE_RULE = 2 was set - it has no kd-tree for the parity mode's search; create the scans after the tune call", what, i);
      return cfear_fail(ctx, CFEAR_ERR_INVALID, msg);
    }
  return CFEAR_OK;
}

// What a per-call problem (Register / GetCost / GetSurface) keeps on the device behind the working arrays of the context scratch
struct CallTail {
  double poses[3 * MAX_SCANS];
  double cov[36];  // cfear_register: the covariance, in and out; cfear_get_cost: the score, then the residual count; cfear_get_surface: the prior
  ScanDev* ptrs[MAX_SCANS];
  alignas(16) cfear_reg_summary sum;  // (up to here cfear_register copies in one piece, each way)
  alignas(16) double prior[36];       // cfear_register_soft
};
static_assert(offsetof(CallTail, sum) == sizeof(double) * (3 * MAX_SCANS + 36) + sizeof(void*) * MAX_SCANS, "the arrays that travel as one copy lie back to back");
// cfear_register_time_continuous: the compensated source view (registration_dev.h) of a scan of up to view_cells cells and its header
struct TcView { ScanDev* hdr; double* view; int view_cells; };
// per-context scratch of the per-call API for scans of up to cap_points points and up to MAX_SCANS - 1 keyframes: the working arrays (B), then a CallTail,
// then a TcView
static int ensure_ctx_scratch(cfear_ctx* ctx, int cap_points, BlockScratch* B, CallTail** tail = nullptr, TcView* tc = nullptr) {
  const int pair_cap = (MAX_SCANS - 1) * cap_points;
  const ScratchLayout L = scratch_layout(cap_points, pair_cap);
  const size_t tc_hdr = align_up(L.total + sizeof(CallTail), 256), tc_view = align_up(tc_hdr + sizeof(ScanDev), 256);
  const size_t need = tc_view + sizeof(double) * 8 * (size_t)cap_points + 4096;  // (and some headroom)
  CFEAR_TRY(ctx->d_scratch.ensure(ctx, need, "hipMalloc context scratch", true));  // dense voxel table starts all-zero
  unsigned char* base = ctx->d_scratch;
  *B = scratch_header(base, cap_points, pair_cap);
  if (tail) *tail = reinterpret_cast<CallTail*>(base + L.total);
  if (tc) { tc->hdr = reinterpret_cast<ScanDev*>(base + tc_hdr); tc->view = reinterpret_cast<double*>(base + tc_view); tc->view_cells = cap_points; }
  return CFEAR_OK;
}
// the scans of a per-call problem: all there and built under the current tie rule; their device blocks and the largest point capacity among them
static int problem_scans(cfear_ctx* ctx, cfear_scan* const* scans, int n, const char* what, ScanDev** ptrs, int* capmax) {
  *capmax = ctx->A * ctx->par.k_strongest;
  for (int i = 0; i < n; i++) {
    if (!scans[i]) {
      char msg[64];
      snprintf(msg, sizeof(msg), "%s: null scan", what);
      return cfear_fail(ctx, CFEAR_ERR_INVALID, msg);
    }
    if (scans[i]->cap_points > *capmax) *capmax = scans[i]->cap_points;
    ptrs[i] = reinterpret_cast<ScanDev*>(scans[i]->d_block);
  }
  return check_tie_rule_scans(ctx, scans, n, what);
}
// ... with the context scratch sized for them: the kernels' working memory, the device tail (d) and the scan pointer table to upload into it
struct CallProblem { BlockScratch B; CallTail* d; ScanDev* ptrs[MAX_SCANS]; TcView tc; };
static int call_problem(cfear_ctx* ctx, cfear_scan* const* scans, int n, const char* what, CallProblem* pb) {
  int capmax = 0;
  CFEAR_TRY(problem_scans(ctx, scans, n, what, pb->ptrs, &capmax));
  return ensure_ctx_scratch(ctx, capmax, &pb->B, &pb->d, &pb->tc);
}
// the pointer table and the poses of a problem from the caller's memory to the device, on the context stream (GetCost / GetSurface / the
// cost-sampling covariance; cfear_register sends them through the pinned staging instead)
static hipError_t upload_problem(cfear_ctx* ctx, ScanDev** d_ptrs, ScanDev* const* h_ptrs, double* d_poses, const double* poses_xyt, int n) {
  const hipError_t e = hipMemcpyAsync(d_ptrs, h_ptrs, sizeof(void*) * n, hipMemcpyHostToDevice, ctx->stream);
  return e != hipSuccess ? e : hipMemcpyAsync(d_poses, poses_xyt, sizeof(double) * 3 * n, hipMemcpyHostToDevice, ctx->stream);
}
// a HIP call of an entry point that reports its failures under its own name (CFEAR_HIP_CHECK reports the call's text)
#define CFEAR_HIP_CHECK_AS(ctx, what, call)                                   \
  do {                                                                        \
    const hipError_t _e = (call);                                             \
    if (_e != hipSuccess) return cfear_fail((ctx), CFEAR_ERR_HIP, what, _e);  \
  } while (0)

extern "C" {

// ---- clouds ------------------------------------------------------------------------------------
__attribute__((visibility("hidden"))) int cfear_cloud_alloc(cfear_ctx* ctx, int cap, cfear_cloud** out) {
  cfear_cloud* c = new (std::nothrow) cfear_cloud();
  if (!c) return cfear_fail(ctx, CFEAR_ERR_NOMEM, "cloud alloc");
  c->cap = cap > 0 ? cap : 1;
  const int rc = cfear_pool_alloc(ctx, 16 + sizeof(float) * 3 * (size_t)c->cap, &c->block, &c->bytes);  // one block from the context's pool
  if (rc != CFEAR_OK) { delete c; return rc; }
  c->d_n = static_cast<int*>(c->block);
  c->d_xyi = reinterpret_cast<float*>(static_cast<unsigned char*>(c->block) + 16);
  c->h_block = static_cast<unsigned char*>(cfear_hpool_alloc(ctx, 16 + sizeof(float) * 3 * (size_t)c->cap, &c->h_bytes));
  *out = c;
  return CFEAR_OK;
}

void cfear_cloud_release(cfear_ctx* ctx, cfear_cloud* c) {
  if (!c) return;
  cfear_pool_free(ctx, c->block, c->bytes);  // (stream-ordered reuse; no synchronisation, no hipFree on the per-sweep path)
  cfear_hpool_free(ctx, c->h_block, c->h_bytes);
  delete c;
}

int cfear_filter_polar_device(cfear_ctx* ctx, const uint8_t* d_polar, cfear_cloud** cloud, cfear_cloud** cloud_peaks) {
  if (!ctx || !d_polar || !cloud) return cfear_fail(ctx, CFEAR_ERR_INVALID, "filter_polar: bad argument");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  *cloud = nullptr;
  if (cloud_peaks) *cloud_peaks = nullptr;
  int rc = cfear_ensure_staging(ctx, 1);
  if (rc != CFEAR_OK) return rc;
  rc = cfear_launch_kstrongest(ctx, d_polar, 1, ctx->d_slots, ctx->stream, true);  // radar_driver.cpp:58 (with the flag: the peaks cloud reads it)
  if (rc != CFEAR_OK) return rc;
  const int A = ctx->A, k = ctx->par.k_strongest, cap = A * k;
  cfear_cloud *c0 = nullptr, *c1 = nullptr;  // radar_driver.cpp:59-60
  rc = cfear_cloud_alloc(ctx, cap, &c0);
  if (rc != CFEAR_OK) return rc;
  if (cloud_peaks) { rc = cfear_cloud_alloc(ctx, cap, &c1); if (rc != CFEAR_OK) { cfear_cloud_release(ctx, c0); return rc; } }
  cfear_launch_cloud(ctx->d_slots, A, k, ctx->d_trig, ctx->par.range_res, ctx->par.min_distance, c0, c1, ctx->stream);
  c0->mirror_valid = c0->h_block != nullptr;
  *cloud = c0;
  if (c1) { c1->mirror_valid = c1->h_block != nullptr; *cloud_peaks = c1; }
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  return CFEAR_OK;
}

int cfear_filter_polar(cfear_ctx* ctx, const uint8_t* h_polar, cfear_cloud** cloud, cfear_cloud** cloud_peaks) {
  if (!ctx || !h_polar || !cloud) return cfear_fail(ctx, CFEAR_ERR_INVALID, "filter_polar: bad argument");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int rc = cfear_ensure_staging(ctx, 1);
  if (rc != CFEAR_OK) return rc;
  rc = cfear_upload_image(ctx, ctx->d_polar, h_polar, (size_t)ctx->A * ctx->R);
  if (rc != CFEAR_OK) return rc;
  return cfear_filter_polar_device(ctx, ctx->d_polar, cloud, cloud_peaks);
}

int cfear_cloud_upload(cfear_ctx* ctx, const float* xyi, int n, cfear_cloud** cloud) {
  if (!ctx || !cloud || n < 0 || (n > 0 && !xyi)) return cfear_fail(ctx, CFEAR_ERR_INVALID, "cloud_upload: bad argument");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  cfear_cloud* c = nullptr;
  int rc = cfear_cloud_alloc(ctx, n, &c);
  if (rc != CFEAR_OK) return rc;
  hipError_t e = hipSuccess;
  if (n > 0) e = hipMemcpyAsync(c->d_xyi, xyi, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(c->d_n, &n, sizeof(int), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) { cfear_cloud_release(ctx, c); return cfear_fail(ctx, CFEAR_ERR_HIP, "cloud_upload", e); }
  if (c->h_block) { *c->h_n() = n; if (n > 0) memcpy(c->h_xyi(), xyi, sizeof(float) * 3 * (size_t)n); c->mirror_valid = true; }
  *cloud = c;
  return CFEAR_OK;
}

int cfear_cloud_size(cfear_ctx* ctx, const cfear_cloud* c, int* n) {
  if (!ctx || !c || !n) return cfear_fail(ctx, CFEAR_ERR_INVALID, "cloud_size: bad argument");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (c->mirror_valid) { CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream)); *n = *c->h_n(); return CFEAR_OK; }
  CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(n, c->d_n, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return CFEAR_OK;
}

// m clouds to the host with ONE synchronisation: count and points of every cloud travel together into pinned staging, the first
// min(n, capacity) points are handed on (the per-sweep route downloads cloud and cloud_peaks, radar_driver.cpp:59-60 / utils.cpp:96-113)
int cfear_clouds_download(cfear_ctx* ctx, const cfear_cloud* const* clouds, int m, float* const* xyi, const int* capacity, int* n) {
  if (!ctx || !clouds || m <= 0 || m > 16) return cfear_fail(ctx, CFEAR_ERR_INVALID, "clouds_download: bad argument");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  size_t off[17]; off[0] = 0;
  for (int i = 0; i < m; i++) {
    if (!clouds[i]) return cfear_fail(ctx, CFEAR_ERR_INVALID, "clouds_download: null cloud");
    const int want = (xyi && xyi[i] && capacity) ? (capacity[i] < clouds[i]->cap ? capacity[i] : clouds[i]->cap) : 0;
    off[i + 1] = off[i] + ((16 + sizeof(float) * 3 * (size_t)(want > 0 ? want : 0) + 63) & ~(size_t)63);
  }
  bool all_mirrored = true;
  for (int i = 0; i < m; i++) all_mirrored = all_mirrored && clouds[i]->mirror_valid;
  if (all_mirrored) {  // the kernels wrote the host copies: wait for them, hand the points on
    CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < m; i++) {
      const int cnt = *clouds[i]->h_n();
      if (n) n[i] = cnt;
      const int want = (xyi && xyi[i] && capacity) ? (capacity[i] < clouds[i]->cap ? capacity[i] : clouds[i]->cap) : 0;
      const int take = cnt < want ? cnt : want;
      if (take > 0) memcpy(xyi[i], clouds[i]->h_xyi(), sizeof(float) * 3 * (size_t)take);
    }
    return CFEAR_OK;
  }
  int rc = cfear_ensure_hstage(ctx, off[m]);
  if (rc != CFEAR_OK) return rc;
  for (int i = 0; i < m; i++) {
    const int want = (xyi && xyi[i] && capacity) ? (capacity[i] < clouds[i]->cap ? capacity[i] : clouds[i]->cap) : 0;
    CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(ctx->h_stage + off[i], clouds[i]->block, 16 + sizeof(float) * 3 * (size_t)(want > 0 ? want : 0), hipMemcpyDeviceToHost, ctx->stream));
  }
  CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < m; i++) {
    const int cnt = *reinterpret_cast<const int*>(ctx->h_stage + off[i]);
    if (n) n[i] = cnt;
    const int want = (xyi && xyi[i] && capacity) ? (capacity[i] < clouds[i]->cap ? capacity[i] : clouds[i]->cap) : 0;
    const int take = cnt < want ? cnt : want;
    if (take > 0) memcpy(xyi[i], ctx->h_stage + off[i] + 16, sizeof(float) * 3 * (size_t)take);
  }
  return CFEAR_OK;
}

int cfear_cloud_download(cfear_ctx* ctx, const cfear_cloud* c, float* xyi, int capacity, int* n) {
  if (!ctx || !c) return cfear_fail(ctx, CFEAR_ERR_INVALID, "cloud_download: bad argument");
  return cfear_clouds_download(ctx, &c, 1, &xyi, &capacity, n);
}

int cfear_compensate(cfear_ctx* ctx, cfear_cloud* c, const double motion_xyt[3], int ccw) {
  if (!ctx || !c || !motion_xyt) return cfear_fail(ctx, CFEAR_ERR_INVALID, "compensate: bad argument");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  // Affine3dToVectorXYeZ of the motion (utils.cpp:109-112): theta passes through atan2(sin, cos)
  const double th = atan2(sin(motion_xyt[2]), cos(motion_xyt[2]));
  cfear_launch_compensate(c, nullptr, motion_xyt[0], motion_xyt[1], th, ccw, ctx->stream);
  c->mirror_valid = c->h_block != nullptr;
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  return CFEAR_OK;
}

int cfear_compensate_pair(cfear_ctx* ctx, cfear_cloud* c0, cfear_cloud* c1, const double motion_xyt[3], int ccw) {
  if (!ctx || !c0 || !c1 || c0 == c1 || !motion_xyt) return cfear_fail(ctx, CFEAR_ERR_INVALID, "compensate_pair: bad argument");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const double th = atan2(sin(motion_xyt[2]), cos(motion_xyt[2]));
  cfear_launch_compensate(c0, c1, motion_xyt[0], motion_xyt[1], th, ccw, ctx->stream);
  c0->mirror_valid = c0->h_block != nullptr; c1->mirror_valid = c1->h_block != nullptr;
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  return CFEAR_OK;
}

// ---- scans -------------------------------------------------------------------------------------
}  // extern "C"
// cfear_tune VOXEL_ORDER = 1: the order PCL <= 1.9 leaves the points of a VoxelGrid voxel in (pointnormal.cpp:277-280 -> pcl::VoxelGrid::applyFilter).
// pcl/filters/impl/voxel_grid.hpp fills a vector of (voxel index, point index) in point order and calls std::sort on it with an operator<
// that compares the voxel index ONLY - an unstable sort, so the order of a voxel's points, and with it the last bit of its float centroid,
// is whatever libstdc++'s introsort leaves. Reproducing that needs the same call on the same sequence: the cloud comes to the host, the
// voxel indices are formed with the kernel's (= PCL's) float arithmetic, std::sort runs here, and the device gets every point's rank
// (features_dev.h: the sort key inside a voxel) and the point at every rank. Per-call scans only (a host round trip per scan: parity mode).
namespace {
struct cloud_point_index_idx {
  unsigned int idx, cloud_point_index;
  bool operator<(const cloud_point_index_idx& p) const { return idx < p.idx; }
};
int voxel_order_stdsort(cfear_ctx* ctx, const cfear_cloud* cloud, int cap_points, DevBuf<int>* d_out /* [2][n]: rank, perm; empty for an empty cloud */) {
  int n = 0;
  CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(&n, cloud->d_n, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  n = std::min(n, std::min(cloud->cap, cap_points));
  if (n <= 0) return CFEAR_OK;
  std::vector<float> xyi(3 * (size_t)n);
  CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(xyi.data(), cloud->d_xyi, sizeof(float) * xyi.size(), hipMemcpyDeviceToHost, ctx->stream));
  CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  const float leaf = (float)((double)(float)ctx->par.res / ctx->par.downsample_factor), inv = 1.0f / leaf;  // features_block
  float mnx = 3.4e38f, mxx = -3.4e38f, mny = 3.4e38f, mxy = -3.4e38f;
  for (int i = 0; i < n; i++) {
    const float x = xyi[3 * (size_t)i], y = xyi[3 * (size_t)i + 1];
    mnx = fminf(mnx, x); mxx = fmaxf(mxx, x); mny = fminf(mny, y); mxy = fmaxf(mxy, y);
  }
  const int min_b0 = (int)floorf(mnx * inv), max_b0 = (int)floorf(mxx * inv), min_b1 = (int)floorf(mny * inv);
  const int div0 = max_b0 - min_b0 + 1;
  std::vector<cloud_point_index_idx> v((size_t)n);
  for (int i = 0; i < n; i++) {
    const int ijk0 = (int)(floorf(xyi[3 * (size_t)i] * inv) - (float)min_b0), ijk1 = (int)(floorf(xyi[3 * (size_t)i + 1] * inv) - (float)min_b1);
    v[(size_t)i].idx = (unsigned int)(ijk0 + ijk1 * div0); v[(size_t)i].cloud_point_index = (unsigned int)i;
  }
  std::sort(v.begin(), v.end(), std::less<cloud_point_index_idx>());
  std::vector<int> rp(2 * (size_t)n);
  for (int r = 0; r < n; r++) { rp[(size_t)v[(size_t)r].cloud_point_index] = r; rp[(size_t)n + r] = (int)v[(size_t)r].cloud_point_index; }
  DevBuf<int> d;
  CFEAR_TRY(d.ensure(ctx, rp.size(), "hipMalloc voxel order"));
  hipError_t e = hipMemcpyAsync(d, rp.data(), sizeof(int) * rp.size(), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // (rp is a local)
  if (e != hipSuccess) return cfear_fail(ctx, CFEAR_ERR_HIP, "voxel order upload", e);
  *d_out = std::move(d);
  return n;
}
}  // namespace
extern "C" {
// a blank per-call scan (common.h)
__attribute__((visibility("hidden"))) int cfear_scan_alloc(cfear_ctx* ctx, int cap_points, int cap_cells, bool with_kd, int n_cells, cfear_scan** out, ScanDev** d_block,
                                                           ScanDev* hdr) {
  cfear_scan* s = new (std::nothrow) cfear_scan();
  if (!s) return cfear_fail(ctx, CFEAR_ERR_NOMEM, "scan alloc");
  s->cap_points = cap_points; s->with_kd = with_kd; s->n_cells = n_cells;
  void* blk = nullptr;
  const int rc = cfear_pool_alloc(ctx, scan_layout(cap_points, cap_cells, true, with_kd).total, &blk, &s->bytes);
  if (rc != CFEAR_OK) { delete s; return rc; }
  s->d_block = static_cast<unsigned char*>(blk);
  *hdr = scan_header(s->d_block, cap_points, cap_cells, true, with_kd);
  *d_block = reinterpret_cast<ScanDev*>(s->d_block);
  *out = s;
  return CFEAR_OK;
}
__attribute__((visibility("hidden"))) size_t cfear_scan_bytes(const cfear_scan* s) { return s ? s->bytes : 0; }

int cfear_scan_create(cfear_ctx* ctx, const cfear_cloud* cloud, cfear_scan** scan) {
  if (!ctx || !cloud || !scan) return cfear_fail(ctx, CFEAR_ERR_INVALID, "scan_create: bad argument");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  *scan = nullptr;
  const int cap = cloud->cap;
  if (cap >= (1 << 24)) return cfear_fail(ctx, CFEAR_ERR_UNSUPPORTED, "scan_create: more than 2^24 points");
  BlockScratch B;
  int rc = ensure_ctx_scratch(ctx, std::max(cap, ctx->A * ctx->par.k_strongest), &B);
  if (rc != CFEAR_OK) return rc;
  cfear_scan* s = nullptr;
  ScanDev* d_scan = nullptr;
  ScanDev h, back;
  CFEAR_TRY(cfear_scan_alloc(ctx, cap, cap, ctx->tune_nn_tie == 2, -1, &s, &d_scan, &h));
  DevBuf<int> d_vorder;  // (freed on every way out, each of them behind the synchronisation below)
  // the header goes in and comes back through the context's pinned staging (from / to the stack the two small copies are pageable: the runtime
  // stages and waits for each - on the per-sweep route two of the ~15 host round trips of a sweep)
  constexpr size_t HS = (sizeof(ScanDev) + 63) & ~(size_t)63;
  rc = cfear_ensure_hstage(ctx, 2 * HS);
  if (rc != CFEAR_OK) { cfear_scan_release(ctx, s); return rc; }
  memcpy(ctx->h_stage, &h, sizeof(h));
  hipError_t e = hipMemcpyAsync(d_scan, ctx->h_stage, sizeof(h), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    if (ctx->tune_voxel_order == 1) {  // PCL <= 1.9's intra-voxel order (parity mode): ranks from a host std::sort
      const int nv = voxel_order_stdsort(ctx, cloud, cap, &d_vorder);
      if (nv < 0) { cfear_scan_release(ctx, s); return nv; }
      if (d_vorder) { B.vrank = d_vorder; B.vperm = d_vorder + nv; }
    }
    cfear_launch_features(d_scan, cloud->d_xyi, cloud->d_n, feature_params(ctx), B, ctx->stream);
    e = hipGetLastError();
  }
  // the reference exits on an empty cloud (pointnormal.cpp:72-75); report it instead
  if (e == hipSuccess) e = hipMemcpyAsync(ctx->h_stage + HS, d_scan, sizeof(back), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) memcpy(&back, ctx->h_stage + HS, sizeof(back));
  if (e != hipSuccess) { cfear_scan_release(ctx, s); return cfear_fail(ctx, CFEAR_ERR_HIP, "scan_create", e); }
  if (back.status != 0) { cfear_scan_release(ctx, s); return cfear_fail(ctx, CFEAR_ERR_EMPTY, "scan_create: empty cloud (reference: 'error, cloud empty' + exit)"); }
  s->n_cells = back.n_cells;
  *scan = s;
  return CFEAR_OK;
}

int cfear_scan_from_cells(cfear_ctx* ctx, const cfear_cell* cells, int n, cfear_scan** scan) {
  if (!ctx || !scan || n < 0 || (n > 0 && !cells)) return cfear_fail(ctx, CFEAR_ERR_INVALID, "scan_from_cells: bad argument");
  if (n >= (1 << 24)) return cfear_fail(ctx, CFEAR_ERR_UNSUPPORTED, "scan_from_cells: more than 2^24 cells");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  *scan = nullptr;
  if (n == 0) return cfear_fail(ctx, CFEAR_ERR_EMPTY, "scan_from_cells: no cells (reference: 'error, cloud empty' + exit)");
  BlockScratch B;
  int rc = ensure_ctx_scratch(ctx, std::max(n, ctx->A * ctx->par.k_strongest), &B);
  if (rc != CFEAR_OK) return rc;
  cfear_scan* s = nullptr;
  ScanDev* d_scan = nullptr;
  ScanDev h;
  CFEAR_TRY(cfear_scan_alloc(ctx, n, n, ctx->tune_nn_tie == 2, n, &s, &d_scan, &h));
  hipError_t e = hipMemcpyAsync(d_scan, &h, sizeof(h), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(h.cells, cells, sizeof(cfear_cell) * (size_t)n, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    cfear_launch_scan_from_cells(d_scan, n, feature_params(ctx), B, ctx->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // h and the caller's cells are read until here
  if (e != hipSuccess) { cfear_scan_release(ctx, s); return cfear_fail(ctx, CFEAR_ERR_HIP, "scan_from_cells", e); }
  *scan = s;
  return CFEAR_OK;
}

void cfear_scan_release(cfear_ctx* ctx, cfear_scan* s) {
  if (!s) return;
  cfear_pool_free(ctx, s->d_block, s->bytes);  // back to the context's pool (stream-ordered reuse, no synchronisation)
  delete s;
}

static int scan_header_download(cfear_ctx* ctx, const cfear_scan* s, ScanDev* h) {
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(h, s->d_block, sizeof(ScanDev), hipMemcpyDeviceToHost, ctx->stream));
  CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return CFEAR_OK;
}

int cfear_scan_size(cfear_ctx* ctx, const cfear_scan* s, int* n_cells) {
  if (!ctx || !s || !n_cells) return cfear_fail(ctx, CFEAR_ERR_INVALID, "scan_size: bad argument");
  if (s->n_cells >= 0) { *n_cells = s->n_cells; return CFEAR_OK; }  // cfear_scan_create read the header back already
  ScanDev h;
  int rc = scan_header_download(ctx, s, &h);
  if (rc != CFEAR_OK) return rc;
  *n_cells = h.n_cells;
  return CFEAR_OK;
}

int cfear_scan_download_cells(cfear_ctx* ctx, const cfear_scan* s, cfear_cell* cells, int capacity, int* n) {
  if (!ctx || !s) return cfear_fail(ctx, CFEAR_ERR_INVALID, "scan_download_cells: bad argument");
  ScanDev h;
  int rc = scan_header_download(ctx, s, &h);
  if (rc != CFEAR_OK) return rc;
  if (n) *n = h.n_cells;
  const int cnt = h.n_cells < capacity ? h.n_cells : capacity;
  if (cnt > 0 && cells) {
    CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(cells, h.cells, sizeof(cfear_cell) * (size_t)cnt, hipMemcpyDeviceToHost, ctx->stream));
    CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  }
  return CFEAR_OK;
}

int cfear_scan_closest(cfear_ctx* ctx, const cfear_scan* s, const double* qxy, int nq, double d, int32_t* idx) {
  if (!ctx || !s || !qxy || !idx || nq <= 0) return cfear_fail(ctx, CFEAR_ERR_INVALID, "scan_closest: bad argument");
  { cfear_scan* one = const_cast<cfear_scan*>(s); const int trc = check_tie_rule_scans(ctx, &one, 1, "scan_closest"); if (trc != CFEAR_OK) return trc; }
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  DevBuf<double> dq; DevBuf<int> di;
  CFEAR_TRY(dq.ensure(ctx, 2 * (size_t)nq, "hipMalloc queries"));
  CFEAR_TRY(di.ensure(ctx, (size_t)nq, "hipMalloc idx"));
  hipError_t e = hipMemcpyAsync(dq, qxy, sizeof(double) * 2 * (size_t)nq, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    cfear_launch_closest(reinterpret_cast<const ScanDev*>(s->d_block), dq, nq, d, di, ctx->tune_nn_tie, ctx->stream);
    e = hipMemcpyAsync(idx, di, sizeof(int) * (size_t)nq, hipMemcpyDeviceToHost, ctx->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return cfear_fail(ctx, CFEAR_ERR_HIP, "scan_closest", e);
  return CFEAR_OK;
}

// ---- registration ------------------------------------------------------------------------------
// vel: null = Register; the sweep velocity (vx, vy, vtheta) = RegisterTimeContinuous with that velocity and rotation direction
static int register_impl(cfear_ctx* ctx, cfear_scan* const* scans, int n, double* poses_xyt, const double* prior_cov6, double* cov6_last,
                         cfear_reg_summary* summary, const double* vel = nullptr, int ccw = 0) {
  if (!ctx || !scans || !poses_xyt || n < 2) return cfear_fail(ctx, CFEAR_ERR_INVALID, "register: need >= 2 scans and poses");
  if (n > MAX_SCANS) return cfear_fail(ctx, CFEAR_ERR_UNSUPPORTED, "register: more than 64 scans");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  CallProblem pb;
  CFEAR_TRY(call_problem(ctx, scans, n, "register", &pb));
  // arguments and results travel through pinned staging laid out like the device tail: one copy each way and one synchronisation per
  // registration (round 6; it was three small pageable copies in, three out)
  CFEAR_TRY(cfear_ensure_hstage(ctx, sizeof(CallTail)));
  CallTail* h = reinterpret_cast<CallTail*>(static_cast<unsigned char*>(ctx->h_stage));
  const size_t in_bytes = offsetof(CallTail, sum);
  memset(h, 0, in_bytes);
  memcpy(h->ptrs, pb.ptrs, sizeof(void*) * n);
  memcpy(h->poses, poses_xyt, sizeof(double) * 3 * n);
  // a registration that fails does not touch the caller's covariance (reg_cov of n_scan_normal_reg::Register, n_scan_normal.cpp:82-187):
  // the device copy starts as the caller's matrix, so that what comes back is the caller's matrix (not the previous call's result)
  if (cov6_last) memcpy(h->cov, cov6_last, sizeof(double) * 36);
  CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(pb.d, h, in_bytes, hipMemcpyHostToDevice, ctx->stream));
  double* d_prior = nullptr;
  if (prior_cov6) {
    d_prior = pb.d->prior;
    memcpy(h->prior, prior_cov6, sizeof(double) * 36);
    CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(d_prior, h->prior, sizeof(double) * 36, hipMemcpyHostToDevice, ctx->stream));
  }
  TcLaunch tc;
  if (vel) {
    // (the cells of a scan are known on the host since its creation; a scan that does not know them yet is covered by its capacity)
    const int cells = scans[n - 1]->n_cells >= 0 ? scans[n - 1]->n_cells : scans[n - 1]->cap_points;
    tc = TcLaunch{pb.ptrs[n - 1], pb.tc.hdr, pb.tc.view, pb.tc.view_cells, cells, vel[0], vel[1], vel[2], ccw ? 1 : 0};
  }
  cfear_launch_register(pb.d->ptrs, n, pb.d->poses, pb.d->cov, reg_params(ctx), pb.B, &pb.d->sum, d_prior, vel ? &tc : nullptr, ctx->stream);
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(h, pb.d, in_bytes + sizeof(cfear_reg_summary), hipMemcpyDeviceToHost, ctx->stream));
  CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  memcpy(poses_xyt, h->poses, sizeof(double) * 3 * n);
  if (cov6_last) memcpy(cov6_last, h->cov, sizeof(double) * 36);
  if (summary) memcpy(summary, &h->sum, sizeof(cfear_reg_summary));
  if (h->sum.assoc_path < 0)  // (registration_dev.h: the kd descent's stack did not fit the match scratch)
    return cfear_fail(ctx, CFEAR_ERR_UNSUPPORTED, "register: NN_TIE_RULE could not be honoured for this problem size (match scratch too small for the kd-tree descent); the result used the production rule");
  return CFEAR_OK;
}

int cfear_register(cfear_ctx* ctx, cfear_scan* const* scans, int n, double* poses_xyt, double* cov6_last,
                   cfear_reg_summary* summary) {
  return register_impl(ctx, scans, n, poses_xyt, nullptr, cov6_last, summary);
}

int cfear_register_soft(cfear_ctx* ctx, cfear_scan* const* scans, int n, double* poses_xyt, const double* prior_cov6, double* cov6_last,
                        cfear_reg_summary* summary) {
  if (!prior_cov6) return cfear_fail(ctx, CFEAR_ERR_INVALID, "register_soft: null prior covariance");
  return register_impl(ctx, scans, n, poses_xyt, prior_cov6, cov6_last, summary);
}

int cfear_register_time_continuous(cfear_ctx* ctx, cfear_scan* const* scans, int n, double* poses_xyt, const double velocity_xyt[3], int ccw,
                                   const double* prior_cov6, double* cov6_last, cfear_reg_summary* summary) {
  if (!ctx || !velocity_xyt) return cfear_fail(ctx, CFEAR_ERR_INVALID, "register_time_continuous: null context or velocity");
  if (!std::isfinite(velocity_xyt[0]) || !std::isfinite(velocity_xyt[1]) || !std::isfinite(velocity_xyt[2]))
    return cfear_fail(ctx, CFEAR_ERR_INVALID, "register_time_continuous: the velocity is not finite");
  return register_impl(ctx, scans, n, poses_xyt, prior_cov6, cov6_last, summary, velocity_xyt, ccw);
}

int cfear_get_cost(cfear_ctx* ctx, cfear_scan* const* scans, int n, const double* poses_xyt, int itr, double* score, double* residuals,
                   int capacity, int* n_residuals) {
  if (!ctx || !scans || !poses_xyt || !score || !n_residuals || n < 2 || capacity < 0 || (capacity > 0 && !residuals))
    return cfear_fail(ctx, CFEAR_ERR_INVALID, "get_cost: need >= 2 scans, poses and output pointers");
  if (n > MAX_SCANS) return cfear_fail(ctx, CFEAR_ERR_UNSUPPORTED, "get_cost: more than 64 scans");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  CallProblem pb;
  CFEAR_TRY(call_problem(ctx, scans, n, "get_cost", &pb));
  double* d_score = pb.d->cov;
  int* d_nres = reinterpret_cast<int*>(d_score + 1);
  DevBuf<double> d_res;
  CFEAR_TRY(d_res.ensure(ctx, (size_t)capacity, "hipMalloc residuals"));
  CFEAR_HIP_CHECK_AS(ctx, "get_cost", upload_problem(ctx, pb.d->ptrs, pb.ptrs, pb.d->poses, poses_xyt, n));
  cfear_launch_get_cost(pb.d->ptrs, n, pb.d->poses, reg_params(ctx), pb.B, itr, d_score, d_res, capacity, d_nres, ctx->stream);
  CFEAR_HIP_CHECK_AS(ctx, "get_cost", hipGetLastError());
  int nres = -1;
  CFEAR_HIP_CHECK_AS(ctx, "get_cost", hipMemcpyAsync(score, d_score, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  CFEAR_HIP_CHECK_AS(ctx, "get_cost", hipMemcpyAsync(&nres, d_nres, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  CFEAR_HIP_CHECK_AS(ctx, "get_cost", hipStreamSynchronize(ctx->stream));
  if (nres > 0 && capacity > 0)
    CFEAR_HIP_CHECK_AS(ctx, "get_cost", hipMemcpy(residuals, d_res, sizeof(double) * (size_t)(nres < capacity ? nres : capacity), hipMemcpyDeviceToHost));
  *n_residuals = nres;
  if (nres < 0) return cfear_fail(ctx, CFEAR_ERR_EMPTY, "get_cost: too few residuals");  // GetCost returns false (:205-208)
  return CFEAR_OK;
}

// ---- cost surfaces (n_scan_normal.cpp:29-65; surface_dev.h) ---------------------------------------------
int cfear_get_surface(cfear_ctx* ctx, cfear_scan* const* scans, int n, const double* poses_xyt, const double* prior_cov6, int itr,
                      double res, int width, double* surface, int* nx, int* ny) {
  if (!ctx || !scans || !poses_xyt || !surface || n < 2) return cfear_fail(ctx, CFEAR_ERR_INVALID, "get_surface: need >= 2 scans, poses and an output");
  if (n > MAX_SCANS) return cfear_fail(ctx, CFEAR_ERR_UNSUPPORTED, "get_surface: more than 64 scans");
  int pixels = 0, vx = 0, vy = 0;
  {
    // the grid is centred on the round-tripped last pose (:44-45): Affine3dToVectorXYeZ keeps x and y as they are
    const int rc = cfear_surface_dims(res, width, poses_xyt[3 * (n - 1)], poses_xyt[3 * (n - 1) + 1], &pixels, &vx, &vy);
    if (rc == CFEAR_ERR_INVALID) return cfear_fail(ctx, rc, "get_surface: res must be finite and > 0, width >= 0");
    if (rc != CFEAR_OK) return cfear_fail(ctx, rc, "get_surface: more than CFEAR_SURFACE_MAX_SIDE pixels per side");
  }
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  CallProblem pb;
  CFEAR_TRY(call_problem(ctx, scans, n, "get_surface", &pb));
  double* d_prior = pb.d->cov;
  // header, coordinates, their counts and the surface: one allocation per call
  const size_t np = (size_t)pixels * pixels;
  const size_t hdr_b = (sizeof(SurfHdr) + 255) / 256 * 256, crd_b = (sizeof(double) * 2 * pixels + 255) / 256 * 256;
  DevBuf<unsigned char> buf;
  CFEAR_TRY(buf.ensure(ctx, hdr_b + crd_b + 256 + sizeof(double) * np, "hipMalloc surface"));
  unsigned char* d_buf = buf;
  SurfHdr* d_hdr = reinterpret_cast<SurfHdr*>(d_buf);
  double* d_coords = reinterpret_cast<double*>(d_buf + hdr_b);
  int* d_nxy = reinterpret_cast<int*>(d_buf + hdr_b + crd_b);
  double* d_out = reinterpret_cast<double*>(d_buf + hdr_b + crd_b + 256);
  std::vector<double> coords(2 * (size_t)pixels, 0.0);
  const int nxy[2] = {cfear_surface_axis(poses_xyt[3 * (n - 1)], res, width, pixels, coords.data()),
                      cfear_surface_axis(poses_xyt[3 * (n - 1) + 1], res, width, pixels, coords.data() + pixels)};
  CFEAR_HIP_CHECK_AS(ctx, "get_surface", upload_problem(ctx, pb.d->ptrs, pb.ptrs, pb.d->poses, poses_xyt, n));
  if (prior_cov6) CFEAR_HIP_CHECK_AS(ctx, "get_surface", hipMemcpyAsync(d_prior, prior_cov6, sizeof(double) * 36, hipMemcpyHostToDevice, ctx->stream));
  CFEAR_HIP_CHECK_AS(ctx, "get_surface", hipMemcpyAsync(d_coords, coords.data(), sizeof(double) * 2 * pixels, hipMemcpyHostToDevice, ctx->stream));
  CFEAR_HIP_CHECK_AS(ctx, "get_surface", hipMemcpyAsync(d_nxy, nxy, sizeof(nxy), hipMemcpyHostToDevice, ctx->stream));
  const RegParams P = reg_params(ctx);
  cfear_launch_surface_build(pb.d->ptrs, n, pb.d->poses, P, pb.B, itr, prior_cov6 ? d_prior : nullptr, d_hdr, d_coords, d_nxy, pixels, d_out, ctx->stream);
  CFEAR_HIP_CHECK_AS(ctx, "get_surface", hipGetLastError());
  if (!cfear_surface_build_evaluates()) {
    launch_surface_eval(P, 1, d_hdr, d_coords, d_nxy, pixels, d_out, ctx->stream);
    CFEAR_HIP_CHECK_AS(ctx, "get_surface", hipGetLastError());
  }
  CFEAR_HIP_CHECK_AS(ctx, "get_surface", hipMemcpyAsync(surface, d_out, sizeof(double) * np, hipMemcpyDeviceToHost, ctx->stream));
  CFEAR_HIP_CHECK_AS(ctx, "get_surface", hipStreamSynchronize(ctx->stream));
  if (nx) *nx = nxy[0];
  if (ny) *ny = nxy[1];
  return CFEAR_OK;
}

// ---- cost-sampling covariance (odometrykeyframefuser.cpp:261-380; the design and the fit: cov_design.h) ------------
int cfear_cov_by_sampling(cfear_ctx* ctx, cfear_scan* const* scans, int n, const double* poses_xyt, int itr, double xy_range,
                          double yaw_range, int samples_per_axis, double covariance_scaler, double final_cost, int num_residuals,
                          double* cov6, int* success, double* sample_costs) {
  if (!ctx || !scans || !poses_xyt || !cov6 || !success || n < 2 || samples_per_axis < 1 || samples_per_axis > 32)
    return cfear_fail(ctx, CFEAR_ERR_INVALID, "cov_by_sampling: bad argument");
  if (n > MAX_SCANS) return cfear_fail(ctx, CFEAR_ERR_UNSUPPORTED, "cov_by_sampling: more than 64 scans");
  *success = 0;
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  ScanDev* h_ptrs[MAX_SCANS];
  int capmax = 0;  // (not needed: the samples' match arrays are an allocation of this call)
  CFEAR_TRY(problem_scans(ctx, scans, n, "cov_by_sampling", h_ptrs, &capmax));
  int nsrc = 0;
  CFEAR_TRY(cfear_scan_size(ctx, scans[n - 1], &nsrc));
  const int steps = samples_per_axis, m = steps * steps * steps, L = 3 * (n - 1);
  // match scratch per sample: a pair of capacity per (keyframe, source cell); under a non-production tie rule the kd descent's per-thread stacks
  // live there too (registration_dev.h associate_pair_rule: 64 B per pair of capacity for blockDim x 64 entries of 16 B)
  const int cap = std::max((n - 1) * (nsrc > 0 ? nsrc : 1), ctx->tune_nn_tie != 0 ? 4096 : 1);
  std::vector<double> samples, A, costs((size_t)m);  // samples: the design's offsets (in the reference's loop order), then offset + registered pose
  std::vector<int> nres((size_t)m);
  cov_sample_design(xy_range, yaw_range, steps, samples, A);
  for (int k = 0; k < m; k++)
    for (int j = 0; j < 3; j++) samples[3 * k + j] = samples[3 * k + j] + poses_xyt[L + j];
  // device buffers: poses, samples, scan pointers, costs, residual counts, per-sample match arrays
  const size_t bytes = sizeof(double) * (3 * (size_t)n + 3 * (size_t)m + (size_t)m) + sizeof(void*) * (size_t)n + sizeof(int) * (size_t)m +
                       (sizeof(double) * 8 + 3 * sizeof(int)) * (size_t)m * cap + 256;  // (three ints of association scratch per pair: the grouped path, as scratch_layout)
  DevBuf<double> d;
  CFEAR_TRY(d.ensure(ctx, (bytes + 7) / 8, "hipMalloc cost samples"));
  double* d_match = d;
  double* d_poses = d_match + 8 * (size_t)m * cap;
  double* d_samples = d_poses + 3 * n;
  double* d_costs = d_samples + 3 * m;
  ScanDev** d_ptrs = reinterpret_cast<ScanDev**>(d_costs + m);
  int* d_nres = reinterpret_cast<int*>(d_ptrs + n);
  int* d_assoc = d_nres + m;
  CFEAR_HIP_CHECK_AS(ctx, "cov_by_sampling", upload_problem(ctx, d_ptrs, h_ptrs, d_poses, poses_xyt, n));
  CFEAR_HIP_CHECK_AS(ctx, "cov_by_sampling", hipMemcpyAsync(d_samples, samples.data(), sizeof(double) * 3 * m, hipMemcpyHostToDevice, ctx->stream));
  cfear_launch_get_cost_samples(d_ptrs, n, d_poses, d_samples, m, reg_params(ctx), d_match, d_assoc, cap, itr, d_costs, d_nres, ctx->stream);
  CFEAR_HIP_CHECK_AS(ctx, "cov_by_sampling", hipGetLastError());
  CFEAR_HIP_CHECK_AS(ctx, "cov_by_sampling", hipMemcpyAsync(costs.data(), d_costs, sizeof(double) * m, hipMemcpyDeviceToHost, ctx->stream));
  CFEAR_HIP_CHECK_AS(ctx, "cov_by_sampling", hipMemcpyAsync(nres.data(), d_nres, sizeof(int) * m, hipMemcpyDeviceToHost, ctx->stream));
  CFEAR_HIP_CHECK_AS(ctx, "cov_by_sampling", hipStreamSynchronize(ctx->stream));
  double last = 0.0;  // a failed GetCost leaves sample_cost at its previous value (:305: the return value is ignored)
  for (int i = 0; i < m; i++) { if (nres[i] >= 0) last = costs[i]; costs[i] = last; }
  if (sample_costs) memcpy(sample_costs, costs.data(), sizeof(double) * m);
  double c[10];
  lstsq10_svd(m, A.data(), costs.data(), c);
  if (cov_from_quadratic(c, final_cost, num_residuals, covariance_scaler, cov6)) *success = 1;  // :340-373
  return CFEAR_OK;
}

}  // extern "C"
