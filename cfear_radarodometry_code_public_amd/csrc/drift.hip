// drift.hip -- KITTI drift (translation %, rotation deg / 100 m, with the per-length table) of every trajectory of a batch on the
// device: the metric of include/cfear_hip/kitti_metric.hpp (kitti_drift_by_length), which the reference's evaluation worker computes
// once per job (launch/oxford/eval/utils/worker:94-98), for the sequences of one batched odometry object - the rows of a parameter
// grid - straight from the sweep records cfear_odometry_replay_device leaves on the device.
//
// What depends on the ground truth alone is computed once, on the host, into a plan: the segment list (kitti_segments), dgt =
// gt[first]^-1 * gt[last] per segment (pose_inv / pose_mul of kitti_metric.hpp) and 1 / len. What is left per (row, segment) is a few
// dozen flops on two planar poses.
//
// Mapping: lanes run over SEQUENCES. For a fixed segment the 64 lanes of a wave then read 64 neighbouring poses, seq_stride apart
// (80 B in a record buffer: 40 consecutive 128-B lines per wave load, 30 % of the fetched bytes used and every line shared by the x, y
// and theta loads); with lanes over the segments of one row every lane would sit on a line of its own, n_sequences * 80 B apart. The
// segment's table entry is the same for the whole workgroup (its index derives from blockIdx and loop counters only), so it comes in
// through the scalar unit. A start's first pose and its sincos are loaded once for its <= 8 lengths; the segments of a start are its
// lengths 100, 200, ... in turn (a longer length crosses later), so the 16 accumulators (t and r per length) are indexed statically.
//
// Determinism: grid = (tiles of 256 sequences) x (chunks of CHUNK_STARTS starts). A block adds the segments of its starts in table
// order and stores 16 partial sums per sequence; the second kernel adds the chunks in ascending order. No atomics; the chunking depends
// on the plan and n only; a lane never sees another row. So a row's result is a function of (plan, n_sweeps, its poses) alone.
#include "common.h"

#include <math.h>

#include <algorithm>

#pragma GCC visibility push(hidden)
#include "../../include/cfear_hip/kitti_metric.hpp"
#pragma GCC visibility pop

namespace {

using cfear_host::kKittiLengths;
constexpr int NLEN = kKittiLengths;
constexpr int TILE = 256;        // sequences per workgroup
constexpr int CHUNK_STARTS = 8;  // segment starts per workgroup: 8800 poses -> 110 chunks, x 6 tiles at 1536 rows
constexpr int MAX_CHUNKS = 65535;
static_assert(sizeof(cfear_drift) == 184, "cfear_drift is 184 bytes (include/cfear_hip.h)");

struct DriftSeg {  // one (start, length) pair of the plan
  int32_t first, last, length_index, pad;
  double inv_len;
  double dgt[12];  // gt[first]^-1 * gt[last], 3x4 row-major
};
static_assert(sizeof(DriftSeg) == 120, "segment table entry");

struct DriftCounts { int32_t by_length[NLEN]; };  // segments with last < n: a matter of the plan and n, not of a row

__global__ __launch_bounds__(TILE) void drift_partial_kernel(const DriftSeg* __restrict__ segs, const int32_t* __restrict__ start_seg,
                                                             const unsigned char* __restrict__ poses, size_t sweep_stride, size_t seq_stride, int n,
                                                             int n_sequences, int n_starts, double* __restrict__ partial) {
  const int q = blockIdx.x * TILE + threadIdx.x;
  if (q >= n_sequences) return;
  const unsigned char* row = poses + (size_t)q * seq_stride;
  double acc_t[NLEN], acc_r[NLEN];
#pragma unroll
  for (int j = 0; j < NLEN; j++) acc_t[j] = acc_r[j] = 0.0;
  const int s0 = blockIdx.y * CHUNK_STARTS, s1 = min(s0 + CHUNK_STARTS, n_starts);
  for (int s = s0; s < s1; s++) {
    const int b = start_seg[s], cnt = start_seg[s + 1] - b;  // (uniform over the workgroup, as everything read from segs[])
    if (cnt <= 0) continue;
    const double* pf = reinterpret_cast<const double*>(row + (size_t)segs[b].first * sweep_stride);
    const double xf = pf[0], yf = pf[1];
    double sf, cf;
    sincos(pf[2], &sf, &cf);
#pragma unroll
    for (int j = 0; j < NLEN; j++) {
      if (j >= cnt) break;
      const DriftSeg& g = segs[b + j];
      if (g.last >= n) break;  // a shorter replay: the later crossings of this start lie behind its end too
      const double* pl = reinterpret_cast<const double*>(row + (size_t)g.last * sweep_stride);
      const double dx = pl[0] - xf, dy = pl[1] - yf;
      double sl, cl;
      sincos(pl[2], &sl, &cl);
      // des = est[first]^-1 * est[last] of two planar poses: rotation by (cd, sd), translation R_first^T (p_last - p_first)
      const double cd = cf * cl + sf * sl, sd = cf * sl - sf * cl;
      const double tx = cf * dx + sf * dy, ty = cf * dy - sf * dx;
      // e = des^-1 * dgt: trace(e_R) = sum of the diagonal of R_des^T dgt_R; |e_t| = |dgt_t - des_t| (a rotation keeps the norm)
      const double e00 = cd * g.dgt[0] + sd * g.dgt[4], e11 = cd * g.dgt[5] - sd * g.dgt[1];
      // A non-finite component of either pose makes BOTH errors of the segment NaN, as in kitti.drift (the inverse of a des with one NaN
      // is all NaN) - in closed form x, y would never reach the rotation, nor theta[last] the translation. 0 * finite is an exact zero.
      const double poison = 0.0 * ((tx + ty) + (cd + sd));
      double c = 0.5 * (e00 + e11 + g.dgt[10] - 1.0) + poison;
      c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);  // not fmin / fmax: those drop a NaN, the host's clamp keeps it
      const double ux = g.dgt[3] - tx, uy = g.dgt[7] - ty, uz = g.dgt[11];
      acc_r[j] += acos(c) * g.inv_len;
      acc_t[j] += (sqrt(ux * ux + uy * uy + uz * uz) + poison) * g.inv_len;
    }
  }
  double* out = partial + (size_t)blockIdx.y * (2 * NLEN) * n_sequences + q;
#pragma unroll
  for (int j = 0; j < NLEN; j++) {
    out[(size_t)j * n_sequences] = acc_t[j];
    out[(size_t)(NLEN + j) * n_sequences] = acc_r[j];
  }
}

__global__ __launch_bounds__(TILE) void drift_finish_kernel(const double* __restrict__ partial, int n_chunks, int n_sequences, DriftCounts counts,
                                                            cfear_drift* __restrict__ out) {
  const int q = blockIdx.x * TILE + threadIdx.x;
  if (q >= n_sequences) return;
  double acc[2 * NLEN];
#pragma unroll
  for (int k = 0; k < 2 * NLEN; k++) acc[k] = 0.0;
  for (int c = 0; c < n_chunks; c++) {
    const double* p = partial + (size_t)c * (2 * NLEN) * n_sequences + q;
#pragma unroll
    for (int k = 0; k < 2 * NLEN; k++) acc[k] += p[(size_t)k * n_sequences];
  }
  const double deg100 = (180.0 / 3.14159265358979323846) * 100.0;
  cfear_drift d;
  double sum_t = 0.0, sum_r = 0.0;
  int segments = 0;
#pragma unroll
  for (int j = 0; j < NLEN; j++) {
    const int m = counts.by_length[j];
    d.segments_by_length[j] = m;
    d.translation_percent_by_length[j] = m > 0 ? 100.0 * acc[j] / m : 0.0;
    d.rotation_deg_per_100m_by_length[j] = m > 0 ? (acc[NLEN + j] / m) * deg100 : 0.0;
    if (m > 0) { sum_t += acc[j]; sum_r += acc[NLEN + j]; segments += m; }
  }
  d.translation_percent = segments > 0 ? 100.0 * sum_t / segments : 0.0;
  d.rotation_deg_per_100m = segments > 0 ? (sum_r / segments) * deg100 : 0.0;
  d.segments = segments;
  d.reserved = 0;
  out[q] = d;
}

bool all_finite(const double* v, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!std::isfinite(v[i])) return false;
  return true;
}

std::vector<cfear_host::KittiSegment> segments_of(const double* gt34, int n_gt) {
  static_assert(sizeof(cfear_host::Pose34) == 12 * sizeof(double), "a Pose34 is the 12 doubles of a KITTI line");
  return cfear_host::kitti_segments(reinterpret_cast<const cfear_host::Pose34*>(gt34), (size_t)n_gt);
}

}  // namespace

struct cfear_drift_plan {
  int n_gt = 0, n_segments = 0, n_starts = 0;  // n_starts: starts with a segment (a prefix of 0, 10, 20, ...)
  DevBuf<DriftSeg> d_segs;
  DevBuf<int32_t> d_start_seg;                 // [n_starts + 1] first table entry of a start
  std::vector<int32_t> last_of[NLEN];          // per length: `last` of its segments, ascending with the start
};

namespace {

// The one launcher behind both routes: d_poses and d_out on the device, everything queued on the context stream.
int launch_drift(cfear_ctx* ctx, const cfear_drift_plan* plan, const void* d_poses, size_t sweep_stride, size_t seq_stride, int n_sweeps, int n_sequences,
                 cfear_drift* d_out) {
  const int n = std::min(n_sweeps, plan->n_gt);
  DriftCounts counts;
  for (int j = 0; j < NLEN; j++)  // the segments of the truncated problem: those with last < n
    counts.by_length[j] = (int32_t)(std::lower_bound(plan->last_of[j].begin(), plan->last_of[j].end(), (int32_t)n) - plan->last_of[j].begin());
  const int n_starts = counts.by_length[0];  // a start with any segment has the 100 m one
  const int n_chunks = (n_starts + CHUNK_STARTS - 1) / CHUNK_STARTS;
  if (n_chunks > MAX_CHUNKS) return cfear_fail(ctx, CFEAR_ERR_UNSUPPORTED, "drift: more than 5242800 ground-truth poses");
  const int tiles = (n_sequences + TILE - 1) / TILE;
  // (growing frees the old block, which waits for the launches that use it)
  CFEAR_TRY(ctx->d_drift.ensure(ctx, 2 * NLEN * (size_t)n_sequences * (size_t)std::max(n_chunks, 1), "hipMalloc drift scratch"));
  if (n_chunks > 0)
    hipLaunchKernelGGL(drift_partial_kernel, dim3(tiles, n_chunks), dim3(TILE), 0, ctx->stream, plan->d_segs, plan->d_start_seg,
                       static_cast<const unsigned char*>(d_poses), sweep_stride, seq_stride, n, n_sequences, n_starts, ctx->d_drift);
  hipLaunchKernelGGL(drift_finish_kernel, dim3(tiles), dim3(TILE), 0, ctx->stream, ctx->d_drift, n_chunks, n_sequences, counts, d_out);
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  return CFEAR_OK;
}

int check_score_args(cfear_ctx* ctx, const char* route, const cfear_drift_plan* plan, const void* poses, const char* poses_name, size_t sweep_stride,
                     size_t seq_stride, int n_sweeps, int n_sequences, const void* out, const char* out_name) {
  const char* bad = nullptr;
  char what[48];
  if (!plan) bad = "plan is null";
  else if (!poses) { snprintf(what, sizeof(what), "%s is null", poses_name); bad = what; }
  else if (!out) { snprintf(what, sizeof(what), "%s is null", out_name); bad = what; }
  else if (poses_name[0] == 'd' && reinterpret_cast<uintptr_t>(poses) % 8) { /* host poses are copied to an aligned block */ snprintf(what, sizeof(what), "%s is not aligned to 8 bytes", poses_name); bad = what; }
  else if (sweep_stride % 8) bad = "sweep_stride is not a multiple of 8";
  else if (seq_stride % 8) bad = "seq_stride is not a multiple of 8";
  else if (seq_stride < 24) bad = "seq_stride < 24 (a pose is three doubles)";
  else if (n_sequences < 1) bad = "n_sequences < 1";
  else if (n_sweeps < 0) bad = "n_sweeps < 0";
  if (!bad) return CFEAR_OK;
  char msg[128];
  snprintf(msg, sizeof(msg), "%s: %s", route, bad);
  return cfear_fail(ctx, CFEAR_ERR_INVALID, msg);
}

}  // namespace

extern "C" {

int cfear_drift_segments(const double* gt34, int n_gt, int32_t* first, int32_t* last, int32_t* length_index, int capacity, int* n_segments) {
  if (!gt34 || !n_segments || n_gt < 1 || capacity < 0 || (capacity > 0 && (!first || !last || !length_index))) return CFEAR_ERR_INVALID;
  if (!all_finite(gt34, 12 * (size_t)n_gt)) return CFEAR_ERR_INVALID;
  const std::vector<cfear_host::KittiSegment> segs = segments_of(gt34, n_gt);
  *n_segments = (int)segs.size();
  for (int i = 0; i < (int)segs.size() && i < capacity; i++) { first[i] = segs[i].first; last[i] = segs[i].last; length_index[i] = segs[i].length_index; }
  return (int)segs.size() > capacity ? CFEAR_ERR_CAPACITY : CFEAR_OK;
}

int cfear_drift_plan_create(cfear_ctx* ctx, const double* gt34, int n_gt, cfear_drift_plan** plan) {
  if (!ctx) return CFEAR_ERR_INVALID;
  if (!plan) return cfear_fail(ctx, CFEAR_ERR_INVALID, "drift_plan_create: plan is null");
  *plan = nullptr;
  if (!gt34) return cfear_fail(ctx, CFEAR_ERR_INVALID, "drift_plan_create: gt34 is null");
  if (n_gt < 1) return cfear_fail(ctx, CFEAR_ERR_INVALID, "drift_plan_create: n_gt < 1");
  if (!all_finite(gt34, 12 * (size_t)n_gt)) return cfear_fail(ctx, CFEAR_ERR_INVALID, "drift_plan_create: gt34 has a non-finite entry");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const cfear_host::Pose34* gt = reinterpret_cast<const cfear_host::Pose34*>(gt34);
  const std::vector<cfear_host::KittiSegment> segs = segments_of(gt34, n_gt);
  cfear_drift_plan* p = new cfear_drift_plan;
  p->n_gt = n_gt;
  p->n_segments = (int)segs.size();
  std::vector<DriftSeg> table(segs.size());
  std::vector<int32_t> start_seg;
  for (size_t i = 0; i < segs.size(); i++) {
    const cfear_host::KittiSegment& s = segs[i];
    if (i == 0 || s.first != segs[i - 1].first) start_seg.push_back((int32_t)i);
    DriftSeg& g = table[i];
    g.first = s.first; g.last = s.last; g.length_index = s.length_index; g.pad = 0;
    g.inv_len = 1.0 / cfear_host::kitti_length(s.length_index);
    const cfear_host::Pose34 dgt = cfear_host::pose_mul(cfear_host::pose_inv(gt[s.first]), gt[s.last]);
    memcpy(g.dgt, dgt.m, sizeof(g.dgt));
    p->last_of[s.length_index].push_back(s.last);
  }
  p->n_starts = (int)start_seg.size();
  start_seg.push_back((int32_t)segs.size());
  // what the kernel's static indexing rests on: the starts with a segment are 0, 10, 20, ... without a gap, and the segments of a start
  // are its lengths 100, 200, ... in turn (dist never decreases)
  bool regular = true;
  for (int s = 0; s < p->n_starts && regular; s++)
    for (int i = start_seg[s]; i < start_seg[s + 1]; i++) regular = regular && segs[i].first == s * cfear_host::kKittiStep && segs[i].length_index == i - start_seg[s];
  if (!regular) { delete p; return cfear_fail(ctx, CFEAR_ERR_UNSUPPORTED, "drift_plan_create: irregular segment table"); }
  bool ok = p->d_segs.ensure(ctx, std::max<size_t>(table.size(), 1), "") == CFEAR_OK && p->d_start_seg.ensure(ctx, start_seg.size(), "") == CFEAR_OK;
  ok = ok && (table.empty() || hipMemcpy(p->d_segs, table.data(), sizeof(DriftSeg) * table.size(), hipMemcpyHostToDevice) == hipSuccess);
  ok = ok && hipMemcpy(p->d_start_seg, start_seg.data(), sizeof(int32_t) * start_seg.size(), hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) { cfear_drift_plan_release(ctx, p); return cfear_fail(ctx, CFEAR_ERR_NOMEM, "drift_plan_create: device memory"); }
  *plan = p;
  return CFEAR_OK;
}

void cfear_drift_plan_release(cfear_ctx* ctx, cfear_drift_plan* plan) {
  if (!plan) return;
  if (ctx) { (void)hipSetDevice(ctx->device); (void)hipStreamSynchronize(ctx->stream); }  // a queued scoring may still read the table
  delete plan;
}

int cfear_drift_device(cfear_ctx* ctx, const cfear_drift_plan* plan, const void* d_poses, size_t sweep_stride, size_t seq_stride, int n_sweeps,
                       int n_sequences, cfear_drift* d_out) {
  if (!ctx) return CFEAR_ERR_INVALID;
  CFEAR_TRY(check_score_args(ctx, "drift_device", plan, d_poses, "d_poses", sweep_stride, seq_stride, n_sweeps, n_sequences, d_out, "d_out"));
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return launch_drift(ctx, plan, d_poses, sweep_stride, seq_stride, n_sweeps, n_sequences, d_out);
}

int cfear_drift_host(cfear_ctx* ctx, const cfear_drift_plan* plan, const void* h_poses, size_t sweep_stride, size_t seq_stride, int n_sweeps,
                     int n_sequences, cfear_drift* h_out) {
  if (!ctx) return CFEAR_ERR_INVALID;
  CFEAR_TRY(check_score_args(ctx, "drift_host", plan, h_poses, "h_poses", sweep_stride, seq_stride, n_sweeps, n_sequences, h_out, "h_out"));
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  // only the sweeps that are scored travel: the bytes up to the last pose of sweep n - 1
  const int n = std::min(n_sweeps, plan->n_gt);
  const size_t in_bytes = n > 0 ? (size_t)(n - 1) * sweep_stride + (size_t)(n_sequences - 1) * seq_stride + 24 : 0;
  const size_t out_off = (in_bytes + 255) & ~(size_t)255, out_bytes = sizeof(cfear_drift) * (size_t)n_sequences;
  void* blk = nullptr;
  size_t got = 0;
  CFEAR_TRY(cfear_pool_alloc(ctx, out_off + out_bytes, &blk, &got));
  unsigned char* d = static_cast<unsigned char*>(blk);
  hipError_t e = in_bytes ? hipMemcpyAsync(d, h_poses, in_bytes, hipMemcpyHostToDevice, ctx->stream) : hipSuccess;
  int rc = CFEAR_OK;
  if (e == hipSuccess) rc = launch_drift(ctx, plan, d, sweep_stride, seq_stride, n, n_sequences, reinterpret_cast<cfear_drift*>(d + out_off));
  if (e == hipSuccess && rc == CFEAR_OK) e = hipMemcpyAsync(h_out, d + out_off, out_bytes, hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  cfear_pool_free(ctx, blk, got);
  if (rc != CFEAR_OK) return rc;
  if (e != hipSuccess || es != hipSuccess) return cfear_fail(ctx, CFEAR_ERR_HIP, "drift_host", e != hipSuccess ? e : es);
  return CFEAR_OK;
}

}  // extern "C"
