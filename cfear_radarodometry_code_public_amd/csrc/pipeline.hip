// pipeline.hip -- kernels and C-ABI entry points for stages 1.5-3 and the batched odometry step.
// Interface contract + reference citations: include/cfear_hip.h. Device code: features_dev.h,
// registration_dev.h.
//
// One radar sweep of B independent sequences = three launches on the context stream, no host round trip:
//   kstrongest_kernel      (kstrongest.hip)  B*A wavefront-rows, HBM streaming
//   features_step_kernel   one 512-thread workgroup per sequence (79,680 B of LDS, two per compute unit): cloud + motion
//                          compensation, voxel bitmap + counting sort, chunked cell statistics, cell-mean grid
//   register_step_kernel   one 256-thread workgroup per sequence (53 KB LDS incl. the match array, three per compute
//                          unit so that the serial Levenberg-Marquardt controllers of different sequences overlap):
//                          association, robust normal equations, LM, outer loop, keyframe logic
// Per-call entry points (clouds, scans, Register, GetCost, cost-sampling covariance) use the same device code.
// The object itself (struct cfear_odometry) is odometry_obj.h's; its life - creation, reset, destruction, the step entry points, the profile,
// the replay and the plain reads - is odometry_run.hip's, over the launch layer of this file (odo_params, odo_launch_sweep, odo_launch_cfar); its per-sequence configuration - the setters and getters of rows, source
// map, shapes, detectors and fuser options, the device table (seq_table_upload) and odo_seq_sync's re-check - lives in odometry_seq.hip
// over seq_config.h. This file reads the configuration through o->cfg (effective(), sources(), other_cost()) and never writes it.
// The keyframe graph - its kernels, its log (o->kf), its setters and reading routes - is keyframes.hip's: the sweep here launches its two
// stages, and cfear_scan_alloc hands it the blank per-call scans it rebuilds from the log.
#include <math.h>
#include <cmath>
#include <stdlib.h>

#include <algorithm>
#include <new>

#include "odometry_obj.h"
#include "odometry_plan.h"
#include "cov_sampling_dev.h"

namespace {

// ---- per-call kernels -------------------------------------------------------------------------
// one workgroup per cloud: block 0 the filtered cloud, block 1 (if launched) the peaks cloud (radar_driver.cpp:59-60); each also writes its
// cloud's host mirror (cfear_cloud::h_block) when it has one
struct CloudOut { float* xyi; int* d_n; float* h_xyi; int* h_n; int cap; };
__device__ __forceinline__ void cloud_mirror_block(const float* xyi, int n, int cap, float* h_xyi, int* h_n) {
  if (!h_xyi) return;
  __syncthreads();  // the block's own writes of xyi
  const int m = 3 * (n < cap ? n : cap);
  for (int i = threadIdx.x; i < m; i += blockDim.x) h_xyi[i] = xyi[i];
  if (threadIdx.x == 0) *h_n = n;
}
__global__ __launch_bounds__(BLOCK_F) void cloud_kernel(const uint32_t* slots, int A, int k, const double* trig, float rr,
                                                        float md, CloudOut o0, CloudOut o1) {
  __shared__ int red_i[64];
  const int peaks = blockIdx.x;
  const CloudOut o = peaks ? o1 : o0;
  const int n = cloud_build_block(slots, A, k, trig, rr, md, peaks, o.xyi, o.cap, red_i);
  if (threadIdx.x == 0) *o.d_n = n;
  cloud_mirror_block(o.xyi, n, o.cap, o.h_xyi, o.h_n);
}

// Compensate (utils.cpp:96-113) of one cloud or of a sweep's two (the fuser compensates cloud and cloud_peaks by the same motion,
// odometrykeyframefuser.cpp:148-149): one workgroup each
__global__ __launch_bounds__(BLOCK_F) void compensate_kernel(CloudOut o0, CloudOut o1, double m0, double m1, double m2, int ccw) {
  const CloudOut o = blockIdx.x ? o1 : o0;
  const int n = *o.d_n;
  compensate_block(o.xyi, n, m0, m1, m2, ccw);
  cloud_mirror_block(o.xyi, n, o.cap, o.h_xyi, o.h_n);
}

__global__ __launch_bounds__(BLOCK_F) void features_kernel(ScanDev* S, const float* src_xyi, const int* d_n, FeatureParams P,
                                                           BlockScratch B) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[FeatLdsC::total];
  int n = *d_n;
  if (n > S->cap_points) n = S->cap_points;
  int bytes = 1;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const float x = src_xyi[3 * i], y = src_xyi[3 * i + 1], w = src_xyi[3 * i + 2];
    S->xyi[3 * i] = x; S->xyi[3 * i + 1] = y; S->xyi[3 * i + 2] = w;
    bytes &= (w >= 0.f && w <= 255.f && w == (float)(int)w) ? 1 : 0;
  }
  const bool byte_intensities = __syncthreads_and(bytes) != 0;  // (the barrier also makes the copy visible to the whole block)
  PointRegs PR;
  point_regs_from_global(S->xyi, n, PR);
  features_dispatch(S, n, P, B, lds, nullptr, nullptr, false, byte_intensities, PR);
}

// MapPointNormal from given cells (raw = true identity cells, pointnormal.cpp:76-82; the transformed-copy constructor
// :91-110): the cells are already in S->cells; this writes their float means, the registration views and the search grid
__global__ __launch_bounds__(BLOCK_F) void scan_from_cells_kernel(ScanDev* S, int n, FeatureParams P, BlockScratch B) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[FeatLdsC::bm];  // the two reduction arrays
  const FeatureScratch W = make_fscratch(B, lds);
  const size_t cc = (size_t)S->cap_cells;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const cfear_cell c = S->cells[i];
    S->mean_f[2 * i] = (float)c.mean[0]; S->mean_f[2 * i + 1] = (float)c.mean[1];
    double* rs = S->rsrc + i;
    rs[0] = c.mean[0]; rs[cc] = c.mean[1]; rs[2 * cc] = c.normal[0]; rs[3 * cc] = c.normal[1]; rs[4 * cc] = (double)c.nsamples; rs[5 * cc] = c.scale;
    double* rt = S->rtar + 8 * (size_t)i;
    rt[0] = c.mean[0]; rt[1] = c.mean[1]; rt[2] = c.normal[0]; rt[3] = c.normal[1]; rt[4] = (double)c.nsamples; rt[5] = c.scale;
    double* rc = S->rcov + 3 * (size_t)i;
    rc[0] = c.cov[0]; rc[1] = c.cov[1]; rc[2] = c.cov[2];
  }
  if (threadIdx.x == 0) { S->n_points = 0; S->n_samples = 0; S->n_cells = n; S->status = n > 0 ? 0 : CFEAR_ERR_EMPTY; }
  __syncthreads();
  cell_grid_block(S, n, P, W, false, nullptr);
  if (P.nn_tie == 2) kd_build_block(S, B);
}

__global__ void closest_kernel(const ScanDev* S, const double* q, int nq, double d, int* idx, int rule) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq) return;
  if (rule == 0) { idx[i] = scan_closest(grid_view(S), q[2 * i], q[2 * i + 1], d); return; }
  KdVisit stack[CFEAR_KD_STACK];  // (per-thread scratch: this little kernel only)
  idx[i] = scan_closest_rule(S, grid_view(S), q[2 * i], q[2 * i + 1], d, rule, stack);
}

__global__ __launch_bounds__(BLOCK_R, 3) void register_kernel(ScanDev* const* scans, int n, double* poses, double* cov6, RegParams P,
                                                           BlockScratch B, cfear_reg_summary* out, const double* prior_cov6) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[RegLds::total];
  ScanDev** sp = reinterpret_cast<ScanDev**>(lds + RegLds::scanptr);
  for (int i = threadIdx.x; i < n; i += blockDim.x) sp[i] = scans[i];
  __syncthreads();
  const RegScratch W = make_rscratch(B, lds);
  register_block(sp, n, poses, cov6, P, W, reinterpret_cast<double*>(lds + RegLds::par),
                 reinterpret_cast<RegShared*>(lds + RegLds::regsh), out, nullptr, prior_cov6);
}

// ---- RegisterTimeContinuous (registration_dev.h: time-continuous registration) ----------------------------------------
// the prologue, once per call: one thread per source cell writes the compensated source view; thread 0 its header - the source's own
// with rsrc pointing at the view (same cap_cells, so the same strides)
__global__ __launch_bounds__(BLOCK_R) void tc_prologue_kernel(const ScanDev* src, ScanDev* hdr, double* view, int view_cells, double vx, double vy,
                                                              double vth, int ccw) {
  const int j = blockIdx.x * BLOCK_R + threadIdx.x;
  const int cc = src->cap_cells;
  const bool fits = cc <= view_cells;  // (the host sizes the view for the scan's capacity; a view that cannot hold it is a scan without cells)
  if (j == 0) { *hdr = *src; hdr->rsrc = view; if (!fits) { hdr->n_cells = 0; hdr->status = CFEAR_ERR_EMPTY; } }
  if (!fits || j >= src->n_cells || j >= cc) return;
  tc_compensate_cell(src->rsrc, (size_t)cc, view, j, vx, vy, vth, ccw);
}
// register_kernel with the header of the compensated view in the place of the last scan
__global__ __launch_bounds__(BLOCK_R, 3) void register_tc_kernel(ScanDev* const* scans, int n, double* poses, double* cov6, RegParams P,
                                                              BlockScratch B, cfear_reg_summary* out, const double* prior_cov6, ScanDev* src_view) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[RegLds::total];
  ScanDev** sp = reinterpret_cast<ScanDev**>(lds + RegLds::scanptr);
  for (int i = threadIdx.x; i < n; i += blockDim.x) sp[i] = (i == n - 1) ? src_view : scans[i];
  __syncthreads();
  const RegScratch W = make_rscratch(B, lds);
  register_block<-1, true>(sp, n, poses, cov6, P, W, reinterpret_cast<double*>(lds + RegLds::par),
                           reinterpret_cast<RegShared*>(lds + RegLds::regsh), out, nullptr, prior_cov6);
}

__global__ __launch_bounds__(BLOCK_R, 3) void get_cost_kernel(ScanDev* const* scans, int n, const double* poses, RegParams P, BlockScratch B,
                                                           int itr, double* score, double* residuals, int cap, int* n_res) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[RegLds::total];
  ScanDev** sp = reinterpret_cast<ScanDev**>(lds + RegLds::scanptr);
  for (int i = threadIdx.x; i < n; i += blockDim.x) sp[i] = scans[i];
  __syncthreads();
  const RegScratch W = make_rscratch(B, lds);
  get_cost_block(sp, n, poses, P, W, reinterpret_cast<double*>(lds + RegLds::par), reinterpret_cast<RegShared*>(lds + RegLds::regsh), itr,
                 score, residuals, cap, n_res);
}

// GetCost of many candidate poses of the last scan at once (cost-sampling covariance, odometrykeyframefuser.cpp:291-321):
// one workgroup per sample pose; match arrays of workgroup b at match_base + b * 8 * cap (used when they do not fit in LDS)
__global__ __launch_bounds__(BLOCK_R, 3) void get_cost_samples_kernel(ScanDev* const* scans, int n, const double* poses, const double* samples,
                                                                   RegParams P, double* match_base, int* assoc_base, int cap, int itr,
                                                                   double* costs, int* n_res) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[RegLds::total];
  // the sample's poses are written where get_cost_block keeps its parameter vectors: thread i converts pose i in place
  double* my_poses = reinterpret_cast<double*>(lds + RegLds::par);
  const int b = blockIdx.x;
  ScanDev** sp = reinterpret_cast<ScanDev**>(lds + RegLds::scanptr);
  for (int i = threadIdx.x; i < n; i += blockDim.x) sp[i] = scans[i];
  for (int i = threadIdx.x; i < 3 * n; i += blockDim.x) my_poses[i] = (i >= 3 * (n - 1)) ? samples[3 * b + (i - 3 * (n - 1))] : poses[i];
  __syncthreads();
  RegScratch W;
  const size_t c = (size_t)cap;
  double* m = match_base + (size_t)b * 8 * c;
  W.tmx = m; W.tmy = m + c; W.a0 = m + 2 * c; W.a1 = m + 3 * c; W.a2 = m + 4 * c; W.sx = m + 5 * c; W.sy = m + 6 * c; W.w = m + 7 * c;
  W.assoc = assoc_base + (size_t)b * 3 * c; W.cap = cap; W.acap = 3 * cap;
  W.red = reinterpret_cast<double*>(lds + RegLds::red_d);
  W.red_i = reinterpret_cast<int*>(lds + RegLds::red_i);
  get_cost_block(sp, n, my_poses, P, W, reinterpret_cast<double*>(lds + RegLds::par), reinterpret_cast<RegShared*>(lds + RegLds::regsh), itr,
                 costs + b, nullptr, 0, n_res + b);
}

// ---- cost surfaces (surface_dev.h): build stage + evaluation -------------------------------------------
// The A/B build CFEAR_SURFACE_NAIVE evaluates in the build kernel, pixel after pixel, with evaluate_partial (the blocks as the build
// stage leaves them: memory SoA, source means rotated - so the rotation it applies is the identity) and its workgroup reduction.
__device__ inline void surface_naive_eval(RegShared* sh, const SurfHdr* hdr, const double* coords, int nx, int ny, int pixels, double* out) {
  LRegShared* ls = (LRegShared*)sh;
  const int M = hdr->nblk;
  for (int p = 0; p < pixels * pixels; p++) {
    const int i = p / pixels, j = p - i * pixels;
    if (i >= nx || j >= ny) { if (threadIdx.x == 0) out[p] = __builtin_nan(""); continue; }
    const double x = coords[i], y = coords[pixels + j];
    __syncthreads();
    evaluate_partial(ls, M, 0, x, y, 1.0, 0.0);
    __syncthreads();
    if (threadIdx.x == 0) {
      gather_partials(ls->rw.red, &ls->G);
      double v = ls->G.cost;
      if (hdr->prior_on) {
        const double a = hdr->palpha;
        const double d0 = a * (hdr->pguess[0] - x), d1 = a * (hdr->pguess[1] - y), d2 = a * (hdr->pguess[2] - hdr->yaw);
        double r[3];
        for (int k = 0; k < 3; k++) r[k] = hdr->pL[3 * k] * d0 + hdr->pL[3 * k + 1] * d1 + hdr->pL[3 * k + 2] * d2;
        v += 0.5 * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
      }
      out[p] = v;
    }
  }
}
// the build stage of one problem (cfear_get_surface)
template <bool NAIVE>
__global__ __launch_bounds__(BLOCK_R, 3) void surface_build_kernel(ScanDev* const* scans, int n, const double* poses, RegParams P, BlockScratch B,
                                                                int itr, const double* prior_cov6, SurfHdr* hdr, const double* coords,
                                                                const int* nxy, int pixels, double* out) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[RegLds::total];
  ScanDev** sp = reinterpret_cast<ScanDev**>(lds + RegLds::scanptr);
  for (int i = threadIdx.x; i < n; i += blockDim.x) sp[i] = scans[i];
  __syncthreads();
  const RegScratch W = make_rscratch(B, lds);
  RegShared* sh = reinterpret_cast<RegShared*>(lds + RegLds::regsh);
  surface_build_block(sp, n, poses, P, W, reinterpret_cast<double*>(lds + RegLds::par), sh, itr, prior_cov6, hdr);
  if (NAIVE) {
    __syncthreads();
    surface_naive_eval(sh, hdr, coords, nxy[0], nxy[1], pixels, out);
  }
}
// ... of every sequence of a batched odometry object around its last registration (cfear_odometry_surface): what register_step_body
// recorded in OP.cs.ctx; a sequence without a registration in the last step (n < 2) gets no blocks (its coordinates: none visited).
// A sequence whose registration ran soft (cfear_fuser_options::soft_constraint) gets the prior the fuser passes: Identity66
// (FormatScans, odometrykeyframefuser.cpp:486-491) around the recorded pose, as cfear_get_surface with that prior_cov6
template <bool NAIVE>
__global__ __launch_bounds__(BLOCK_R, 3) void surface_build_step_kernel(OdoParams OP, const BlockScratch* scratch, SurfHdr* hdr, const double* coords,
                                                                     const int* nxy, int pixels, double* out) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[RegLds::total];
  const int q = blockIdx.x;
  const CovSampleCtx* cx = OP.cs.ctx + q;
  const int n = cx->n;  // (block-uniform)
  if (n < 2) {
    if (threadIdx.x == 0) { hdr[q].blk = nullptr; hdr[q].cap = 0; hdr[q].nblk = 0; hdr[q].prior_on = 0; hdr[q].yaw = 0; hdr[q].loss = 0; hdr[q].loss_limit = 0; }
    if (NAIVE) for (int p = threadIdx.x; p < pixels * pixels; p += BLOCK_R) out[(size_t)q * pixels * pixels + p] = __builtin_nan("");
    return;
  }
  const int nslots = OP.submap + 1;
  ScanDev** sp = reinterpret_cast<ScanDev**>(lds + RegLds::scanptr);
  for (int i = threadIdx.x; i < n; i += BLOCK_R)
    sp[i] = reinterpret_cast<ScanDev*>(OP.scans_base + OP.scan_stride * ((size_t)q * nslots + cx->slot[i]));
  __shared__ double prior_id[36];
  if (threadIdx.x < 36) prior_id[threadIdx.x] = (threadIdx.x % 7 == 0) ? 1.0 : 0.0;
  __syncthreads();
  const RegScratch W = make_rscratch(scratch[q], lds);
  RegShared* sh = reinterpret_cast<RegShared*>(lds + RegLds::regsh);
  surface_build_block(sp, n, cx->pose, OP.rp, W, reinterpret_cast<double*>(lds + RegLds::par), sh, cx->itr, cx->soft ? prior_id : nullptr, hdr + q,
                      seq_row(OP, q));
  if (NAIVE) {
    __syncthreads();
    surface_naive_eval(sh, hdr + q, coords + (size_t)q * 2 * pixels, nxy[2 * q], nxy[2 * q + 1], pixels, out + (size_t)q * pixels * pixels);
  }
}
// the evaluation (the hot path): grid (tiles of BLOCK * PPT pixels, problems)
template <int COST, int PPT>
__global__ __launch_bounds__(CFEAR_SURFACE_BLOCK) void surface_eval_kernel(const SurfHdr* hdr, const double* coords, const int* nxy, int pixels, double* out) {
  const int q = blockIdx.y;
  surface_eval_tile<COST, PPT>(hdr + q, coords + (size_t)q * 2 * pixels, nxy[2 * q], nxy[2 * q + 1], pixels, out + (size_t)q * pixels * pixels, blockIdx.x);
}

// ---- batched odometry: one launch per stage and sweep (bodies: odometry_step_dev.h) ----
// TIMED: per-phase timestamps (tools/); the production instantiation carries no timer at all
template <bool TIMED>
__global__ __launch_bounds__(BLOCK_F, 4) void features_step_kernel(const uint32_t* slots_all, const double* trig, OdoParams OP,
                                                                   const SeqState* states, ScanDev* const* /*unused: launched as null, kept for the kernarg layout*/,
                                                                   const BlockScratch* scratch) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[FeatLdsC::total];
  features_step_body<TIMED>(lds, OP.seq0 + (int)blockIdx.x, slots_all, trig, OP, states, scratch);
}
// the production registration shape (256 threads, three workgroups per unit) compiled for the 64 scans a sequence can keep: submaps of 8 .. 63
// keyframes when there are more sequences than compute units (launch_register_step). A kernel name of its own: register_step.hip instantiates
// register_step_kernel with 8-scan shared state under the same template arguments, and profilers key on the name.
template <bool TIMED, int KCOST>
__global__ __launch_bounds__(BLOCK_R, CFEAR_REG_MIN_WG) void register_step64_kernel(OdoParams OP, SeqState* states, const BlockScratch* scratch, double* cov_work,
                                                                                   cfear_reg_summary* summaries, double* poses_out) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[RegLds::total];
  register_step_body<TIMED, KCOST>(lds, OP.order ? OP.order[blockIdx.x] : OP.seq0 + (int)blockIdx.x, OP, states, scratch, cov_work, summaries, poses_out);
}
// estimate_cov_by_sampling of the batched step (cov_sampling_dev.h): one workgroup per sequence after the sweep's registration, on its stream
template <bool GENERAL>
__global__ __launch_bounds__(BLOCK_R, 2) void cov_sample_kernel(OdoParams OP, const BlockScratch* scratch, double* cov_work) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[RegLds::total];
  cov_sample_body<GENERAL>(lds, OP.seq0 + (int)blockIdx.x, OP, scratch, cov_work);
}
// the same stage from clouds on the device (filter_type CA-CFAR / cfear_odometry_step_cloud_device)
__global__ __launch_bounds__(BLOCK_F, 4) void features_cloud_step_kernel(const float* xyi_all, int cap, const int* counts, OdoParams OP,
                                                                         const SeqState* states, const BlockScratch* scratch) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[FeatLdsC::total];
  features_cloud_step_body(lds, OP.seq0 + (int)blockIdx.x, xyi_all, cap, counts, OP, states, scratch);
}
// Registration workgroups longest first: sequences ordered by the work their registration took in the previous sweep (a sequence's
// scene changes slowly), as a counting sort over 256 buckets of the key - one workgroup, a few microseconds. The order inside a
// bucket is whatever the atomics give: results do not depend on which workgroup slot a sequence takes.
__global__ __launch_bounds__(1024) void order_kernel(const unsigned* work, int B, int* order) {
  __shared__ unsigned hist[256], red[16];
  const int tid = threadIdx.x;
  unsigned mx = 1u;
  for (int i = tid; i < B; i += 1024) mx = max(mx, work[i]);
  for (int o = 32; o > 0; o >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, o));
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  if (tid < 256) hist[tid] = 0u;
  __syncthreads();
  mx = 1u;
  for (int i = 0; i < 16; i++) mx = max(mx, red[i]);
  const float scale = 255.0f / (float)mx;
  for (int i = tid; i < B; i += 1024) atomicAdd(&hist[255 - min(255, (int)((float)work[i] * scale))], 1u);  // bucket 0 = the most work
  __syncthreads();
  if (tid < 64) {  // exclusive scan of the 256 counts: four per lane, a wave scan across the lanes
    const unsigned c0 = hist[4 * tid], c1 = hist[4 * tid + 1], c2 = hist[4 * tid + 2], c3 = hist[4 * tid + 3];
    unsigned v = c0 + c1 + c2 + c3, incl = v;
    for (int o = 1; o < 64; o <<= 1) { const unsigned u = (unsigned)__shfl_up((int)incl, o); if (tid >= o) incl += u; }
    const unsigned ex = incl - v;
    hist[4 * tid] = ex; hist[4 * tid + 1] = ex + c0; hist[4 * tid + 2] = ex + c0 + c1; hist[4 * tid + 3] = ex + c0 + c1 + c2;
  }
  __syncthreads();
  for (int i = tid; i < B; i += 1024) order[atomicAdd(&hist[255 - min(255, (int)((float)work[i] * scale))], 1u)] = i;
}
// The same order for an object whose sequences run in groups (cfear_odometry_set_sequence_shapes: one registration launch per group,
// seq_groups.h): the counting sort segmented by group. group[i] in 0 .. CFEAR_SEQ_GROUPS - 1 is sequence i's group; the buckets are
// (group, 256 keys scaled by the group's own largest), scanned in that order, so group g's permutation lands in the segment of `order`
// its launch reads - the segments lie in group order and hold exactly the group's sequences (cfear_seq_groups::offset / count), and the
// positions handed out are 0 .. B - 1 whatever `work` holds.
__global__ __launch_bounds__(1024) void order_groups_kernel(const unsigned* work, int B, const int* group, int* order) {
  constexpr int NB = 256 * CFEAR_SEQ_GROUPS;
  static_assert(NB % 64 == 0, "the scan deals the buckets to one wave");
  __shared__ unsigned hist[NB], gmax[CFEAR_SEQ_GROUPS];
  const int tid = threadIdx.x;
  for (int i = tid; i < NB; i += 1024) hist[i] = 0u;
  if (tid < CFEAR_SEQ_GROUPS) gmax[tid] = 1u;
  __syncthreads();
  for (int i = tid; i < B; i += 1024) atomicMax(&gmax[min(max(group[i], 0), CFEAR_SEQ_GROUPS - 1)], work[i]);
  __syncthreads();
  auto bucket = [&](int i) -> int {
    const int g = min(max(group[i], 0), CFEAR_SEQ_GROUPS - 1);
    return 256 * g + 255 - min(255, (int)((float)work[i] * (255.0f / (float)gmax[g])));  // bucket 0 of a group = the most work
  };
  for (int i = tid; i < B; i += 1024) atomicAdd(&hist[bucket(i)], 1u);
  __syncthreads();
  if (tid < 64) {  // exclusive scan of the counts: NB / 64 consecutive buckets per lane, a wave scan across the lanes
    constexpr int PER = NB / 64;
    unsigned v = 0u;
    for (int j = 0; j < PER; j++) v += hist[PER * tid + j];
    unsigned incl = v;
    for (int o = 1; o < 64; o <<= 1) { const unsigned u = (unsigned)__shfl_up((int)incl, o); if (tid >= o) incl += u; }
    unsigned ex = incl - v;
    for (int j = 0; j < PER; j++) { const unsigned c = hist[PER * tid + j]; hist[PER * tid + j] = ex; ex += c; }
  }
  __syncthreads();
  for (int i = tid; i < B; i += 1024) {
    const unsigned at = atomicAdd(&hist[bucket(i)], 1u);
    if (at < (unsigned)B) order[at] = i;  // (always: B sequences were counted)
  }
}
// ---- host-side helpers ---------------------------------------------------------------------------
FeatureParams feature_params(const cfear_ctx* ctx) {
  FeatureParams P;
  P.nn_tie = ctx->tune_nn_tie;
  P.range_res = ctx->par.range_res; P.min_distance = ctx->par.min_distance;
  P.radius = (float)ctx->par.res;
  P.downsample_factor = ctx->par.downsample_factor;
  P.weight_intensity = ctx->par.weight_intensity;
  P.assoc_radius = ctx->par.assoc_radius;
  return P;
}
RegParams reg_params(const cfear_ctx* ctx) {
  RegParams P;
  P.cost = ctx->par.cost; P.loss = ctx->par.loss; P.weight_opt = ctx->par.weight_opt;
  P.recompute_repeats = ctx->tune_repeat_shortcut ? 0 : 1;
  P.nn_tie = ctx->tune_nn_tie;
  P.loss_limit = ctx->par.loss_limit; P.covar_scale = ctx->par.covar_scale; P.regularization = ctx->par.regularization;
  P.assoc_radius = ctx->par.assoc_radius;
  P.max_outer = ctx->par.max_itr_association; P.min_itr = ctx->par.min_itr; P.max_inner = ctx->par.max_solver_iterations;
  return P;
}

constexpr int GRID_CAP = CFEAR_GRID_CAP;

struct ScanLayout { size_t xyi, cells, mean_f, gstart, gpts, rsrc, rtar, rcov, kd_nodes, kd_vind, kd_data, total; };
// cap_cells <= cap_points: cells a scan can hold (every cell is the centroid neighbourhood of an occupied voxel, so never more than
// points; the batched odometry may be sized for fewer: cfear_tune MAX_CELLS). with_cells: the 120-byte cfear_cell records exist (the
// per-call scans, whose cells can be downloaded); the scans of the batched odometry objects go without
ScanLayout scan_layout(int cap_points, int cap_cells, bool with_cells = true, bool with_kd = false) {
  ScanLayout L;
  size_t o = align_up(sizeof(ScanDev), 256);
  L.xyi = o; o = align_up(o + sizeof(float) * 3 * (size_t)cap_points, 256);
  L.cells = o; if (with_cells) o = align_up(o + sizeof(cfear_cell) * (size_t)cap_cells, 256);
  L.mean_f = o; o = align_up(o + sizeof(float) * 2 * (size_t)cap_cells, 256);
  L.gstart = o; o = align_up(o + (sizeof(int) + sizeof(uint2)) * (GRID_CAP + 4), 256);  // 32-bit offsets + the region of the 16-bit ones (grid_off16)
  L.gpts = o; o = align_up(o + sizeof(float4) * (size_t)cap_cells, 256);
  L.rsrc = o; o = align_up(o + sizeof(double) * 6 * (size_t)cap_cells, 256);
  L.rtar = o; o = align_up(o + sizeof(double) * 8 * (size_t)cap_cells, 256);
  L.rcov = o; o = align_up(o + sizeof(double) * 3 * (size_t)cap_cells, 256);
  L.kd_nodes = L.kd_vind = L.kd_data = 0;
  if (with_kd) {  // cfear_tune NN_TIE_RULE = 2 (kdtree_flann_dev.h)
    L.kd_nodes = o; o = align_up(o + sizeof(KdNode) * (2 * (size_t)cap_cells + 2), 256);
    L.kd_vind = o; o = align_up(o + sizeof(int) * (size_t)cap_cells, 256);
    L.kd_data = o; o = align_up(o + sizeof(float) * 2 * (size_t)cap_cells, 256);
  }
  L.total = o;
  return L;
}
// writes a ScanDev header for a flat device block at d_base
ScanDev scan_header(unsigned char* d_base, int cap_points, int cap_cells, bool with_cells = true, bool with_kd = false) {
  const ScanLayout L = scan_layout(cap_points, cap_cells, with_cells, with_kd);
  ScanDev h;
  memset(&h, 0, sizeof(h));
  h.status = CFEAR_ERR_EMPTY;
  h.cap_points = cap_points; h.cap_cells = cap_cells; h.cap_grid = GRID_CAP;
  h.xyi = reinterpret_cast<float*>(d_base + L.xyi);
  h.cells = with_cells ? reinterpret_cast<cfear_cell*>(d_base + L.cells) : nullptr;
  h.rcov = reinterpret_cast<double*>(d_base + L.rcov);
  if (with_kd) {
    h.kd.nodes = reinterpret_cast<KdNode*>(d_base + L.kd_nodes); h.kd.vind = reinterpret_cast<int*>(d_base + L.kd_vind);
    h.kd.data = reinterpret_cast<float*>(d_base + L.kd_data);
  }
  h.kd.root = -1;
  h.mean_f = reinterpret_cast<float*>(d_base + L.mean_f);
  h.gstart = reinterpret_cast<int*>(d_base + L.gstart);
  h.gpts = reinterpret_cast<float4*>(d_base + L.gpts);
  h.rsrc = reinterpret_cast<double*>(d_base + L.rsrc);
  h.rtar = reinterpret_cast<double*>(d_base + L.rtar);
  h.gcell = 1.f;
  return h;
}

struct ScratchLayout { size_t keys, spts, order, vstart, vlist, vcur, rng, part, tmpi, samples, match, assoc, total; int p2cap; bool big; };
ScratchLayout scratch_layout(int cap_points, int pair_cap) {
  ScratchLayout L;
  int p2 = 1; while (p2 < cap_points) p2 <<= 1;
  L.p2cap = p2;
  L.big = true;  // the general feature path (clouds beyond the compact path's limits) works in these global arrays
  const size_t cp = (size_t)cap_points, kp = (size_t)p2;
  size_t o = 0;
  L.keys = o; o = align_up(o + sizeof(uint64_t) * kp, 256);
  L.spts = o; o = align_up(o + sizeof(float) * 3 * cp, 256);
  L.order = o; o = align_up(o + sizeof(int) * cp, 256);
  L.vstart = o; o = align_up(o + sizeof(int) * (cp + 2), 256);
  L.vlist = o; o = align_up(o + sizeof(int) * cp, 256);
  L.vcur = o; o = align_up(o + sizeof(int) * (GRID_CAP + 4), 256);
  L.rng = o; o = align_up(o + sizeof(int) * 8 * (size_t)cap_points, 256);
  L.part = o; o = align_up(o + sizeof(double) * 7 * (size_t)cap_points, 256);
  L.tmpi = o; o = align_up(o + sizeof(int) * (2 * (size_t)cap_points + 16), 256);
  L.samples = o; o = align_up(o + sizeof(float) * 3 * (size_t)cap_points, 256);
  L.match = o; o = align_up(o + sizeof(double) * 8 * (size_t)pair_cap, 256);
  L.assoc = o; o = align_up(o + sizeof(int) * 3 * (size_t)pair_cap, 256);  // registration_dev.h build_problem_block: six ints per (group of four keyframes, source cell) <= 3 per pair
  L.total = o;
  return L;
}
BlockScratch scratch_header(unsigned char* d_base, int cap_points, int pair_cap) {
  const ScratchLayout L = scratch_layout(cap_points, pair_cap);
  BlockScratch B;
  B.keys = reinterpret_cast<uint64_t*>(d_base + L.keys);
  B.spts = reinterpret_cast<float*>(d_base + L.spts);
  B.order = reinterpret_cast<int*>(d_base + L.order);
  B.vstart = reinterpret_cast<int*>(d_base + L.vstart);
  B.vlist = reinterpret_cast<int*>(d_base + L.vlist);
  B.vcur = reinterpret_cast<int*>(d_base + L.vcur);
  B.rng = reinterpret_cast<int*>(d_base + L.rng);
  B.part = reinterpret_cast<double*>(d_base + L.part);
  B.tmpi = reinterpret_cast<int*>(d_base + L.tmpi);
  B.samples = reinterpret_cast<float*>(d_base + L.samples);
  B.match = reinterpret_cast<double*>(d_base + L.match);
  B.assoc = reinterpret_cast<int*>(d_base + L.assoc);
  B.cap_points = cap_points; B.p2cap = L.p2cap; B.pair_cap = pair_cap;
  B.vrank = nullptr; B.vperm = nullptr;
  return B;
}

}  // namespace

struct cfear_scan {
  unsigned char* d_block = nullptr;  // ScanDev header + arrays (a block of the context's pool)
  size_t bytes = 0;
  int n_cells = -1;                  // known on the host since creation (cfear_scan_size without a device round trip)
  int cap_points = 0;
  bool with_kd = false;  // built under cfear_tune NN_TIE_RULE = 2: carries the kd-tree the parity mode's search walks
};
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
// the kernel parameters of one odometry step of `o` under the context's current settings
OdoParams odo_params(const cfear_ctx* ctx, const cfear_odometry* o) {
  OdoParams OP;
  OP.fp = feature_params(ctx); OP.rp = reg_params(ctx);
  OP.A = ctx->A; OP.k = ctx->par.k_strongest; OP.compensate = ctx->par.compensate; OP.ccw = ctx->par.radar_ccw;
  OP.use_keyframe = ctx->par.use_keyframe; OP.submap = ctx->par.submap_scan_size;
  OP.min_keyframe_dist = ctx->par.min_keyframe_dist; OP.min_keyframe_rot_deg = ctx->par.min_keyframe_rot_deg;
  OP.phase_times = o->wg_only ? nullptr : o->d_phase_times; OP.phase_detail = o->phase_detail;
  OP.wg_times = o->wg_only ? o->d_phase_times : nullptr;
  OP.seq0 = 0;
  OP.scans_base = o->d_scans; OP.scan_stride = o->scan_stride;
  OP.records = nullptr;
  OP.flags = o->d_flags;
  OP.order = nullptr; OP.work = o->d_work;
  OP.cs.ctx = nullptr; OP.cs.pinv = nullptr; OP.cs.offs = nullptr; OP.cs.costs = nullptr; OP.cs.cov_out = nullptr; OP.cs.scaler = 0; OP.cs.m = 0;
  if (o->cov_on || o->surf_on) OP.cs.ctx = o->d_cov_ctx;  // (register_step_body records; the sampling stage runs only with cs.m > 0)
  if (o->cov_on) {
    OP.cs.pinv = o->d_cov_design; OP.cs.offs = o->d_cov_design + 10 * (size_t)o->cov_m;
    OP.cs.costs = o->d_cov_costs; OP.cs.scaler = o->cov_scaler; OP.cs.m = o->cov_m;
  }
  OP.seq = o->d_seq; OP.n_sources = odo_sources(o);
  return OP;
}

// the registration step kernel of a sweep. register_step.hip holds the production instantiations (one per cost metric, registrations of
// up to CFEAR_STEP_SMALL_SCANS scans: a bigger LDS match array); a larger submap runs the instantiation of this file (any cost, 64 scans)
// the registration kernel of `count` sequences that are not small (8 .. 63 keyframes), see launch_register_kernel. n_large / max_submap: what
// the choice between the two shapes looks at
static void launch_register_not_small(const OdoParams& P, int count, hipStream_t st, cfear_odometry* o, int n_large, int max_submap) {
  const bool large = o->large_kernel == 2 || (o->large_kernel == 0 && (n_large <= o->n_cus || max_submap >= 24));
  if (large) {
    cfear_launch_register_step_large(P, count, st, o->d_states, o->d_scratch_hdr, o->d_cov_work, o->d_summaries, o->d_poses_out);
    return;
  }
  CFEAR_LAUNCH_REG_BY_COST(register_step64_kernel, P, count, st, o->d_states, o->d_scratch_hdr, o->d_cov_work, o->d_summaries, o->d_poses_out);
}
// ... of an object with per-sequence shapes (cfear_odometry_set_sequence_shapes): one launch per non-empty group (cost, small or not), each on
// the production instantiation of its cost, over the group's segment of the list (seq_groups.h). Whole-batch launches only (an object with
// overlap streams takes no shapes). The sequences that are not small run ONE shape, chosen by today's rule from their number and their
// largest submap; cfear_seq_group() alone decides who is small: register_step_kernel's per-scan LDS arrays hold CFEAR_STEP_SMALL_SCANS scans.
static void launch_register_groups(const OdoParams& P_in, hipStream_t st, cfear_odometry* o) {
  const cfear_seq_groups& G = o->groups;
  const int* list = o->d_group_list;
  if (o->d_order) {  // cfear_tune REGISTRATION_ORDER: longest first inside every group, from the second sweep on
    if (o->order_ready) {
      hipLaunchKernelGGL(order_groups_kernel, dim3(1), dim3(1024), 0, st, o->d_work, o->B, o->d_seq_group, o->d_order);
      list = o->d_order;
    }
    o->order_ready = true;
  }
  for (int g = 0; g < CFEAR_SEQ_GROUPS; g++) {
    if (G.count[g] <= 0) continue;
    OdoParams P = P_in;
    P.rp.cost = cfear_seq_groups::cost_of(g);  // selects the instantiation (the kernel itself takes the cost from the sequence's row)
    P.order = list + G.offset[g];
    if (cfear_seq_groups::small_of(g)) cfear_launch_register_step_small(P, G.count[g], st, o->d_states, o->d_scratch_hdr, o->d_cov_work, o->d_summaries, o->d_poses_out);
    else launch_register_not_small(P, G.count[g], st, o, G.n_large, G.max_large_submap);
  }
}
static void launch_register_kernel(const OdoParams& P_in, int count, hipStream_t st, cfear_odometry* o) {
  const bool shaped = !o->cfg.shapes.empty();
  if (shaped && o->groups.n_launches > 1) { launch_register_groups(P_in, st, o); return; }
  OdoParams P = P_in;
  if (o->d_order && count == o->B && P.seq0 == 0) {  // (whole-batch launches only: the sub-batches of the overlap mode keep their ranges)
    if (o->order_ready) {
      hipLaunchKernelGGL(order_kernel, dim3(1), dim3(1024), 0, st, o->d_work, o->B, o->d_order);
      P.order = o->d_order;
    }
    o->order_ready = true;  // this launch records the keys of the next one
  }
  // shapes that form one group: one launch as without them, on the kernel of the group's cost and size (not of the context's)
  bool small = P.submap + 1 <= CFEAR_STEP_SMALL_SCANS;
  int n_large = count, max_submap = P.submap;
  if (shaped) {
    int g = 0;
    while (g + 1 < CFEAR_SEQ_GROUPS && o->groups.count[g] == 0) g++;
    P.rp.cost = cfear_seq_groups::cost_of(g); small = cfear_seq_groups::small_of(g);
    n_large = o->groups.n_large; max_submap = o->groups.max_large_submap;
  }
  if (small) {
    cfear_launch_register_step_small(P, count, st, o->d_states, o->d_scratch_hdr, o->d_cov_work, o->d_summaries, o->d_poses_out);
    return;
  }
  // a larger submap (8 .. 63 keyframes). Few sequences - at most one per compute unit - or a very large submap (>= 24 keyframes):
  // register_step_large.hip, a unit's threads and LDS for each registration (2 x faster per registration at fifty keyframes); otherwise the
  // production shape compiled for 64 scans, three workgroups per unit (one instantiation per cost metric there too: a ten- or fifty-keyframe
  // submap evaluates thousands of residual blocks 30-80 times per registration). In aggregate both shapes are bound by the same thing, the vector
  // instructions of the evaluation and the association (0.7-0.8 of the issue slots at fifty keyframes), so they differ by
  // < 10 % at 768 sequences and the small shape is the better one at ten keyframes. cfear_tune LARGE_SUBMAP_KERNEL forces either.
  launch_register_not_small(P, count, st, o, n_large, max_submap);
}
// ... and behind it, on the same stream, the cost-sampling stage (estimate_cov_by_sampling) and / or the copy of every sequence's cov_current
// (the replay's per-sweep covariances): before the next sweep's features kernel may reuse a slot the registration read
// src / trig: what the feature stage of this sweep read (the cloud stage of the keyframe log reads the slots again)
static void launch_register_step(const OdoParams& P, int count, hipStream_t st, cfear_odometry* o, const SweepPoints& src, const double* trig) {
  launch_register_kernel(P, count, st, o);
  if (P.cs.m || P.cs.cov_out) {  // (cs.m: sampling on; cs.ctx alone: the surface recording only)
    if (CFEAR_COV_SAMPLING_NAIVE || P.rp.nn_tie != 0)  // (cov_sample_general)
      hipLaunchKernelGGL(cov_sample_kernel<true>, dim3(count), dim3(BLOCK_R), 0, st, P, o->d_scratch_hdr, o->d_cov_work);
    else
      hipLaunchKernelGGL(cov_sample_kernel<false>, dim3(count), dim3(BLOCK_R), 0, st, P, o->d_scratch_hdr, o->d_cov_work);
  }
  // ... and the keyframe recorder (AddToGraph, :234-248 behind the sampling of :202-208: cov_work holds cov_current): the same sequences on the
  // same stream, so the sub-batches of the overlap mode need nothing extra
  // (with a point log the cloud stage goes first: it reads KfLog::tmot before the recorder moves it on, and the recorder commits its verdict)
  if (o->kf.records_clouds()) cfear_launch_keyframe_clouds(o->kf.view(), P, count, st, o->d_states, src.slots, trig);
  if (o->kf.what) cfear_launch_keyframe_record(o->kf.view(), P, count, st, o->d_states, o->d_cov_work);
}
// one sweep of `count` sequences from P.seq0 on (odometry_obj.h): the features stage from the filter's slots or from clouds on the device, then the
// registration stage and what runs behind it
int odo_launch_sweep(cfear_ctx* ctx, cfear_odometry* o, const OdoParams& P, const SweepPoints& src, int count, hipStream_t st, bool timed, hipEvent_t consumed) {
  if (timed) CFEAR_TRY(o->timers.take(ctx, st, o->stage_events));
  if (!src.slots)
    hipLaunchKernelGGL(features_cloud_step_kernel, dim3(count), dim3(BLOCK_F), 0, st, src.xyi, src.cap, src.counts, P, o->d_states, o->d_scratch_hdr);
  else if (P.phase_times)
    hipLaunchKernelGGL(features_step_kernel<true>, dim3(count), dim3(BLOCK_F), 0, st, src.slots, ctx->d_trig, P, o->d_states, nullptr, o->d_scratch_hdr);
  else
    hipLaunchKernelGGL(features_step_kernel<false>, dim3(count), dim3(BLOCK_F), 0, st, src.slots, ctx->d_trig, P, o->d_states, nullptr, o->d_scratch_hdr);
  // the overlap mode's ev_free: the slot buffer may be filtered into again. An object that records keyframe clouds reads the slots once more
  // behind the registration (the cloud stage), so there the event follows that stage: building the clouds in front of the registration into a
  // staging area instead would build them for every sweep, not only for those that fuse, and keep 2 * A * k points per sequence beside the log
  const bool late = consumed && o->kf.records_clouds() && src.slots;
  if (consumed && !late) {
    const hipError_t e = hipEventRecord(consumed, st);
    if (e != hipSuccess) return cfear_fail(ctx, CFEAR_ERR_HIP, "hipEventRecord(o->ev_free[buf][i], so)", e);
  }
  if (timed) CFEAR_TRY(o->timers.take(ctx, st, o->stage_events));
  launch_register_step(P, count, st, o, src, ctx->d_trig);
  if (late) {
    const hipError_t e = hipEventRecord(consumed, st);
    if (e != hipSuccess) return cfear_fail(ctx, CFEAR_ERR_HIP, "hipEventRecord(o->ev_free[buf][i], so)", e);
  }
  if (timed) CFEAR_TRY(o->timers.take(ctx, st, o->stage_events));
  return CFEAR_OK;
}
int odo_shape_check(cfear_ctx* ctx, const cfear_odometry* o, const char* what) {
  bool ok = o->nslots == ctx->par.submap_scan_size + 1 && o->filter == ctx->par.filter_type;
  if ((ctx->tune_nn_tie == 2 && !o->with_kd) || (ctx->tune_nn_tie != 0 && o->pair_cap < 8192 /* cfear_odo_capacities */)) ok = false;  // the tie rule was switched after the object was created
  if (ctx->tune_voxel_order != 0) ok = false;  // per-call scans only (cfear_odometry_create refuses it too)
  if (ok && o->cap_points == cfear_odo_cap_points(o->filter == CFEAR_FILTER_CACFAR, ctx->A, ctx->par.k_strongest, ctx->par.cfar_max_points)) return CFEAR_OK;
  char msg[320];
  snprintf(msg, sizeof(msg), "%s: submap_scan_size / k_strongest / filter_type changed after odometry_create, or a parity mode (cfear_tune NN_TIE_RULE / VOXEL_ORDER) was switched under the object", what);
  return cfear_fail(ctx, CFEAR_ERR_INVALID, msg);
}
// the CA-CFAR stage of n_steps sweeps of every sequence (radar_driver.cpp:52-56) into clouds of o->cap_points points each, [step][sequence]: the
// context's detector over one image per sequence, or the sequences' own over the sources they share
int odo_launch_cfar(cfear_ctx* ctx, cfear_odometry* o, const uint8_t* d_polar, int n_steps, float* d_xyi, int* d_counts, int* d_rows, hipStream_t st) {
  if (o->det_grid) return cfear_launch_cfar_grid(ctx, o->det_grid.get(), d_polar, n_steps, ctx->par.cfar_max_distance, d_xyi, o->cap_points, d_counts, d_rows, st);
  return cfear_launch_cfar_batch(ctx, d_polar, n_steps * o->B, ctx->par.cfar_window_size, ctx->par.cfar_nb_guard_cells, ctx->par.cfar_false_alarm_rate,
                                 ctx->par.cfar_max_distance, d_xyi, o->cap_points, d_counts, d_rows, st);
}
// after a synchronisation of the context stream: has any scan of this object overflowed its cell capacity (CFEAR_TUNE_MAX_CELLS)?
int odo_capacity_check(cfear_ctx* ctx, cfear_odometry* o, const char* what) {
  if (!o->d_flags) return CFEAR_OK;  // sized for every filtered point: cannot happen
  int f = 0;
  CFEAR_HIP_CHECK(ctx, hipMemcpy(&f, o->d_flags, sizeof(int), hipMemcpyDeviceToHost));
  if (f & 2) {
    char msg[320];
    snprintf(msg, sizeof(msg), "%s: a sweep's cloud had more points than the %d this object is sized for (cfear_params.cfar_max_points with filter_type CA-CFAR; the "
             "capacity argument of cfear_odometry_step_cloud_device): the first %d in (azimuth, range) order were kept, the results of that sequence are those "
             "of a truncated cloud", what, o->cap_points, o->cap_points);
    return cfear_fail(ctx, CFEAR_ERR_CAPACITY, msg);
  }
  if (f & 1) {
    char msg[400];
    snprintf(msg, sizeof(msg), "%s: a scan produced more than %d oriented surface points (%s): its first %d were kept, the results of that sequence are those of a "
             "truncated scan", what, o->cap_cells, ctx->tune_max_cells > 0 ? "cfear_tune CFEAR_TUNE_MAX_CELLS of this object" :
             "the default of objects with more than 7 keyframes: min(points per scan, 4096); raise it with cfear_tune CFEAR_TUNE_MAX_CELLS before cfear_odometry_create", o->cap_cells);
    return cfear_fail(ctx, CFEAR_ERR_CAPACITY, msg);
  }
  return CFEAR_OK;
}
// the scan and scratch layouts of an object (odometry_obj.h): the bytes of one scan slot and of one sequence's scratch block ...
void odo_block_bytes(const cfear_odometry* o, size_t* scan_bytes, size_t* scratch_bytes) {
  *scan_bytes = scan_layout(o->cap_points, o->cap_cells, false, o->with_kd).total;
  *scratch_bytes = scratch_layout(o->cap_points, o->pair_cap).total;
}
// ... and their headers into d_scans (o->scan_stride apart) and d_scratch_hdr
int odo_upload_headers(cfear_ctx* ctx, cfear_odometry* o, size_t scratch_bytes) {
  const int B = o->B;
  std::vector<BlockScratch> hdrs((size_t)B);
  std::vector<ScanDev> scan_hdrs((size_t)B * o->nslots);  // all headers built on the host, uploaded with one strided copy
  for (int q = 0; q < B; q++) {
    for (int j = 0; j < o->nslots; j++)
      scan_hdrs[(size_t)q * o->nslots + j] = scan_header(o->d_scans + o->scan_stride * ((size_t)q * o->nslots + j), o->cap_points, o->cap_cells, false, o->with_kd);
    hdrs[q] = scratch_header(o->d_scratch + scratch_bytes * (size_t)q, o->cap_points, o->pair_cap);
  }
  bool ok = hipMemcpy2D(o->d_scans, o->scan_stride, scan_hdrs.data(), sizeof(ScanDev), sizeof(ScanDev), scan_hdrs.size(), hipMemcpyHostToDevice) == hipSuccess;
  ok = ok && hipMemcpy(o->d_scratch_hdr, hdrs.data(), sizeof(BlockScratch) * hdrs.size(), hipMemcpyHostToDevice) == hipSuccess;
  return ok ? CFEAR_OK : cfear_fail(ctx, CFEAR_ERR_HIP, "odometry state upload");
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
static CloudOut cloud_out(cfear_cloud* c) {
  CloudOut o; o.xyi = c->d_xyi; o.d_n = c->d_n; o.cap = c->cap;
  o.h_xyi = c->h_block ? c->h_xyi() : nullptr; o.h_n = c->h_block ? c->h_n() : nullptr;
  return o;
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
  hipLaunchKernelGGL(cloud_kernel, dim3(c1 ? 2 : 1), dim3(BLOCK_F), 0, ctx->stream, ctx->d_slots, A, k, ctx->d_trig,
                     ctx->par.range_res, ctx->par.min_distance, cloud_out(c0), cloud_out(c1 ? c1 : c0));
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
  hipLaunchKernelGGL(compensate_kernel, dim3(1), dim3(BLOCK_F), 0, ctx->stream, cloud_out(c), cloud_out(c), motion_xyt[0], motion_xyt[1], th, ccw);
  c->mirror_valid = c->h_block != nullptr;
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  return CFEAR_OK;
}

int cfear_compensate_pair(cfear_ctx* ctx, cfear_cloud* c0, cfear_cloud* c1, const double motion_xyt[3], int ccw) {
  if (!ctx || !c0 || !c1 || c0 == c1 || !motion_xyt) return cfear_fail(ctx, CFEAR_ERR_INVALID, "compensate_pair: bad argument");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const double th = atan2(sin(motion_xyt[2]), cos(motion_xyt[2]));
  hipLaunchKernelGGL(compensate_kernel, dim3(2), dim3(BLOCK_F), 0, ctx->stream, cloud_out(c0), cloud_out(c1), motion_xyt[0], motion_xyt[1], th, ccw);
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
    const FeatureParams P = feature_params(ctx);
    hipLaunchKernelGGL(features_kernel, dim3(1), dim3(BLOCK_F), 0, ctx->stream, d_scan, cloud->d_xyi, cloud->d_n, P, B);
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
    hipLaunchKernelGGL(scan_from_cells_kernel, dim3(1), dim3(BLOCK_F), 0, ctx->stream, d_scan, n, feature_params(ctx), B);
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
    hipLaunchKernelGGL(closest_kernel, dim3((nq + 255) / 256), dim3(256), 0, ctx->stream, reinterpret_cast<const ScanDev*>(s->d_block), dq, nq, d, di, ctx->tune_nn_tie);
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
  if (vel) {
    // (the cells of a scan are known on the host since its creation; a scan that does not know them yet is covered by its capacity)
    const int cells = scans[n - 1]->n_cells >= 0 ? scans[n - 1]->n_cells : scans[n - 1]->cap_points;
    hipLaunchKernelGGL(tc_prologue_kernel, dim3(std::max(1, (cells + BLOCK_R - 1) / BLOCK_R)), dim3(BLOCK_R), 0, ctx->stream, pb.ptrs[n - 1], pb.tc.hdr,
                       pb.tc.view, pb.tc.view_cells, vel[0], vel[1], vel[2], ccw ? 1 : 0);
    CFEAR_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(register_tc_kernel, dim3(1), dim3(BLOCK_R), 0, ctx->stream, pb.d->ptrs, n, pb.d->poses, pb.d->cov, reg_params(ctx), pb.B, &pb.d->sum,
                       d_prior, pb.tc.hdr);
  } else {
    hipLaunchKernelGGL(register_kernel, dim3(1), dim3(BLOCK_R), 0, ctx->stream, pb.d->ptrs, n, pb.d->poses, pb.d->cov, reg_params(ctx), pb.B, &pb.d->sum, d_prior);
  }
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
  double* d_poses = pb.d->poses;
  double* d_score = pb.d->cov;
  int* d_nres = reinterpret_cast<int*>(d_score + 1);
  ScanDev** d_ptrs = pb.d->ptrs;
  DevBuf<double> d_res;
  CFEAR_TRY(d_res.ensure(ctx, (size_t)capacity, "hipMalloc residuals"));
  hipError_t e = hipMemcpyAsync(d_ptrs, pb.ptrs, sizeof(void*) * n, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_poses, poses_xyt, sizeof(double) * 3 * n, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(get_cost_kernel, dim3(1), dim3(BLOCK_R), 0, ctx->stream, d_ptrs, n, d_poses, reg_params(ctx), pb.B, itr, d_score, d_res,
                       capacity, d_nres);
    e = hipGetLastError();
  }
  int nres = -1;
  if (e == hipSuccess) e = hipMemcpyAsync(score, d_score, sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(&nres, d_nres, sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess && nres > 0 && capacity > 0)
    e = hipMemcpy(residuals, d_res, sizeof(double) * (size_t)(nres < capacity ? nres : capacity), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return cfear_fail(ctx, CFEAR_ERR_HIP, "get_cost", e);
  *n_residuals = nres;
  if (nres < 0) return cfear_fail(ctx, CFEAR_ERR_EMPTY, "get_cost: too few residuals");  // GetCost returns false (:205-208)
  return CFEAR_OK;
}

// ---- cost surfaces (n_scan_normal.cpp:29-65; surface_dev.h) ---------------------------------------------
__attribute__((visibility("hidden"))) int cfear_surface_axis(double v0, double res, int width, int pixels, double* out);  // cabi.hip
namespace {
// the evaluation of `problems` surfaces (surface_eval_kernel): two pixels per thread, or one where that leaves fewer than two
// workgroups per compute unit (a single surface)
static void launch_surface_eval(const RegParams& P, int problems, const SurfHdr* d_hdr, const double* d_coords, const int* d_nxy, int pixels,
                         double* d_out, hipStream_t st) {
  const int np = pixels * pixels;
  const int t2 = (np + 2 * CFEAR_SURFACE_BLOCK - 1) / (2 * CFEAR_SURFACE_BLOCK);
  const bool two = (long long)t2 * problems >= 512;
  const dim3 grid(two ? t2 : (np + CFEAR_SURFACE_BLOCK - 1) / CFEAR_SURFACE_BLOCK, problems);
#define CFEAR_SURF_EVAL(C, K) hipLaunchKernelGGL((surface_eval_kernel<C, K>), grid, dim3(CFEAR_SURFACE_BLOCK), 0, st, d_hdr, d_coords, d_nxy, \
                                                 pixels, d_out)
  if (P.cost == CFEAR_COST_P2L) { if (two) CFEAR_SURF_EVAL(CFEAR_COST_P2L, 2); else CFEAR_SURF_EVAL(CFEAR_COST_P2L, 1); }
  else if (P.cost == CFEAR_COST_P2D) { if (two) CFEAR_SURF_EVAL(CFEAR_COST_P2D, 2); else CFEAR_SURF_EVAL(CFEAR_COST_P2D, 1); }
  else { if (two) CFEAR_SURF_EVAL(CFEAR_COST_P2P, 2); else CFEAR_SURF_EVAL(CFEAR_COST_P2P, 1); }
#undef CFEAR_SURF_EVAL
}
}  // namespace

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
  double* d_poses = pb.d->poses;
  double* d_prior = pb.d->cov;
  ScanDev** d_ptrs = pb.d->ptrs;
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
  hipError_t e = hipMemcpyAsync(d_ptrs, pb.ptrs, sizeof(void*) * n, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_poses, poses_xyt, sizeof(double) * 3 * n, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess && prior_cov6) e = hipMemcpyAsync(d_prior, prior_cov6, sizeof(double) * 36, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_coords, coords.data(), sizeof(double) * 2 * pixels, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_nxy, nxy, sizeof(nxy), hipMemcpyHostToDevice, ctx->stream);
  const RegParams P = reg_params(ctx);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(surface_build_kernel<CFEAR_SURFACE_NAIVE != 0>, dim3(1), dim3(BLOCK_R), 0, ctx->stream, d_ptrs, n, d_poses, P, pb.B, itr,
                       prior_cov6 ? d_prior : nullptr, d_hdr, d_coords, d_nxy, pixels, d_out);
    e = hipGetLastError();
  }
  if (e == hipSuccess && !CFEAR_SURFACE_NAIVE) {
    launch_surface_eval(P, 1, d_hdr, d_coords, d_nxy, pixels, d_out, ctx->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(surface, d_out, sizeof(double) * np, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return cfear_fail(ctx, CFEAR_ERR_HIP, "get_surface", e);
  if (nx) *nx = nxy[0];
  if (ny) *ny = nxy[1];
  return CFEAR_OK;
}

// ---- cost-sampling covariance (odometrykeyframefuser.cpp:261-380) ------------------------------------
namespace {
// Minimum-norm least squares of A c = b (A: m x 10), what Eigen's bdcSvd().solve() returns (odometrykeyframefuser.cpp:337), by a
// one-sided Jacobi (Hestenes) singular value decomposition: plane rotations from the right make the columns of W = A V
// mutually orthogonal; then the singular values are the column norms, U = W / sigma, and c = V diag(1 / sigma) U^T b over the
// singular values above the rank threshold (Eigen's SVDBase::threshold(): diagSize = min(m, n) times epsilon, times sigma_max; numpy's lstsq
// default is max(m, n) - with 27-125 samples 3-12 x higher, which would cut a weakly observed yaw direction Eigen keeps). Works on A itself - no normal
// equations - so nothing is lost to squaring the condition number (the yaw column is ~1e-5 of the others).
static void jacobi10(int m, const double* A, std::vector<double>& W, double V[100], double sig[10], double* thr_out) {
  const int n = 10;
  W.assign((size_t)m * n, 0.0);
  for (int i = 0; i < m * n; i++) W[i] = A[i];
  for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) V[i * n + j] = (i == j) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 60; sweep++) {
    bool rotated = false;
    for (int p = 0; p < n - 1; p++)
      for (int q = p + 1; q < n; q++) {
        double al = 0, be = 0, ga = 0;
        for (int i = 0; i < m; i++) { const double x = W[(size_t)i * n + p], y = W[(size_t)i * n + q]; al += x * x; be += y * y; ga += x * y; }
        if (ga == 0.0 || fabs(ga) <= 1e-15 * sqrt(al * be)) continue;
        rotated = true;
        const double zeta = (be - al) / (2.0 * ga);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
        for (int i = 0; i < m; i++) {
          const double x = W[(size_t)i * n + p], y = W[(size_t)i * n + q];
          W[(size_t)i * n + p] = cs * x - sn * y; W[(size_t)i * n + q] = sn * x + cs * y;
        }
        for (int i = 0; i < n; i++) {
          const double x = V[i * n + p], y = V[i * n + q];
          V[i * n + p] = cs * x - sn * y; V[i * n + q] = sn * x + cs * y;
        }
      }
    if (!rotated) break;
  }
  double smax = 0;
  for (int j = 0; j < n; j++) {
    double q = 0;
    for (int i = 0; i < m; i++) q += W[(size_t)i * n + j] * W[(size_t)i * n + j];
    sig[j] = sqrt(q);
    if (sig[j] > smax) smax = sig[j];
  }
  *thr_out = (double)(m < n ? m : n) * 2.220446049250313e-16 * smax;
}
static void lstsq10_svd(int m, const double* A, const double* b, double c[10]) {
  const int n = 10;
  std::vector<double> W;
  double V[100], sig[10], thr;
  jacobi10(m, A, W, V, sig, &thr);
  for (int k = 0; k < n; k++) c[k] = 0.0;
  for (int j = 0; j < n; j++) {
    if (!(sig[j] > thr)) continue;
    double q = 0;
    for (int i = 0; i < m; i++) q += W[(size_t)i * n + j] * b[i];  // sigma_j * (u_j . b)
    q /= sig[j] * sig[j];
    for (int k = 0; k < n; k++) c[k] += V[k * n + j] * q;
  }
}
// The same decomposition as the minimum-norm pseudo-inverse P (10 x m, row-major): c = P b for every b (the batched routes' sample design
// is fixed by (xy_range, yaw_range, samples_per_axis), so the device fit is a 10 x m product). Same rank threshold as lstsq10_svd.
static void pinv10_svd(int m, const double* A, double* P) {
  const int n = 10;
  std::vector<double> W;
  double V[100], sig[10], thr;
  jacobi10(m, A, W, V, sig, &thr);
  for (size_t i = 0; i < (size_t)n * m; i++) P[i] = 0.0;
  for (int j = 0; j < n; j++) {
    if (!(sig[j] > thr)) continue;
    const double s2 = sig[j] * sig[j];
    for (int k = 0; k < n; k++) {
      const double v = V[k * n + j];
      for (int i = 0; i < m; i++) P[(size_t)k * m + i] += v * (W[(size_t)i * n + j] / s2);
    }
  }
}
static void linspace(double start, double end, int num, std::vector<double>& v) {  // odometrykeyframefuser.cpp:497-524
  v.clear();
  if (num <= 0) return;
  if (num == 1) { v.push_back(start); return; }
  const double delta = (end - start) / ((double)num - 1);
  for (int i = 0; i < num - 1; i++) v.push_back(start + delta * i);
  v.push_back(end);
}
// the reference's sample design (odometrykeyframefuser.cpp:277-336): offsets [m][3] (x, y, yaw) in its loop order (:294-296) and the
// rows [m][10] of the least-squares quadratic
static void cov_sample_design(double xy_range, double yaw_range, int steps, std::vector<double>& offs, std::vector<double>& A) {
  std::vector<double> xs, ths;  // :277-290
  linspace(-xy_range * 0.5, xy_range * 0.5, steps, xs);
  linspace(-yaw_range * 0.5, yaw_range * 0.5, steps, ths);
  const size_t m = (size_t)steps * steps * steps;
  offs.assign(3 * m, 0.0); A.assign(10 * m, 0.0);
  int k = 0;
  for (int it = 0; it < steps; it++)  // the reference's loop order (:294-296)
    for (int ix = 0; ix < steps; ix++)
      for (int iy = 0; iy < steps; iy++, k++) {
        const double x = xs[ix], y = xs[iy], z = ths[it];
        offs[3 * k] = x; offs[3 * k + 1] = y; offs[3 * k + 2] = z;
        double* r = &A[10 * (size_t)k];
        r[0] = x * x; r[1] = y * y; r[2] = z * z; r[3] = x * y; r[4] = y * z; r[5] = z * x; r[6] = x; r[7] = y; r[8] = z; r[9] = 1.0;  // :325-336
      }
}
}  // namespace

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
  hipError_t e = hipMemcpyAsync(d_ptrs, h_ptrs, sizeof(void*) * n, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_poses, poses_xyt, sizeof(double) * 3 * n, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_samples, samples.data(), sizeof(double) * 3 * m, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(get_cost_samples_kernel, dim3(m), dim3(BLOCK_R), 0, ctx->stream, d_ptrs, n, d_poses, d_samples, reg_params(ctx), d_match,
                       d_assoc, cap, itr, d_costs, d_nres);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(costs.data(), d_costs, sizeof(double) * m, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(nres.data(), d_nres, sizeof(int) * m, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return cfear_fail(ctx, CFEAR_ERR_HIP, "cov_by_sampling", e);
  double last = 0.0;  // a failed GetCost leaves sample_cost at its previous value (:305: the return value is ignored)
  for (int i = 0; i < m; i++) { if (nres[i] >= 0) last = costs[i]; costs[i] = last; }
  if (sample_costs) memcpy(sample_costs, costs.data(), sizeof(double) * m);
  double c[10];
  lstsq10_svd(m, A.data(), costs.data(), c);
  if (cov_from_quadratic(c, final_cost, num_residuals, covariance_scaler, cov6)) *success = 1;  // :340-373
  return CFEAR_OK;
}

// ---- batched odometry: the object's life is odometry_run.hip's; here the routes that run kernels of this file --------------------
// the [B] records of the registrations (cost sampling and surface recording share them), all 'nothing recorded'. The streams are idle.
static int odo_ensure_cov_ctx(cfear_ctx* ctx, cfear_odometry* o, const char* what) {
  return o->d_cov_ctx.ensure(ctx, (size_t)o->B, what, true);
}

// ---- estimate_cov_by_sampling on the batched routes (cov_sampling_dev.h) ------------------------------------------------
int cfear_odometry_set_cov_sampling(cfear_ctx* ctx, cfear_odometry* o, int enable, double xy_range, double yaw_range, int samples_per_axis,
                                    double covariance_scaler) {
  if (!ctx || !o) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_set_cov_sampling: bad argument");
  if (!enable) {  // the buffers stay for a later switch back on; kernels already queued keep the parameters they were given
    o->cov_on = false;
    return CFEAR_OK;
  }
  if (samples_per_axis < 1 || !std::isfinite(xy_range) || !std::isfinite(yaw_range) || !std::isfinite(covariance_scaler))
    return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_set_cov_sampling: samples_per_axis < 1 or a range / scaler that is not finite");
  if (samples_per_axis > 8) return cfear_fail(ctx, CFEAR_ERR_UNSUPPORTED, "odometry_set_cov_sampling: at most 8 samples per axis (512 GetCost per sweep)");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  CFEAR_TRY(odo_join(ctx, o));
  CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // nothing in flight reads the design or the costs while they are replaced
  const int m = samples_per_axis * samples_per_axis * samples_per_axis;
  std::vector<double> offs, A, design((size_t)13 * m);
  cov_sample_design(xy_range, yaw_range, samples_per_axis, offs, A);
  pinv10_svd(m, A.data(), design.data());
  memcpy(design.data() + 10 * (size_t)m, offs.data(), sizeof(double) * 3 * m);
  CFEAR_TRY(odo_ensure_cov_ctx(ctx, o, "hipMalloc cost-sampling buffers"));
  CFEAR_TRY(o->d_cov_design.ensure(ctx, 13 * (size_t)m, "hipMalloc cost-sampling buffers"));
  CFEAR_TRY(o->d_cov_costs.ensure(ctx, (size_t)m * o->B, "hipMalloc cost-sampling buffers"));
  CFEAR_HIP_CHECK(ctx, hipMemset(o->d_cov_costs, 0, sizeof(double) * (size_t)m * o->B));
  CFEAR_HIP_CHECK(ctx, hipMemcpy(o->d_cov_design, design.data(), sizeof(double) * 13 * (size_t)m, hipMemcpyHostToDevice));
  // no sweep sampled yet under these settings (n = 0: cov_samples reads zeros and 'not sampled')
  CFEAR_HIP_CHECK(ctx, hipMemset(o->d_cov_ctx, 0, sizeof(CovSampleCtx) * (size_t)o->B));
  o->cov_m = m; o->cov_scaler = covariance_scaler; o->cov_on = true;
  return CFEAR_OK;
}

// ---- cost surfaces on the batched step (surface_dev.h) ---------------------------------------------------------------
int cfear_odometry_set_surface_recording(cfear_ctx* ctx, cfear_odometry* o, int enable) {
  if (!ctx || !o) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_set_surface_recording: bad argument");
  if (!enable) { o->surf_on = false; return CFEAR_OK; }
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (!o->d_cov_ctx) {
    CFEAR_TRY(odo_join(ctx, o));
    CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    CFEAR_TRY(odo_ensure_cov_ctx(ctx, o, "hipMalloc surface records"));
  }
  o->surf_on = true;
  return CFEAR_OK;
}

int cfear_odometry_surface(cfear_ctx* ctx, cfear_odometry* o, double res, int width, double* d_surface, int* n_used, int* itr_used,
                           double* poses_used) {
  if (!ctx || !o || !d_surface) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_surface: bad argument");
  if (!o->surf_on && !o->cov_on)
    return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_surface: nothing is recorded (cfear_odometry_set_surface_recording)");
  int pixels = 0, vx = 0, vy = 0;
  {
    const int rc = cfear_surface_dims(res, width, 0.0, 0.0, &pixels, &vx, &vy);
    if (rc == CFEAR_ERR_INVALID) return cfear_fail(ctx, rc, "odometry_surface: res must be finite and > 0, width >= 0");
    if (rc != CFEAR_OK) return cfear_fail(ctx, rc, "odometry_surface: more than CFEAR_SURFACE_MAX_SIDE pixels per side");
  }
  if (const int q = o->cfg.other_cost()) {
    char msg[320];
    snprintf(msg, sizeof(msg), "odometry_surface: the sequences' shapes differ in cost (sequence 0: %d, sequence %d: %d; cfear_odometry_set_sequence_shapes) - the "
             "evaluation is one launch per cost metric over all problems; surfaces run under shapes of one cost (any submap_scan_size)",
             (int)o->cfg.shapes[0].cost, q, (int)o->cfg.shapes[(size_t)q].cost);
    return cfear_fail(ctx, CFEAR_ERR_UNSUPPORTED, msg);
  }
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  CFEAR_TRY(odo_seq_sync(ctx, o, "odometry_surface"));
  CFEAR_TRY(odo_join(ctx, o));
  const int B = o->B;
  // what the last step's registrations used: the grid of each is centred on its recorded pose (computed here, on the host)
  std::vector<CovSampleCtx> rec;
  if (o->surf_ready) {
    rec.resize((size_t)B);
    CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(rec.data(), o->d_cov_ctx, sizeof(CovSampleCtx) * (size_t)B, hipMemcpyDeviceToHost, ctx->stream));
  }
  CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  const int cap_rc = odo_capacity_check(ctx, o, "odometry_surface");  // (the stream is idle: the surfaces are computed all the same)
  CFEAR_TRY(o->d_surf_hdr.ensure(ctx, (size_t)B, "hipMalloc surface buffers"));
  CFEAR_TRY(o->d_surf_coords.ensure(ctx, 2 * (size_t)pixels * B, "hipMalloc surface buffers"));
  CFEAR_TRY(o->d_surf_nxy.ensure(ctx, 2 * (size_t)B, "hipMalloc surface buffers"));
  std::vector<double> coords(2 * (size_t)pixels * B, 0.0);
  std::vector<int> nxy(2 * (size_t)B, 0);
  for (int q = 0; q < B; q++) {
    const int n = o->surf_ready ? rec[q].n : 0;
    if (n >= 2) {
      const double* last = rec[q].pose + 3 * (n - 1);
      nxy[2 * q] = cfear_surface_axis(last[0], res, width, pixels, coords.data() + (size_t)q * 2 * pixels);
      nxy[2 * q + 1] = cfear_surface_axis(last[1], res, width, pixels, coords.data() + (size_t)q * 2 * pixels + pixels);
    }
    if (n_used) n_used[q] = n >= 2 ? n : 0;
    if (itr_used) itr_used[q] = n >= 2 ? rec[q].itr : 0;
    if (poses_used) {
      double* d = poses_used + (size_t)q * 3 * MAX_SCANS;
      for (int i = 0; i < 3 * MAX_SCANS; i++) d[i] = (n >= 2 && i < 3 * n) ? rec[q].pose[i] : 0.0;
    }
  }
  CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(o->d_surf_coords, coords.data(), sizeof(double) * coords.size(), hipMemcpyHostToDevice, ctx->stream));
  CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(o->d_surf_nxy, nxy.data(), sizeof(int) * nxy.size(), hipMemcpyHostToDevice, ctx->stream));
  OdoParams OP = odo_params(ctx, o);
  OP.cs.ctx = o->d_cov_ctx;
  if (o->surf_ready) {
    hipLaunchKernelGGL(surface_build_step_kernel<CFEAR_SURFACE_NAIVE != 0>, dim3(B), dim3(BLOCK_R), 0, ctx->stream, OP, o->d_scratch_hdr, o->d_surf_hdr,
                       o->d_surf_coords, o->d_surf_nxy, pixels, d_surface);
    CFEAR_HIP_CHECK(ctx, hipGetLastError());
  } else {  // no step since the last reset / replay: no blocks, no visited cells (all NaN)
    CFEAR_HIP_CHECK(ctx, hipMemsetAsync(o->d_surf_hdr, 0, sizeof(SurfHdr) * (size_t)B, ctx->stream));
  }
  if (!CFEAR_SURFACE_NAIVE || !o->surf_ready) {
    RegParams eval_rp = OP.rp;
    eval_rp.cost = o->cfg.effective(0, ctx->par).par.cost;  // (one cost: checked above)
    launch_surface_eval(eval_rp, B, o->d_surf_hdr, o->d_surf_coords, o->d_surf_nxy, pixels, d_surface, ctx->stream);
    CFEAR_HIP_CHECK(ctx, hipGetLastError());
  }
  return cap_rc;
}

int cfear_odometry_cov_samples(cfear_ctx* ctx, cfear_odometry* o, int sequence, double* costs, int* sampled) {
  if (!ctx || !o || sequence < 0 || sequence >= o->B || (!costs && !sampled)) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_cov_samples: bad argument");
  if (!o->cov_on) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_cov_samples: cost sampling is off (cfear_odometry_set_cov_sampling)");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  CFEAR_TRY(odo_join(ctx, o));
  CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (costs) CFEAR_HIP_CHECK(ctx, hipMemcpy(costs, o->d_cov_costs + (size_t)sequence * o->cov_m, sizeof(double) * o->cov_m, hipMemcpyDeviceToHost));
  if (sampled) {
    CovSampleCtx c;
    CFEAR_HIP_CHECK(ctx, hipMemcpy(&c, o->d_cov_ctx + sequence, sizeof(c), hipMemcpyDeviceToHost));
    *sampled = c.n >= 2 ? c.sampled : 0;
  }
  return odo_capacity_check(ctx, o, "odometry_cov_samples");
}

}  // extern "C"
