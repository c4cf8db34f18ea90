// pipeline.hip -- the kernels unit: every kernel of stages 1.5-3, per call and per batched step, and the functions that launch them.
// Interface contract + reference citations: include/cfear_hip.h. Device code: features_dev.h,
// registration_dev.h.
// No entry point of the public API lives here. A unit is one optimisation domain - a kernel moved out of it compiles to other code, and so
// do the kernels it leaves behind ("Which unit holds what") - so the kernels stay and the host code around them went:
// the per-call API to percall.hip, the cov / surface routes of the batched object to odometry_cov.hip, both over the typed launch
// functions at the end of this file (pipeline_launch.h); the layouts of scans and scratch to scan_layout.h.
//
// One radar sweep of B independent sequences = three launches on the context stream, no host round trip:
//   kstrongest_kernel      (kstrongest.hip)  B*A wavefront-rows, HBM streaming
//   features_step_kernel   one 512-thread workgroup per sequence (79,680 B of LDS, two per compute unit): cloud + motion
//                          compensation, voxel bitmap + counting sort, chunked cell statistics, cell-mean grid
//   register_step_kernel   one 256-thread workgroup per sequence (53 KB LDS incl. the match array, three per compute
//                          unit so that the serial Levenberg-Marquardt controllers of different sequences overlap):
//                          association, robust normal equations, LM, outer loop, keyframe logic
// The per-call kernels (clouds, scans, Register, GetCost, GetSurface, cost-sampling covariance) use the same device code.
// The object itself (struct cfear_odometry) is odometry_obj.h's; its life - creation, reset, destruction, the step entry points, the profile,
// the replay and the plain reads - is odometry_run.hip's, over the launch layer of this file (odo_params, odo_launch_sweep, odo_launch_cfar); its per-sequence configuration - the setters and getters of rows, source
// map, shapes, detectors and fuser options, the device table (seq_table_upload) and odo_seq_sync's re-check - lives in odometry_seq.hip
// over seq_config.h. This file reads the configuration through o->cfg (effective(), sources(), other_cost()) and never writes it.
// The keyframe graph - its kernels, its log (o->kf), its setters and reading routes - is keyframes.hip's: the sweep here launches its two
// stages.
#include <math.h>
#include <cmath>
#include <stdlib.h>

#include <algorithm>
#include <new>

#include "odometry_obj.h"
#include "odometry_plan.h"
#include "cov_sampling_dev.h"
#include "scan_layout.h"
#include "pipeline_launch.h"

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
}  // namespace

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

// ---- the per-call kernels as launch functions (pipeline_launch.h): percall.hip and odometry_cov.hip run them ------------------------
static CloudOut cloud_out(cfear_cloud* c) {
  CloudOut o; o.xyi = c->d_xyi; o.d_n = c->d_n; o.cap = c->cap;
  o.h_xyi = c->h_block ? c->h_xyi() : nullptr; o.h_n = c->h_block ? c->h_n() : nullptr;
  return o;
}
void cfear_launch_cloud(const uint32_t* d_slots, int A, int k, const double* d_trig, float range_res, float min_distance, cfear_cloud* c0, cfear_cloud* c1,
                        hipStream_t st) {
  hipLaunchKernelGGL(cloud_kernel, dim3(c1 ? 2 : 1), dim3(BLOCK_F), 0, st, d_slots, A, k, d_trig, range_res, min_distance, cloud_out(c0), cloud_out(c1 ? c1 : c0));
}
void cfear_launch_compensate(cfear_cloud* c0, cfear_cloud* c1, double m0, double m1, double m2, int ccw, hipStream_t st) {
  hipLaunchKernelGGL(compensate_kernel, dim3(c1 ? 2 : 1), dim3(BLOCK_F), 0, st, cloud_out(c0), cloud_out(c1 ? c1 : c0), m0, m1, m2, ccw);
}
void cfear_launch_features(ScanDev* d_scan, const float* d_xyi, const int* d_n, const FeatureParams& P, const BlockScratch& B, hipStream_t st) {
  hipLaunchKernelGGL(features_kernel, dim3(1), dim3(BLOCK_F), 0, st, d_scan, d_xyi, d_n, P, B);
}
void cfear_launch_scan_from_cells(ScanDev* d_scan, int n, const FeatureParams& P, const BlockScratch& B, hipStream_t st) {
  hipLaunchKernelGGL(scan_from_cells_kernel, dim3(1), dim3(BLOCK_F), 0, st, d_scan, n, P, B);
}
void cfear_launch_closest(const ScanDev* d_scan, const double* d_q, int nq, double d, int* d_idx, int rule, hipStream_t st) {
  hipLaunchKernelGGL(closest_kernel, dim3((nq + 255) / 256), dim3(256), 0, st, d_scan, d_q, nq, d, d_idx, rule);
}
void cfear_launch_register(ScanDev* const* d_scans, int n, double* d_poses, double* d_cov6, const RegParams& P, const BlockScratch& B, cfear_reg_summary* d_out,
                           const double* d_prior_cov6, const TcLaunch* tc, hipStream_t st) {
  if (!tc) {
    hipLaunchKernelGGL(register_kernel, dim3(1), dim3(BLOCK_R), 0, st, d_scans, n, d_poses, d_cov6, P, B, d_out, d_prior_cov6);
    return;
  }
  hipLaunchKernelGGL(tc_prologue_kernel, dim3(std::max(1, (tc->cells + BLOCK_R - 1) / BLOCK_R)), dim3(BLOCK_R), 0, st, tc->src, tc->hdr, tc->view, tc->view_cells,
                     tc->vx, tc->vy, tc->vth, tc->ccw);
  if (hipPeekAtLastError() != hipSuccess) return;
  hipLaunchKernelGGL(register_tc_kernel, dim3(1), dim3(BLOCK_R), 0, st, d_scans, n, d_poses, d_cov6, P, B, d_out, d_prior_cov6, tc->hdr);
}
void cfear_launch_get_cost(ScanDev* const* d_scans, int n, const double* d_poses, const RegParams& P, const BlockScratch& B, int itr, double* d_score,
                           double* d_residuals, int cap, int* d_nres, hipStream_t st) {
  hipLaunchKernelGGL(get_cost_kernel, dim3(1), dim3(BLOCK_R), 0, st, d_scans, n, d_poses, P, B, itr, d_score, d_residuals, cap, d_nres);
}
void cfear_launch_get_cost_samples(ScanDev* const* d_scans, int n, const double* d_poses, const double* d_samples, int m, const RegParams& P, double* d_match,
                                   int* d_assoc, int cap, int itr, double* d_costs, int* d_nres, hipStream_t st) {
  hipLaunchKernelGGL(get_cost_samples_kernel, dim3(m), dim3(BLOCK_R), 0, st, d_scans, n, d_poses, d_samples, P, d_match, d_assoc, cap, itr, d_costs, d_nres);
}
bool cfear_surface_build_evaluates() { return CFEAR_SURFACE_NAIVE != 0; }
// (the three surface launchers stand in the order their kernels have always been instantiated in: the evaluation, the build of one
// problem, the build per step - the order decides where each lies in the code object)
// the evaluation of `problems` surfaces (surface_eval_kernel): two pixels per thread, or one where that leaves fewer than two
// workgroups per compute unit (a single surface)
void launch_surface_eval(const RegParams& P, int problems, const SurfHdr* d_hdr, const double* d_coords, const int* d_nxy, int pixels,
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
void cfear_launch_surface_build(ScanDev* const* d_scans, int n, const double* d_poses, const RegParams& P, const BlockScratch& B, int itr,
                                const double* d_prior_cov6, SurfHdr* d_hdr, const double* d_coords, const int* d_nxy, int pixels, double* d_out, hipStream_t st) {
  hipLaunchKernelGGL(surface_build_kernel<CFEAR_SURFACE_NAIVE != 0>, dim3(1), dim3(BLOCK_R), 0, st, d_scans, n, d_poses, P, B, itr, d_prior_cov6, d_hdr, d_coords,
                     d_nxy, pixels, d_out);
}
void cfear_launch_surface_build_step(const OdoParams& OP, int B, const BlockScratch* d_scratch, SurfHdr* d_hdr, const double* d_coords, const int* d_nxy, int pixels,
                                     double* d_out, hipStream_t st) {
  hipLaunchKernelGGL(surface_build_step_kernel<CFEAR_SURFACE_NAIVE != 0>, dim3(B), dim3(BLOCK_R), 0, st, OP, d_scratch, d_hdr, d_coords, d_nxy, pixels, d_out);
}
