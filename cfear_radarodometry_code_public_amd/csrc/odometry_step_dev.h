// odometry_step_dev.h -- one sweep of one sequence of the batched odometry (OdometryKeyframeFuser::processFrame,
// odometrykeyframefuser.cpp:143-259, split after the feature build :161): the device-side state, the kernel parameter block,
// the launchers of the translation units that compile it and the two step bodies, shared by pipeline.hip (one launch per stage
// and sweep), register_step.hip / register_step_large.hip (the registration stage in other shapes) and replay.hip (a persistent
// workgroup per sequence that walks a whole chunk of sweeps).
#pragma once
#include "registration_dev.h"
#include "features_compact_dev.h"

#include <type_traits>

using namespace cfear_dev;

// ---- what the host and every translation unit see alike: the kernels' parameter blocks and the launchers -----------------------------
// Nothing here depends on a per-unit macro (CFEAR_REG_MAX_SCANS, CFEAR_REG_BLOCK, CFEAR_MATCH_LDS_CAP, ...): one definition, one layout.
namespace cfear_dev {
constexpr int MAX_SCANS = 64;  // keyframes + current: the layout of SeqState in memory (whatever CFEAR_REG_MAX_SCANS a unit compiles its registration for)

// Global per-sequence working memory (also one per context for the per-call API).
struct BlockScratch {
  uint64_t* keys; float* spts; int* order; int* vstart; int* vlist;  // big-cloud fallbacks of the LDS arrays
  int* vcur;        // [GRID_CAP + 2]
  int* rng;         // [cap_points][8] candidate row ranges per sample point
  double* part;     // [7][cap_points] partial cell moments per candidate chunk
  int* tmpi;        // [2 * cap_points + 16]
  float* samples;   // [cap_points * 3]
  double* match;    // [8][pair_cap]
  int* assoc;       // [3 * pair_cap]
  int cap_points, p2cap, pair_cap;
  const int* vrank; const int* vperm;  // FeatureScratch::vrank / vperm (cfear_scan_create under cfear_tune VOXEL_ORDER = 1; null otherwise)
};

struct SeqState {  // OdometryKeyframeFuser members (odometrykeyframefuser.h:203-260) for one sequence
  Aff2 T_prev, Tmot, Tcurrent;
  int nkf, free_slot, frames, last_slot;
  int ring[MAX_SCANS];
  Aff2 kf_pose[MAX_SCANS];
};

// Cost-sampling covariance (estimate_cov_by_sampling, odometrykeyframefuser.cpp:202-208, 261-380) of the batched routes: what the
// registration of a sweep used - its scans and poses before AddToReference may hand the oldest slot to the next sweep - written by
// register_step_body when CovSampling::ctx is set, read by the sampling stage (cov_sampling_dev.h) before the next sweep's features run.
struct CovSampleCtx {
  int n;              // scans of the registration (keyframes + current); 0: nothing to sample this sweep (a sequence's first)
  int itr;            // radar_reg->itr_ after Register: the sweep's outer iterations (selects the association radius of GetCost)
  int num_residuals;  // of the registration's last problem (GetCovarianceScaler)
  int sampled;        // cov_sampled_success of the last sampling (written by the sampling stage)
  int soft;           // the registration ran soft (cfear_fuser_options::soft_constraint): num_residuals / final_cost include the prior
                      // block where it joined; cfear_odometry_surface builds its problem with the prior too
  int pad_;
  double final_cost;
  int slot[MAX_SCANS];
  double pose[3 * MAX_SCANS];  // the registration's parameter vectors after the solve: keyframes, then the registered pose (T_vek)
};
struct CovSampling {  // null ctx: off (the production kernels do exactly the work they did without the option)
  CovSampleCtx* ctx;    // [B]
  const double* pinv;   // [10][m] minimum-norm pseudo-inverse of the sample design (odometrykeyframefuser.cpp:325-337)
  const double* offs;   // [m][3] sample offsets (x, y, yaw) in the reference's order (:294-296)
  double* costs;        // [B][m] sampled costs of the last sampling
  double* cov_out;      // optional [B][36]: cov_current after the sweep (cfear_odometry_replay_*_cov; set per sweep)
  double scaler;        // cov_sampling_covariance_scaler
  int m;                // samples_per_axis^3
};

struct OdoParams {
  FeatureParams fp;
  RegParams rp;
  int A, k, compensate, ccw, use_keyframe, submap;
  double min_keyframe_dist, min_keyframe_rot_deg;
  long long* phase_times;  // optional [B][32] wall_clock64 ticks (tools/)
  long long* wg_times;     // optional [B][32]: start / end clock of every workgroup of the PRODUCTION kernels (slots 0, 1 features;
                           // 14, 15 registration) - two clock reads per workgroup, off the critical path
  int phase_detail;        // also accumulate the evaluation / controller times of every LM command (three clock reads per command:
                           // the registration kernel runs at half speed with them)
  int seq0;  // first sequence of this launch (sub-batches run on their own streams)
  // the scan slots of all sequences are one allocation, slot j of sequence q at scans_base + scan_stride * (q * (submap + 1) + j):
  // computed, not fetched from the pointer table (a memory round trip at the start of both kernels)
  unsigned char* scans_base; size_t scan_stride;
  cfear_sweep_record* records;  // optional [B]: this sweep's record of every sequence (cfear_odometry_replay_host)
  // registration workgroups longest first (cfear_tune REGISTRATION_ORDER): order[blockIdx.x] = the sequence a workgroup takes (null:
  // seq0 + blockIdx.x), work[q] = what sequence q's registration of THIS sweep cost (evaluations x residual blocks + associations),
  // the key the next sweep's order is sorted by (null: not recorded)
  const int* order; unsigned* work;
  CovSampling cs;  // cost-sampling covariance and / or per-sweep covariances (cs.ctx / cs.cov_out null: neither)
  int* flags;  // word 0 for the odometry object, word 1 + q for sequence q: bit 0 = some scan had more cells than its block holds, bit 1 = some cloud had more points
               // than the object is sized for (both CFEAR_ERR_CAPACITY); null: cannot happen
  // per-sequence parameters, input sweeps and fuser options (cfear_odometry_set_sequence_params / _set_sequence_sources /
  // _set_fuser_options): [B] rows, row q for sequence q. null: every sequence runs with the values above, reads sweep q and keeps the
  // fuser's defaults (the production kernels do exactly the work they did without it)
  const SeqParams* seq;
  int n_sources;  // sweeps per step in the filter's output (the sequences when there is no source map)
};
// sequence q's row, or null without a table. The table pointer and q are the same in every lane of a workgroup; read through the first
// lane they are uniform for the compiler too, wherever OP lives (a kernel argument; the LDS copy of the persistent replay kernels), so the
// row's fields arrive as scalar loads
__device__ __forceinline__ SeqRow seq_row(const OdoParams& OP, int q) {
  const unsigned long long a = (unsigned long long)OP.seq;
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)a), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(a >> 32));
  const SeqParams* t = (const SeqParams*)(((unsigned long long)hi << 32) | lo);
  return t ? (SeqRow)(t + __builtin_amdgcn_readfirstlane(q)) : (SeqRow) nullptr;
}

static_assert(sizeof(SeqState) == 3 * sizeof(Aff2) + 4 * sizeof(int) + MAX_SCANS * (sizeof(int) + sizeof(Aff2)), "SeqState is sized by the fixed MAX_SCANS");
static_assert(sizeof(CovSampleCtx) == 6 * sizeof(int) + sizeof(double) + MAX_SCANS * (sizeof(int) + 3 * sizeof(double)), "CovSampleCtx is sized by the fixed MAX_SCANS");
static_assert(std::is_trivially_copyable<OdoParams>::value && std::is_trivially_copyable<BlockScratch>::value && std::is_trivially_copyable<SeqState>::value,
              "kernel arguments and device state are copied byte for byte");
}  // namespace cfear_dev

// The launchers that cross translation units (each unit compiles the step bodies below for its own workgroup shape), called by pipeline.hip.
// register_step.hip: the batched registration step kernel for registrations of up to CFEAR_STEP_SMALL_SCANS scans
__attribute__((visibility("hidden"))) void cfear_launch_register_step_small(const OdoParams& P, int count, hipStream_t st, SeqState* states, const BlockScratch* scratch,
                                                                           double* cov_work, cfear_reg_summary* summaries, double* poses_out);
// register_step_large.hip: ... of more scans (submap_scan_size 8 .. 63), a compute unit per registration
__attribute__((visibility("hidden"))) void cfear_launch_register_step_large(const OdoParams& P, int count, hipStream_t st, SeqState* states, const BlockScratch* scratch,
                                                                           double* cov_work, cfear_reg_summary* summaries, double* poses_out);
// replay.hip: features -> registration of `cnt` consecutive sweeps of every sequence in one launch (a persistent workgroup per sequence)
__attribute__((visibility("hidden"))) void cfear_launch_replay_chunk(const uint32_t* d_slots, int cnt, int B, const double* d_trig, const OdoParams& OP, SeqState* states,
                                                                    const BlockScratch* scratch, double* cov_work, cfear_reg_summary* summaries, double* poses_out,
                                                                    cfear_sweep_record* records, hipStream_t stream);
// ... from the clouds of a chunk ([cnt][B][cap][3] floats, [cnt][B] counts) instead of slots
__attribute__((visibility("hidden"))) void cfear_launch_replay_chunk_cloud(const float* d_xyi, int cap, const int* d_counts, int cnt, int B, const OdoParams& OP,
                                                                          SeqState* states, const BlockScratch* scratch, double* cov_work,
                                                                          cfear_reg_summary* summaries, double* poses_out, cfear_sweep_record* records, hipStream_t stream);
// A registration step kernel KERNEL<TIMED, KCOST> of this unit on `st`: one instantiation per cost metric (the evaluation inline, no run-time
// dispatch), the per-phase timers with the cost read at run time. The arguments after `st` are the kernel's, behind the OdoParams P.
#define CFEAR_LAUNCH_REG_BY_COST(KERNEL, P, count, st, ...)                                                                                          \
  do {                                                                                                                                               \
    if ((P).phase_times) hipLaunchKernelGGL((KERNEL<true, -1>), dim3(count), dim3(BLOCK_R), 0, st, P, __VA_ARGS__);                                   \
    else if ((P).rp.cost == CFEAR_COST_P2L) hipLaunchKernelGGL((KERNEL<false, CFEAR_COST_P2L>), dim3(count), dim3(BLOCK_R), 0, st, P, __VA_ARGS__);  \
    else if ((P).rp.cost == CFEAR_COST_P2D) hipLaunchKernelGGL((KERNEL<false, CFEAR_COST_P2D>), dim3(count), dim3(BLOCK_R), 0, st, P, __VA_ARGS__);  \
    else hipLaunchKernelGGL((KERNEL<false, CFEAR_COST_P2P>), dim3(count), dim3(BLOCK_R), 0, st, P, __VA_ARGS__);                                     \
  } while (0)

namespace {

constexpr int BLOCK_F = CFEAR_FEAT_BLOCK;   // features / cloud kernels: two workgroups per compute unit (features_compact_dev.h)
constexpr int BLOCK_R = CFEAR_REG_BLOCK;   // registration kernels: 256 threads (4 waves = one per SIMD) in pipeline.hip
static_assert(BLOCK_R >= 64 * CFEAR_EVAL_WAVES, "the controller sums the partial results of CFEAR_EVAL_WAVES waves unconditionally");
static_assert(CFEAR_REG_MAX_SCANS <= MAX_SCANS, "a registration cannot have more scans than a sequence keeps");
static_assert(FeatLdsC::total <= 80384, "two feature workgroups per compute unit");
struct RegLds {  // registration kernels
  static constexpr size_t red_d = 0;                                  // 10 sums x CFEAR_RED_STRIDE waves
  static constexpr size_t par = red_d + 10 * CFEAR_RED_STRIDE * sizeof(double);        // 3*CFEAR_REG_MAX_SCANS doubles
  static constexpr size_t red_i = par + 3 * CFEAR_REG_MAX_SCANS * sizeof(double);  // 64 ints
  static constexpr size_t scanptr = red_i + 64 * sizeof(int);        // CFEAR_REG_MAX_SCANS pointers
  static constexpr size_t regsh = scanptr + CFEAR_REG_MAX_SCANS * sizeof(void*);  // RegShared
  static constexpr size_t total = (regsh + sizeof(RegShared) + 15) / 16 * 16;
};

#ifndef CFEAR_REG_LDS_BUDGET
#define CFEAR_REG_LDS_BUDGET 53760  // three registration workgroups per compute unit (replay.hip: one, with the whole unit's LDS)
#endif
static_assert(RegLds::total + sizeof(double) * CFEAR_MATCH_LDS_DOUBLES <= CFEAR_REG_LDS_BUDGET,
              "registration kernels: more than 53,760 B of LDS costs the third workgroup per compute unit");

__device__ inline int next_pow2(int n) { int p = 1; while (p < n) p <<= 1; return p; }

// working memory of one feature build: global arrays of the general path (clouds beyond the compact path's limits) + the two
// LDS reduction arrays
__device__ __forceinline__ FeatureScratch make_fscratch(const BlockScratch& B, unsigned char* lds) {
  FeatureScratch W;
  W.keys = B.keys; W.spts = B.spts; W.order = B.order; W.vstart = B.vstart; W.vlist = B.vlist;
  W.vcur = B.vcur; W.lds = false; W.tab_voxels = 0;
  W.rng = B.rng; W.part = B.part; W.tmpi = B.tmpi;
  W.cap = B.cap_points;
  W.vrank = B.vrank; W.vperm = B.vperm;
  W.samples = B.samples;
  W.red_i = reinterpret_cast<int*>(lds + FeatLdsC::red_i);
  W.red_f = reinterpret_cast<float*>(lds + FeatLdsC::red_f);
  return W;
}
// cfear_tune NN_TIE_RULE = 2: one thread builds the scan's kd-tree (kdtree_flann_dev.h) over the float cell means; the activation stack of the
// build lives in the partial-moment scratch (free once the cells exist). A scan without the arrays (created before the mode was switched on)
// or a stack that does not suffice is reported through the scan's status.
__device__ inline void kd_build_block(ScanDev* S, const BlockScratch& B) {
  __syncthreads();
  if (threadIdx.x == 0) {
    const int frames = (int)(((size_t)7 * B.cap_points * sizeof(double)) / sizeof(KdFrame));
    const bool ok = S->kd.nodes && kd_build_serial(&S->kd, S->mean_f, S->n_cells, reinterpret_cast<KdFrame*>(B.part), frames);
    if (!ok && S->status == 0) S->status = CFEAR_ERR_UNSUPPORTED;
  }
  __syncthreads();
}
// byte_intensities: every intensity of the cloud is an integer in 0..255 (block-uniform; always true for clouds made from
// the filter's slots) - the compact path keeps them as bytes
// (the batched cloud pass leaves the cloud in registers only: the general path needs it in memory and writes it first)
__device__ __forceinline__ void features_dispatch(ScanDev* S, int n, const FeatureParams& P, const BlockScratch& B,
                                                  unsigned char* lds, PhaseTimer* pt, const float* bounds, bool zeroed, bool byte_intensities,
                                                  const PointRegs& PR, bool registers_only = false) {
  const FeatureScratch W = make_fscratch(B, lds);
  if (!(byte_intensities && !W.vrank && features_block_c(S, n, P, W, lds, pt, bounds, zeroed, PR))) {  // (a given voxel order: the general path)
    // registers_only (a constant of the call site): the cloud pass may have left the cloud in registers only (byte intensities)
    if (registers_only && PR.rounds > 0) point_regs_to_global(PR, S->xyi);  // block-uniform
    features_block(S, n, P, W, next_pow2(n), pt, bounds);
  }
  if (P.nn_tie == 2) kd_build_block(S, B);  // parity mode: the kd-tree FLANN builds over the cell means (ComputeSearchTreeFromCells, pointnormal.cpp:151-162)
}
__device__ inline RegScratch make_rscratch(const BlockScratch& B, unsigned char* lds) {
  RegScratch W;
  const size_t c = (size_t)B.pair_cap;
  W.tmx = B.match; W.tmy = B.match + c; W.a0 = B.match + 2 * c; W.a1 = B.match + 3 * c; W.a2 = B.match + 4 * c;
  W.sx = B.match + 5 * c; W.sy = B.match + 6 * c; W.w = B.match + 7 * c;
  W.assoc = B.assoc; W.cap = B.pair_cap; W.acap = 3 * B.pair_cap;  // (scratch_layout: three ints per pair)
  W.red = reinterpret_cast<double*>(lds + RegLds::red_d);
  W.red_i = reinterpret_cast<int*>(lds + RegLds::red_i);
  return W;
}

// ---- batched odometry: OdometryKeyframeFuser::processFrame (odometrykeyframefuser.cpp:143-259) with all
// state on the device, split after the feature build (:161) ------------------------------------------
// TIMED: per-phase timestamps (tools/); the production instantiation carries no timer at all
template <bool TIMED>
__device__ __forceinline__ void features_step_body(unsigned char* lds /* FeatLdsC::total bytes */, int q, const uint32_t* slots_all, const double* trig,
                                                   const OdoParams& OP, const SeqState* states, const BlockScratch* scratch) {
  const SeqState* st = &states[q];
  const BlockScratch B = scratch[q];
  ScanDev* cur = reinterpret_cast<ScanDev*>(OP.scans_base + OP.scan_stride * ((size_t)q * (OP.submap + 1) + st->free_slot));
  const Aff2 TprevMot = st->Tmot;  // :146
  PhaseTimer pt; pt.t = (TIMED && OP.phase_times) ? OP.phase_times + (size_t)q * 32 : nullptr; pt.n = 0; pt.cap = 14; pt.acc = nullptr;
  if (TIMED) pt.mark();
  if (!TIMED && OP.wg_times && threadIdx.x == 0) OP.wg_times[(size_t)q * 32] = (long long)wall_clock64();
  // the voxel bitmap starts all-zero (cleared here: the barriers of the cloud pass publish it)
  {
    uint32_t* z = reinterpret_cast<uint32_t*>(lds + FeatLdsC::bm);
    for (int i = threadIdx.x; i < (int)((FeatLdsC::bmp - FeatLdsC::bm) / 4); i += BLOCK_F) z[i] = 0u;
  }
  // stage 1 (second half) + 1.5: slots -> cloud (radar_driver.cpp:59), motion compensation (:147-150), bounding box
  double mot[3]; aff_to_xyt(TprevMot, mot);
  float bounds[4];
  PointRegs PR;
  // the sequence's own values where it has a row: the sweep it reads, its z_min (applied to the slots of a filter that ran with the smallest
  // z_min of the object: the k strongest above z are the members above z of the k strongest above any z' <= z), compensation, res, weights
  // ... and its k_strongest: the filter ran with the context's K (OP.k, the stride of a bearing's slots); the k strongest of a bearing are the
  // last k of the returns it kept (ascending, in front of the bearing's K slots), so the cloud pass reads that window
  FeatureParams fp = OP.fp;
  int src = q, compensate = OP.compensate, z_min = 0, k = OP.k;
  if (const SeqRow row = seq_row(OP, q)) {
    src = row->source; compensate = row->compensate; z_min = row->z_min; k = row->k;
    fp.radius = row->radius; fp.weight_intensity = row->weight_intensity;
  }
  // (the compact feature path works from the registers: the 58 KB of the cloud are only written when somebody reads them)
  const int n = cloud_step_block(slots_all + (size_t)src * OP.A * OP.k, OP.A, k, OP.k, trig, OP.fp.range_res, OP.fp.min_distance, z_min,
                                 cur->xyi, cur->cap_points, compensate, mot[0], mot[1], mot[2], OP.ccw,
                                 reinterpret_cast<int*>(lds + FeatLdsC::red_i), reinterpret_cast<float*>(lds + FeatLdsC::red_f),
                                 reinterpret_cast<double*>(lds + FeatLdsC::pxy),  // 6 doubles per bearing where the sorted points go later
                                 (int)(CFEAR_CPT_CAP * 8 / (6 * sizeof(double))), bounds, PR, false,
                                 reinterpret_cast<int*>(lds + FeatLdsC::vst), (int)((FeatLdsC::pxy - FeatLdsC::vst) / sizeof(int)));  // (free until the feature build)

  if (TIMED) { pt.mark(); pt.mark(); }
  CFEAR_STOP_AT(1, );
  features_dispatch(cur, n, fp, B, lds, TIMED ? &pt : nullptr, n > 0 ? bounds : nullptr, true, true, PR, true);  // :161
  if (OP.flags && threadIdx.x == 0 && cur->status == CFEAR_ERR_CAPACITY) { atomicOr(OP.flags, 1); OP.flags[1 + q] |= 1; }  // (thread 0 wrote the status itself; word 1 + q: this sequence's own)
  if (!TIMED && OP.wg_times && threadIdx.x == 0) OP.wg_times[(size_t)q * 32 + 1] = (long long)wall_clock64();
}

// The same stage from a CLOUD on the device (filter_type CA-CFAR, radar_driver.cpp:52-56, or cfear_odometry_step_cloud_device): sequence
// q's points are xyi_all + q * cap * 3, min(counts[q], cap) of them. Compensate (odometrykeyframefuser.cpp:146-150, utils.cpp:96-113:
// atan2 / sin / cos per point as written - a detector's points do not sit on bearing rays the per-bearing table of cloud_step_block
// could expand around) and MapPointNormal (:161) through the same dispatch as cfear_scan_create: the compact path when the cloud fits
// it (byte intensities, <= 4864 points), the general path in the sequence's global arrays otherwise.
__device__ __forceinline__ void features_cloud_step_body(unsigned char* lds /* FeatLdsC::total bytes */, int q, const float* xyi_all, int cap, const int* counts,
                                                         const OdoParams& OP, const SeqState* states, const BlockScratch* scratch) {
  const SeqState* st = &states[q];
  const BlockScratch B = scratch[q];
  ScanDev* cur = reinterpret_cast<ScanDev*>(OP.scans_base + OP.scan_stride * ((size_t)q * (OP.submap + 1) + st->free_slot));
  const Aff2 TprevMot = st->Tmot;  // :146
  if (OP.wg_times && threadIdx.x == 0) OP.wg_times[(size_t)q * 32] = (long long)wall_clock64();
  int n = counts[q];
  bool clipped = false;
  if (n > cap) { n = cap; clipped = true; }
  if (n > cur->cap_points) { n = cur->cap_points; clipped = true; }
  if (n < 0) n = 0;
  if (clipped && OP.flags && threadIdx.x == 0) { atomicOr(OP.flags, 2); OP.flags[1 + q] |= 2; }  // more detections than the object is sized for (cfar_max_points)
  const float* src = xyi_all + 3 * (size_t)q * cap;
  int bytes = 1;
  for (int i = threadIdx.x; i < n; i += BLOCK_F) {
    const float x = src[3 * i], y = src[3 * i + 1], w = src[3 * i + 2];
    cur->xyi[3 * i] = x; cur->xyi[3 * i + 1] = y; cur->xyi[3 * i + 2] = w;
    bytes &= (w >= 0.f && w <= 255.f && w == (float)(int)w) ? 1 : 0;
  }
  const bool byte_intensities = __syncthreads_and(bytes) != 0;  // (the barrier also makes the copy visible to the whole block)
  FeatureParams fp = OP.fp;
  int compensate = OP.compensate;
  if (const SeqRow row = seq_row(OP, q)) {  // (z_min and the source belong to the filter in front: uniform on this route)
    compensate = row->compensate; fp.radius = row->radius; fp.weight_intensity = row->weight_intensity;
  }
  if (compensate) {
    double mot[3]; aff_to_xyt(TprevMot, mot);
    compensate_block(cur->xyi, n, mot[0], mot[1], mot[2], OP.ccw);  // :147 (the peaks cloud of :149 is empty and never read)
  }
  PointRegs PR;
  point_regs_from_global(cur->xyi, n, PR);
  features_dispatch(cur, n, fp, B, lds, nullptr, nullptr, false, byte_intensities, PR);  // :161
  if (OP.flags && threadIdx.x == 0 && cur->status == CFEAR_ERR_CAPACITY) { atomicOr(OP.flags, 1); OP.flags[1 + q] |= 1; }
  if (OP.wg_times && threadIdx.x == 0) OP.wg_times[(size_t)q * 32 + 1] = (long long)wall_clock64();
}

template <bool TIMED, int KCOST = -1>
__device__ __forceinline__ void register_step_body(unsigned char* lds /* RegLds::total bytes */, int q, const OdoParams& OP, SeqState* states,
                                                   const BlockScratch* scratch, double* cov_work /*[B][36]*/, cfear_reg_summary* summaries,
                                                   double* poses_out /*[B][3]*/) {
  const int tid = threadIdx.x;
  SeqState* st = &states[q];
  const BlockScratch B = scratch[q];
  const int nslots = OP.submap + 1;
  auto slot_ptr = [&](int j) -> ScanDev* { return reinterpret_cast<ScanDev*>(OP.scans_base + OP.scan_stride * ((size_t)q * nslots + j)); };
  const int cur_slot = st->free_slot;
  ScanDev* cur = slot_ptr(cur_slot);
  const Aff2 T_prev = st->T_prev, TprevMot = st->Tmot;
  const int nkf = st->nkf;
  // this thread's keyframe (threads below nkf), read with the rest of the state: one round trip, before the barrier
  const int my_ring = st->ring[tid < MAX_SCANS ? tid : 0];
  const Aff2 my_kf_pose = st->kf_pose[tid < MAX_SCANS ? tid : 0];
  PhaseTimer pt; pt.t = (TIMED && OP.phase_times) ? OP.phase_times + (size_t)q * 32 + 14 : nullptr; pt.n = 0; pt.cap = 15;
  pt.acc = (TIMED && OP.phase_times && OP.phase_detail) ? OP.phase_times + (size_t)q * 32 + 29 : nullptr;
  pt.acc2 = (TIMED && OP.phase_times && OP.phase_detail == 2) ? OP.phase_times + (size_t)q * 32 : nullptr;  // (over the feature kernel's stamps)
  if (TIMED && pt.acc2 && tid == 0) for (int i = 0; i < 8; i++) pt.acc2[i] = 0;
  if (TIMED) pt.mark();
  if (!TIMED && OP.wg_times && tid == 0) OP.wg_times[(size_t)q * 32 + 14] = (long long)wall_clock64();
  // the fuser's switches of this sequence (cfear_fuser_options; no row: the defaults). Read here and again after the solve: nothing of
  // the row stays in registers across it
  int fopt = 0;
  if (const SeqRow row = seq_row(OP, q)) fopt = row->fuser;
  const Aff2 Tguess = (fopt & SEQ_FUSER_NO_GUESS) ? T_prev : aff_mul(T_prev, TprevMot);  // :165-168 (use_guess)
  cfear_reg_summary* sum = &summaries[q];
  __syncthreads();  // every thread has read the state before thread 0 rewrites it
  if (nkf == 0) {  // :171-177
    if (tid == 0) {
      if (OP.cs.ctx) OP.cs.ctx[q].n = 0;  // no keyframes: no sampling
      st->ring[0] = cur_slot; st->kf_pose[0] = aff_identity(); st->nkf = 1; st->free_slot = (cur_slot + 1) % nslots;
      st->frames++; st->last_slot = cur_slot;
      if (OP.work) OP.work[q] = 0u;
      sum->success = 0; sum->usable = 0; sum->outer_iterations = 0; sum->num_residuals = 0; sum->num_residual_blocks = 0;
      double v[3]; aff_to_xyt(st->Tcurrent, v);
      poses_out[3 * q] = v[0]; poses_out[3 * q + 1] = v[1]; poses_out[3 * q + 2] = v[2];
      if (OP.records) {
        cfear_sweep_record* r = OP.records + q;
        r->pose[0] = v[0]; r->pose[1] = v[1]; r->pose[2] = v[2]; r->final_cost = 0;
        r->outer_iterations = 0; r->num_residuals = 0; r->n_keyframes = 1; r->n_cells = cur->n_cells;
        for (int i = 0; i < 8; i++) r->inner_iterations[i] = 0;
      }
    }
    return;
  }
  // FormatScans (:478-494)
  ScanDev** sp = reinterpret_cast<ScanDev**>(lds + RegLds::scanptr);
  double* poses = reinterpret_cast<double*>(lds + RegLds::par);  // the registration's parameter array itself: the poses never go through memory
  const int ns = nkf + 1;
  if (tid < nkf) {
    sp[tid] = slot_ptr(my_ring);
    double v[3]; aff_to_xyt(my_kf_pose, v);
    poses[3 * tid] = v[0]; poses[3 * tid + 1] = v[1]; poses[3 * tid + 2] = v[2];
  }
  if (tid == 0) {
    sp[ns - 1] = cur;
    double v[3]; aff_to_xyt(Tguess, v);
    poses[3 * (ns - 1)] = v[0]; poses[3 * (ns - 1) + 1] = v[1]; poses[3 * (ns - 1) + 2] = v[2];
  }
  // cov_vek.back() as FormatScans leaves it (Identity66, :486-490): what cov_current is when the registration has no usable
  // solution (it is in/out for register_block); read back through cfear_odometry_covariances
  if (tid >= 64 && tid < 100) cov_work[(size_t)q * 36 + (tid - 64)] = ((tid - 64) % 7 == 0) ? 1.0 : 0.0;
  __syncthreads();
  const RegScratch RW = make_rscratch(B, lds);
  // soft_constraint (:186): the prior's covariance is cov_vek.back(), the Identity66 just written (read by the controller wave before
  // anything writes the covariance); its centre is the normalised Tguess, its weight sqrt(#cells of the current scan) (register_block)
  register_block<KCOST>(sp, ns, poses, cov_work + (size_t)q * 36, OP.rp, RW, reinterpret_cast<double*>(lds + RegLds::par),
                 reinterpret_cast<RegShared*>(lds + RegLds::regsh), sum, TIMED ? &pt : nullptr,
                 (fopt & SEQ_FUSER_SOFT) ? cov_work + (size_t)q * 36 : nullptr, seq_row(OP, q));  // :186 (result ignored, :184-186)
  __syncthreads();
  if (TIMED) pt.mark();
  if (tid == 0) {
    if (OP.cs.ctx) {  // estimate_cov_by_sampling: the scans and poses of this registration, before the sanity check and AddToReference (:202-208)
      CovSampleCtx* c = OP.cs.ctx + q;
      c->n = ns; c->itr = sum->outer_iterations; c->num_residuals = sum->num_residuals; c->final_cost = sum->final_cost;
      c->soft = reinterpret_cast<const RegShared*>(lds + RegLds::regsh)->prior_on;  // (the solver's own state: no option kept across the solve)
      for (int i = 0; i < nkf; i++) c->slot[i] = st->ring[i];
      c->slot[ns - 1] = cur_slot;
      for (int i = 0; i < 3 * ns; i++) c->pose[i] = poses[i];
    }
    Aff2 Tcurrent = aff_from_xyt(poses[3 * (ns - 1)], poses[3 * (ns - 1) + 1], poses[3 * (ns - 1) + 2]);  // :195
    const Aff2 Tpi = aff_inv(T_prev);
    const Aff2 Tmot_current = aff_mul(Tpi, Tcurrent);
    {  // AccelerationVelocitySanityCheck (:76-94)
      const double dt = 0.25, lim = 200;
      const double vel = sqrt(Tmot_current.t0 * Tmot_current.t0 + Tmot_current.t1 * Tmot_current.t1) / dt;
      const double ax = (Tmot_current.t0 - TprevMot.t0) / (dt * dt), ay = (Tmot_current.t1 - TprevMot.t1) / (dt * dt);
      const double acc = sqrt(ax * ax + ay * ay);
      if (acc > lim || vel > lim) Tcurrent = Tguess;  // :198-199
    }
    st->Tmot = aff_mul(Tpi, Tcurrent);  // :200
    st->Tcurrent = Tcurrent;
    const Aff2 Tkeydiff = aff_mul(aff_inv(st->kf_pose[nkf - 1]), Tcurrent);  // :227
    bool fuse = true;
    const SeqRow row = seq_row(OP, q);  // the sequence's own keyframe rule where it has a row
    if (row ? row->use_keyframe : OP.use_keyframe) {  // KeyFrameBasedFuse (:62-73)
      const double tn = sqrt(Tkeydiff.t0 * Tkeydiff.t0 + Tkeydiff.t1 * Tkeydiff.t1);
      const double rot = fabs(atan2(Tkeydiff.l2, Tkeydiff.l3));
      const double kd = row ? row->min_keyframe_dist : OP.min_keyframe_dist, kr = row ? row->min_keyframe_rot_deg : OP.min_keyframe_rot_deg;
      fuse = (tn > kd) || (rot > kr * 3.14159265358979323846 / 180.0);
    }
    if (fuse) {  // AddToReference (:470-476)
      int m = nkf;
      st->ring[m] = cur_slot; st->kf_pose[m] = Tcurrent; m++;
      int freed;
      // the ring's length is the sequence's own where it has a row (cfear_odometry_set_sequence_shapes; a row without shapes carries the
      // context's): s_q <= OP.submap keyframes live in slots 0 .. s_q of the OP.submap + 1 the sequence has
      if (m > (row ? (row->shape >> 2) : OP.submap)) {
        freed = st->ring[0];
        for (int i = 0; i + 1 < m; i++) { st->ring[i] = st->ring[i + 1]; st->kf_pose[i] = st->kf_pose[i + 1]; }
        m--;
      } else {
        freed = m;  // slots are handed out in increasing order until the ring is full
      }
      st->nkf = m; st->free_slot = freed;
    }
    st->T_prev = Tcurrent;  // :257
    st->frames++; st->last_slot = cur_slot;
    double v[3]; aff_to_xyt(Tcurrent, v);
    poses_out[3 * q] = v[0]; poses_out[3 * q + 1] = v[1]; poses_out[3 * q + 2] = v[2];
    if (OP.records) {  // what a caller of pointcloudCallback sees after this sweep, kept per sweep (no host round trip in a replay)
      cfear_sweep_record* r = OP.records + q;
      r->pose[0] = v[0]; r->pose[1] = v[1]; r->pose[2] = v[2]; r->final_cost = sum->final_cost;
      r->outer_iterations = sum->outer_iterations; r->num_residuals = sum->num_residuals; r->n_keyframes = st->nkf; r->n_cells = cur->n_cells;
      for (int i = 0; i < 8; i++) r->inner_iterations[i] = sum->inner_iterations[i];
    }
    if (OP.work) {  // from the solver state in LDS: no read-back of the summary from memory
      const RegShared* rs = reinterpret_cast<const RegShared*>(lds + RegLds::regsh);
      int evals = 0;
      for (int i = 0; i < rs->nrec; i++) evals += rs->orec[i].inner;
      const int nsrc = rs->kf[ns - 1].n_cells;
      OP.work[q] = (unsigned)evals * (unsigned)rs->M + 6u * (unsigned)rs->nrec * (unsigned)(nkf * nsrc);
    }
    if (!TIMED && OP.wg_times) OP.wg_times[(size_t)q * 32 + 15] = (long long)wall_clock64();
  }
}


#ifndef CFEAR_REG_MIN_WG
#define CFEAR_REG_MIN_WG 3  // workgroups per compute unit the registration step kernel is compiled for (tools: A/B builds)
#endif
// KCOST: the cost metric the kernel is compiled for (registration_dev.h evaluate_partial), -1: any (the timed instantiation)
#ifdef CFEAR_REG_NUM_VGPR  // tools/reg_resources.sh: cap the architectural VGPRs below the occupancy budget (the rest of it: AGPRs for spills)
#define CFEAR_REG_VGPR_ATTR __attribute__((amdgpu_num_vgpr(CFEAR_REG_NUM_VGPR)))
#else
#define CFEAR_REG_VGPR_ATTR
#endif
// (the two unused parameters are launched as null: dropping them changes the kernarg layout and with it the code generated for this kernel)
template <bool TIMED, int KCOST>
__global__ __launch_bounds__(BLOCK_R, CFEAR_REG_MIN_WG) CFEAR_REG_VGPR_ATTR void register_step_kernel(OdoParams OP, SeqState* states, ScanDev* const* /*unused*/,
                                                                const BlockScratch* scratch, double* /*unused*/,
                                                                double* cov_work /*[B][36]*/, cfear_reg_summary* summaries,
                                                                double* poses_out /*[B][3]*/) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[RegLds::total];
  register_step_body<TIMED, KCOST>(lds, OP.order ? OP.order[blockIdx.x] : OP.seq0 + (int)blockIdx.x, OP, states, scratch, cov_work, summaries, poses_out);
}

}  // namespace
