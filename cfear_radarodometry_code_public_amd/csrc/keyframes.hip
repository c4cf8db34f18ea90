// keyframes.hip -- the keyframe graph of the batched odometry routes (gfx950 only). OdometryKeyframeFuser::processFrame ends a fused sweep
// with scan_ = RadarScan(Tcurrent, TprevMot, cloud_peaks, cloud, Pcurrent, t) and AddToGraph(keyframes_, scan_, cov_current)
// (odometrykeyframefuser.cpp:171-176, 234-248, 428-445): a node per keyframe (RadarScan, types.h:93-143) with its oriented surface
// points and one odometry Constraint3d (types.h:155-190) to the previous keyframe. Here:
//   keyframe_record_kernel  a stage of its own behind the registration stage, one workgroup per sequence: the sequences that fused
//                           append their node - and their scan's cells - to their own log. It reads what the stages left behind
//                           (SeqState, the scan in last_slot, cov_work); no other kernel knows of it.
//   keyframe_cloud_kernel   with a point log, in front of the recorder: the filtered and the peaks cloud of the sequences that fused.
//   keyframe_scans_kernel   the batched twin of scan_from_cells_kernel: a workgroup per scan rebuilds a per-call scan from the log.
//   keyframe_edges_kernel   constraints between ANY keyframes of a log (cfear_odometry_keyframe_edges): a workgroup per job registers
//                           keyframe `to` against 1 .. 16 fixed keyframes on scans rebuilt from the log and applies the constraint rule.
//   cfear_keyframe_constraint  the rule of AddToGraph :435-440 for the host (keyframe_constraint.h: one function for both sides).
// Behind the kernels the graph's host side: the log is cfear_odometry::kf (KeyframeLog, keyframe_dev.h). pipeline.hip's sweep launches the
// recorder and the cloud stage through the two launchers of that header; the setters (cfear_odometry_set_keyframe_recording / _clouds)
// and the reading routes (counts, nodes, cells, scans, edges, cloud sizes, cloud, clouds) are here. A scan rebuilt from the log is a per-call
// scan of percall.hip: cfear_scan_alloc makes the blank one, cfear_scan_release takes it back.
#include <algorithm>

#include "odometry_obj.h"
#include "keyframe_constraint.h"

namespace cfear_dev {
// One scan to rebuild from the log (cfear_odometry_keyframe_scans): the header of its block, its cells in the log and the working memory
// of its workgroup (the uniform grid's cursors; under NN_TIE_RULE = 2 the kd build's activation stack). Known to this unit only.
struct KfScanJob {
  ScanDev hdr;                     // written to the front of the block by the kernel (hdr's pointers point into the block)
  ScanDev* dst;                    // the block
  const cfear_keyframe_cell* src;  // n cells
  int n, part_doubles;
  int* vcur;                       // [CFEAR_GRID_CAP + 4]
  double* part;                    // [part_doubles], or null
};
// One job of cfear_odometry_keyframe_edges as its workgroup reads it: nodes of the job's sequence (their poses are read from the log on
// the device), positions in the call's scan table (every distinct keyframe of the call is rebuilt once) and the job's slice of the
// call's match / assoc arrays.
struct KfEdgeJob {
  int sequence, to, n_from, ref;
  int has_guess, to_scan, pair_cap, pad_;
  int from[CFEAR_KF_EDGE_MAX_FROM], from_scan[CFEAR_KF_EDGE_MAX_FROM];
  double guess[3];
  unsigned long long pair_off;  // the slice's first pair (a multiple of 64: the arrays of every slice start 256-byte aligned)
};
}  // namespace cfear_dev

namespace {

constexpr int BLOCK_K = 256;

// The cloud stage (cfear_odometry_set_keyframe_clouds): cloud_nopeaks_ and cloud_peaks_ of the RadarScan a fused sweep ends with
// (odometrykeyframefuser.cpp:147-149, 234-248; types.h:93-143), in front of the recorder on the same stream, a workgroup per sequence. A
// sequence that fused - the recorder's own test - writes both clouds behind the points its log holds and leaves its verdict in cloud_word;
// the recorder folds it into `fits` and commits the offsets, so only sequence q's workgroups touch q's words, in stream order.
//   k-strongest routes: the points the feature stage built its cells from, through the same code on the same slots - cloud_step_block with
//     the sequence's own row and the LDS layout of features_step_body (so the same branch, the same bearing table, the same bits) - and
//     the motion the sweep was compensated with (KfLog::tmot, before the recorder moves it on). The peaks cloud is the same pass over the
//     slots with the peak bit (getPeaksFilteredPointCloud(peaks = true) + Compensate, :149). The compaction is cloud_step_block's: ballots
//     per wave and one scan across the waves, row-major over (bearing, slot) - no atomics.
//   cloud routes (slots_all null): the compensated cloud sits in the scan's xyi (features_cloud_step_body); the peaks cloud is empty there
//     (radar_driver.cpp:52-56).
// A cloud that does not fit is cut at the room left (nothing is written past the sequence's region) and the keyframe is dropped whole.
// (The general branch of cloud_step_block reads the three floats at its output pointer back in lanes that hold no point: with no room left
// those belong to the next sequence's region - or to the slack at the buffer's end - may be in the middle of being written, and are discarded.)
__global__ __launch_bounds__(BLOCK_F) void keyframe_cloud_kernel(KfLog L, OdoParams OP, const SeqState* states, const uint32_t* slots_all, const double* trig) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[FeatLdsC::total];
  const int q = OP.seq0 + (int)blockIdx.x, tid = threadIdx.x;
  const SeqState* st = states + q;
  const int nkf = st->nkf, last = st->last_slot;
  const bool fused = nkf > 0 && st->ring[nkf - 1] == last;
  const int* c = L.counts + 4 * (size_t)q;
  int* cw = L.cloud_word + 4 * (size_t)q;
  const int rec = c[0], dropped = c[1], used = c[3];
  if (!fused || dropped != 0 || rec >= L.max_kf) {  // (block-uniform) nothing to write, or a log that takes no more keyframes
    if (tid == 0) { cw[0] = 0; cw[1] = 0; cw[2] = 0; cw[3] = 0; }
    return;
  }
  const ScanDev* S = reinterpret_cast<const ScanDev*>(OP.scans_base + OP.scan_stride * ((size_t)q * (OP.submap + 1) + last));
  const int room = max(L.max_points - used, 0);
  float* dst = L.points + 3 * ((size_t)q * L.max_points + used);
  int f0 = 0, f1 = 0, n0 = 0, n1 = 0;  // points of the two clouds: found, and written (cut at the room left)
  if (!slots_all) {
    f0 = S->n_points;
    n0 = min(f0, room);
    const float* src = S->xyi;
    for (int i = tid; i < 3 * n0; i += BLOCK_F) dst[i] = src[i];
  } else {
    const double* tm = L.tmot + 6 * (size_t)q;
    Aff2 TprevMot;
    TprevMot.l0 = tm[0]; TprevMot.l1 = tm[1]; TprevMot.l2 = tm[2]; TprevMot.l3 = tm[3]; TprevMot.t0 = tm[4]; TprevMot.t1 = tm[5];
    double mot[3]; aff_to_xyt(TprevMot, mot);
    int src = q, compensate = OP.compensate, z_min = 0, k = OP.k;  // the sequence's own row (features_step_body)
    if (const SeqRow row = seq_row(OP, q)) { src = row->source; compensate = row->compensate; z_min = row->z_min; k = row->k; }
    const uint32_t* slots = slots_all + (size_t)src * OP.A * OP.k;
    float bounds[4];
    PointRegs PR;
    n0 = cloud_step_block<false>(slots, OP.A, k, OP.k, trig, OP.fp.range_res, OP.fp.min_distance, z_min, dst, min(room, S->cap_points), compensate,
                                           mot[0], mot[1], mot[2], OP.ccw, reinterpret_cast<int*>(lds + FeatLdsC::red_i), reinterpret_cast<float*>(lds + FeatLdsC::red_f),
                                           reinterpret_cast<double*>(lds + FeatLdsC::pxy), (int)(CFEAR_CPT_CAP * 8 / (6 * sizeof(double))), bounds, PR, true,
                                           reinterpret_cast<int*>(lds + FeatLdsC::vst), (int)((FeatLdsC::pxy - FeatLdsC::vst) / sizeof(int)), &f0);
    if ((L.what & CFEAR_KF_PEAKS) && f0 <= room) {  // (block-uniform)
      __syncthreads();  // the first pass has read its tables
      n1 = cloud_step_block<true>(slots, OP.A, k, OP.k, trig, OP.fp.range_res, OP.fp.min_distance, z_min, dst + 3 * (size_t)n0, min(room - n0, S->cap_points), compensate,
                                   mot[0], mot[1], mot[2], OP.ccw, reinterpret_cast<int*>(lds + FeatLdsC::red_i), reinterpret_cast<float*>(lds + FeatLdsC::red_f),
                                   reinterpret_cast<double*>(lds + FeatLdsC::pxy), (int)(CFEAR_CPT_CAP * 8 / (6 * sizeof(double))), bounds, PR, true,
                                   reinterpret_cast<int*>(lds + FeatLdsC::vst), (int)((FeatLdsC::pxy - FeatLdsC::vst) / sizeof(int)), &f1);
    }
  }
  if (tid == 0) { cw[0] = (f0 <= room && f1 <= room - f0) ? 1 : 0; cw[1] = n0; cw[2] = n1; cw[3] = 0; }
}

__global__ __launch_bounds__(BLOCK_K) void keyframe_record_kernel(KfLog L, const unsigned char* scans_base, size_t scan_stride, int nslots, int seq0, int* flags,
                                                                  const SeqState* states, const double* cov_work /*[B][36]*/) {
  __shared__ double w[72];  // the 6x6 inverse's working matrix (its pivot rows are chosen at run time)
  __shared__ int s_dst;     // where the cells go in the sequence's cells, or -1: nothing to copy
  const int q = seq0 + (int)blockIdx.x, tid = threadIdx.x;
  const SeqState* st = states + q;
  const int nkf = st->nkf, last = st->last_slot;
  // AddToReference ran for this sweep exactly when the scan it built is the newest keyframe (register_step_body; the first sweep too)
  const bool fused = nkf > 0 && st->ring[nkf - 1] == last;
  double* tm = L.tmot + 6 * (size_t)q;
  Aff2 TprevMot;  // (thread 0's)
  if (tid == 0) {  // what this sweep was compensated with; the copy moves on to what the next one will be
    TprevMot.l0 = tm[0]; TprevMot.l1 = tm[1]; TprevMot.l2 = tm[2]; TprevMot.l3 = tm[3]; TprevMot.t0 = tm[4]; TprevMot.t1 = tm[5];
    const Aff2 T = st->Tmot;
    tm[0] = T.l0; tm[1] = T.l1; tm[2] = T.l2; tm[3] = T.l3; tm[4] = T.t0; tm[5] = T.t1;
  }
  if (!fused) return;  // (block-uniform)
  const ScanDev* S = reinterpret_cast<const ScanDev*>(scans_base + scan_stride * ((size_t)q * nslots + last));
  const int n = S->n_cells;
  if (tid == 0) {
    int* c = L.counts + 4 * (size_t)q;
    const int rec = c[0], used = c[2];
    const bool with_cells = (L.what & CFEAR_KF_CELLS) != 0;
    // a gap-free prefix: after the first keyframe that did not fit nothing more is recorded
    // (with a point log: the cloud stage in front has written this keyframe's clouds behind the sequence's points and says whether they fit)
    const int* cw = L.points ? L.cloud_word + 4 * (size_t)q : nullptr;
    const bool fits = c[1] == 0 && rec < L.max_kf && (!with_cells || n <= L.max_cells - used) && (!cw || cw[0] == 1);
    if (!fits) {
      c[1] = c[1] + 1;
      if (flags) flags[1 + q] |= 4;  // (this sequence's own word: only its workgroups write it, and they run in stream order)
      s_dst = -1;
    } else {
      cfear_keyframe_node* nd = L.nodes + (size_t)q * L.max_kf + rec;
      nd->index = rec; nd->sweep = st->frames - 1; nd->n_cells = n; nd->prev = rec - 1;
      double v[3];
      aff_to_xyt(st->Tcurrent, v);  // (as the sweep's record reads it)
      nd->pose[0] = v[0]; nd->pose[1] = v[1]; nd->pose[2] = v[2];
      double m[3];
      aff_to_xyt(TprevMot, m);
      nd->motion[0] = m[0]; nd->motion[1] = m[1]; nd->motion[2] = m[2];
      if (rec > 0) {  // AddToGraph :435-440 against the log's previous node (with submap_scan_size 1 the ring no longer has it)
        const cfear_keyframe_node* pv = nd - 1;
        const double to[3] = {pv->pose[0], pv->pose[1], pv->pose[2]};
        // (a covariance that cannot be inverted leaves inf / NaN in the information, as Eigen's inverse() does in the reference: the header says so)
        (void)cfear_kf::keyframe_constraint(v, to, cov_work + 36 * (size_t)q, nd->t_be, nd->information, w);
      } else {
        for (int i = 0; i < 3; i++) nd->t_be[i] = 0.0;
        for (int i = 0; i < 36; i++) nd->information[i] = 0.0;
      }
      L.cell_off[(size_t)q * L.max_kf + rec] = used;
      if (cw) {
        int* po = L.point_off + 3 * ((size_t)q * L.max_kf + rec);
        po[0] = c[3]; po[1] = cw[1]; po[2] = cw[2];
        c[3] = c[3] + cw[1] + cw[2];
      }
      c[0] = rec + 1;
      if (with_cells) c[2] = used + n;
      s_dst = with_cells ? used : -1;
    }
  }
  __syncthreads();
  const int dst = s_dst;
  if (dst < 0) return;
  // the cells as the registration reads them: rsrc (SoA, stride cap_cells: consecutive lanes read consecutive doubles) and rcov
  const size_t cc = (size_t)S->cap_cells;
  const double* rs = S->rsrc;
  const double* rc = S->rcov;
  cfear_keyframe_cell* out = L.cells + (size_t)q * L.max_cells + dst;
  for (int i = tid; i < n; i += BLOCK_K) {
    cfear_keyframe_cell* c = out + i;
    c->mean[0] = rs[i]; c->mean[1] = rs[cc + i]; c->normal[0] = rs[2 * cc + i]; c->normal[1] = rs[3 * cc + i];
    c->nsamples = (int)rs[4 * cc + i]; c->scale = rs[5 * cc + i];
    c->cov[0] = rc[3 * (size_t)i]; c->cov[1] = rc[3 * (size_t)i + 1]; c->cov[2] = rc[3 * (size_t)i + 2];
    c->pad_ = 0;
  }
}

// MapPointNormal from recorded cells: scan_from_cells_kernel for m scans at once, reading cfear_keyframe_cell records on the device. Every
// workgroup has working memory of its own (the job's), so the scans build side by side.
__global__ __launch_bounds__(BLOCK_F) void keyframe_scans_kernel(const KfScanJob* jobs, FeatureParams P) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[FeatLdsC::bm];  // the two reduction arrays
  const KfScanJob* J = jobs + blockIdx.x;
  ScanDev* S = J->dst;
  const ScanDev& H = J->hdr;  // (read field by field: a private copy of the header is a stack object the compiler parks in LDS)
  const int n = J->n;
  BlockScratch B;
  B.keys = nullptr; B.spts = nullptr; B.order = nullptr; B.vstart = nullptr; B.vlist = nullptr; B.rng = nullptr; B.tmpi = nullptr; B.samples = nullptr;
  B.match = nullptr; B.assoc = nullptr; B.vrank = nullptr; B.vperm = nullptr; B.p2cap = 0; B.pair_cap = 0;
  B.vcur = J->vcur; B.part = J->part; B.cap_points = J->part_doubles / 7;
  const FeatureScratch W = make_fscratch(B, lds);
  cfear_cell* const h_cells = H.cells; float* const h_mean_f = H.mean_f; double* const h_rsrc = H.rsrc; double* const h_rtar = H.rtar; double* const h_rcov = H.rcov;
  if (threadIdx.x == 0) { *S = H; S->n_points = 0; S->n_samples = 0; S->n_cells = n; S->status = n > 0 ? 0 : CFEAR_ERR_EMPTY; }
  const size_t cc = (size_t)H.cap_cells;
  for (int i = threadIdx.x; i < n; i += BLOCK_F) {
    // (field by field, through scalars: a struct temporary with array members would be kept in LDS by the compiler, 76 B per thread)
    const cfear_keyframe_cell* kp = J->src + i;
    const double mx = kp->mean[0], my = kp->mean[1], nx = kp->normal[0], ny = kp->normal[1], cxx = kp->cov[0], cxy = kp->cov[1], cyy = kp->cov[2];
    const double scale = kp->scale;
    const int nsamples = kp->nsamples;
    cfear_cell* c = h_cells + i;
    c->mean[0] = mx; c->mean[1] = my; c->cov[0] = cxx; c->cov[1] = cxy; c->cov[2] = cyy;
    c->normal[0] = nx; c->normal[1] = ny; c->orth[0] = -ny; c->orth[1] = nx;
    {  // the eigenvalues of the symmetric 2x2 covariance in closed form
      const double h = 0.5 * (cxx + cyy), e = 0.5 * (cxx - cyy), d = sqrt(e * e + cxy * cxy);
      c->lambda_min = h - d; c->lambda_max = h + d;
    }
    c->scale = scale; c->sum_intensity = 0.0; c->avg_intensity = 0.0; c->nsamples = nsamples; c->valid = 1;
    h_mean_f[2 * i] = (float)mx; h_mean_f[2 * i + 1] = (float)my;
    double* rs = h_rsrc + i;
    rs[0] = mx; rs[cc] = my; rs[2 * cc] = nx; rs[3 * cc] = ny; rs[4 * cc] = (double)nsamples; rs[5 * cc] = scale;
    double* rt = h_rtar + 8 * (size_t)i;
    rt[0] = mx; rt[1] = my; rt[2] = nx; rt[3] = ny; rt[4] = (double)nsamples; rt[5] = scale;
    double* rc = h_rcov + 3 * (size_t)i;
    rc[0] = cxx; rc[1] = cxy; rc[2] = cyy;
  }
  __syncthreads();
  cell_grid_block(S, n, P, W, false, nullptr);
  if (P.nn_tie == 2) kd_build_block(S, B);
}

// Constraints between any keyframes of a log (cfear_odometry_keyframe_edges): a workgroup per job runs register_kernel's registration -
// Register(scans = from[0 .. n_from - 1] + [to]) - on scans rebuilt from the log, the `from` keyframes fixed at their node poses, under
// the row of the job's sequence, and ends with the rule of a node's own edge (keyframe_constraint) on the result.
//   prologue  the scan pointers into RegLds::scanptr, the n_from + 1 poses into the registration's parameter array itself (as the step
//             kernel keeps them: register_block normalises in place), the job's covariance zeroed
//   epilogue  one thread: the constraint and the 400-byte record. The 6x6 Gauss-Jordan works in the LDS match array, which the
//             registration no longer reads - static LDS stays RegLds::total + the match array, as register_kernel's
// Match / assoc arrays: the job's own slice (job.pair_off, job.pair_cap pairs) of the call's two arrays.
__global__ __launch_bounds__(BLOCK_R, 3) void keyframe_edges_kernel(const KfEdgeJob* jobs, ScanDev* const* scan_tab, KfLog L, OdoParams OP, double* match_base,
                                                                    int* assoc_base, double* cov_all /*[m][36]*/, cfear_reg_summary* sums /*[m]*/,
                                                                    cfear_keyframe_edge* edges /*[m]*/) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[RegLds::total];
  const int b = blockIdx.x, tid = threadIdx.x;
  const KfEdgeJob* J = jobs + b;
  const int q = J->sequence, nf = J->n_from, n = nf + 1;
  const cfear_keyframe_node* nodes = L.nodes + (size_t)q * L.max_kf;
  ScanDev** sp = reinterpret_cast<ScanDev**>(lds + RegLds::scanptr);
  double* poses = reinterpret_cast<double*>(lds + RegLds::par);
  double* cov = cov_all + 36 * (size_t)b;
  if (tid < nf) {
    sp[tid] = scan_tab[J->from_scan[tid]];
    const cfear_keyframe_node* nd = nodes + J->from[tid];
    poses[3 * tid] = nd->pose[0]; poses[3 * tid + 1] = nd->pose[1]; poses[3 * tid + 2] = nd->pose[2];
  }
  if (tid == 64) {
    sp[nf] = scan_tab[J->to_scan];
    const double* g = J->has_guess ? J->guess : nodes[J->to].pose;
    poses[3 * nf] = g[0]; poses[3 * nf + 1] = g[1]; poses[3 * nf + 2] = g[2];
  }
  if (tid >= 128 && tid < 164) cov[tid - 128] = 0.0;  // (in/out for register_block: a registration without a usable solution leaves it)
  __syncthreads();
  RegScratch W;
  {
    const size_t c = (size_t)J->pair_cap;
    double* m = match_base + 8 * (size_t)J->pair_off;
    W.tmx = m; W.tmy = m + c; W.a0 = m + 2 * c; W.a1 = m + 3 * c; W.a2 = m + 4 * c; W.sx = m + 5 * c; W.sy = m + 6 * c; W.w = m + 7 * c;
    W.assoc = assoc_base + 3 * (size_t)J->pair_off; W.cap = J->pair_cap; W.acap = 3 * J->pair_cap;
    W.red = reinterpret_cast<double*>(lds + RegLds::red_d);
    W.red_i = reinterpret_cast<int*>(lds + RegLds::red_i);
  }
  cfear_reg_summary* sum = sums + b;
  (void)register_block<-1, false>(sp, n, poses, cov, OP.rp, W, poses, reinterpret_cast<RegShared*>(lds + RegLds::regsh), sum, nullptr, nullptr, seq_row(OP, q));
  // (register_block ends behind a barrier: what its controller wave wrote - the pose in LDS, the covariance and the summary - is this thread's to read)
  if (tid != 0) return;
  cfear_keyframe_edge* E = edges + b;
  const int ref = J->from[J->ref];
  E->sequence = q; E->to = J->to; E->from = ref; E->n_from = nf;
  const int path = sum->assoc_path, usable = sum->usable;
  E->status = path < 0 ? CFEAR_ERR_UNSUPPORTED : 0;  // (registration_dev.h: the kd descent's stack did not fit the match scratch)
  E->success = sum->success; E->usable = usable; E->outer_iterations = sum->outer_iterations;
  E->num_residuals = sum->num_residuals; E->num_residual_blocks = sum->num_residual_blocks; E->assoc_path = path; E->pad_ = 0;
  E->final_cost = sum->final_cost; E->score = sum->score;
  const double from_xyt[3] = {poses[3 * nf], poses[3 * nf + 1], poses[3 * nf + 2]};
  E->pose[0] = from_xyt[0]; E->pose[1] = from_xyt[1]; E->pose[2] = from_xyt[2];
  if (usable) {
    const cfear_keyframe_node* nd = nodes + ref;
    const double to_xyt[3] = {nd->pose[0], nd->pose[1], nd->pose[2]};
    // (a covariance that cannot be inverted leaves inf / NaN, as in the nodes)
    (void)cfear_kf::keyframe_constraint(from_xyt, to_xyt, cov, E->t_be, E->information, lds_match_base());
  } else {
    for (int i = 0; i < 3; i++) E->t_be[i] = 0.0;
    for (int i = 0; i < 36; i++) E->information[i] = 0.0;
  }
}

}  // namespace

void cfear_launch_keyframe_record(const KfLog& L, const OdoParams& P, int count, hipStream_t st, const SeqState* states, const double* cov_work) {
  hipLaunchKernelGGL(keyframe_record_kernel, dim3(count), dim3(BLOCK_K), 0, st, L, P.scans_base, P.scan_stride, P.submap + 1, P.seq0, P.flags, states, cov_work);
}

void cfear_launch_keyframe_clouds(const KfLog& L, const OdoParams& P, int count, hipStream_t st, const SeqState* states, const uint32_t* slots, const double* trig) {
  hipLaunchKernelGGL(keyframe_cloud_kernel, dim3(count), dim3(BLOCK_F), 0, st, L, P, states, slots, trig);
}

// ... and m scans from the log, a workgroup each
static void cfear_launch_keyframe_scans(const KfScanJob* d_jobs, int m, const FeatureParams& P, hipStream_t st) {
  hipLaunchKernelGGL(keyframe_scans_kernel, dim3(m), dim3(BLOCK_F), 0, st, d_jobs, P);
}

// ---- the host side: setters and reading routes over cfear_odometry::kf -----------------------------------------------------------------
// the reading calls' common start: recording on, the context stream drained; `cnt`: the sequence's four counters (sequence < 0: none)
static int odo_kf_read(cfear_ctx* ctx, cfear_odometry* o, const char* what, int sequence, int cnt[4]) {
  char msg[160];
  if (!ctx || !o) { snprintf(msg, sizeof(msg), "%s: bad argument", what); return cfear_fail(ctx, CFEAR_ERR_INVALID, msg); }
  if (!o->kf.what) { snprintf(msg, sizeof(msg), "%s: keyframe recording is off (cfear_odometry_set_keyframe_recording)", what); return cfear_fail(ctx, CFEAR_ERR_INVALID, msg); }
  if (cnt && (sequence < 0 || sequence >= o->B)) { snprintf(msg, sizeof(msg), "%s: sequence %d of %d", what, sequence, o->B); return cfear_fail(ctx, CFEAR_ERR_INVALID, msg); }
  CFEAR_TRY(odo_drain(ctx, o));
  if (cnt) CFEAR_HIP_CHECK(ctx, hipMemcpy(cnt, o->kf.view().counts + 4 * (size_t)sequence, sizeof(int) * 4, hipMemcpyDeviceToHost));
  return CFEAR_OK;
}
// ... for the point log: odo_kf_read, then the log has clouds (and, for peaks = 1, peaks clouds)
static int odo_kf_read_points(cfear_ctx* ctx, cfear_odometry* o, const char* what, int sequence, int peaks, int cnt[4]) {
  CFEAR_TRY(odo_kf_read(ctx, o, what, sequence, cnt));
  const auto refuse = [&](const char* text) {
    char msg[200];
    snprintf(msg, sizeof(msg), "%s: %s", what, text);
    return cfear_fail(ctx, CFEAR_ERR_INVALID, msg);
  };
  if (!o->kf.records_clouds()) return refuse("the log was switched on without CFEAR_KF_CLOUD (cfear_odometry_set_keyframe_clouds)");
  if (peaks != 0 && peaks != 1) return refuse("peaks must be 0 or 1");
  if (peaks && !o->kf.records_peaks()) return refuse("the log was switched on without CFEAR_KF_PEAKS");
  return CFEAR_OK;
}
// where the cells of keyframes 0 .. recorded - 1 of a sequence start in its cells, and (entry `recorded`) where they end
static int odo_kf_offsets(cfear_ctx* ctx, const KfLog& L, int sequence, const int cnt[4], std::vector<int>& off) {
  off.assign((size_t)cnt[0] + 1, 0);
  if (cnt[0] > 0) CFEAR_HIP_CHECK(ctx, hipMemcpy(off.data(), L.cell_off + (size_t)sequence * L.max_kf, sizeof(int) * (size_t)cnt[0], hipMemcpyDeviceToHost));
  off[(size_t)cnt[0]] = cnt[2];
  return CFEAR_OK;
}
// (first point, points of the filtered cloud, of the peaks cloud) of nodes first .. first + m - 1 of a sequence
static int odo_kf_point_offsets(cfear_ctx* ctx, const KfLog& L, int sequence, int first, int m, std::vector<int>& off) {
  off.assign(3 * (size_t)std::max(m, 0), 0);
  if (m > 0)
    CFEAR_HIP_CHECK(ctx, hipMemcpy(off.data(), L.point_off + 3 * ((size_t)sequence * L.max_kf + first), sizeof(int) * 3 * (size_t)m, hipMemcpyDeviceToHost));
  return CFEAR_OK;
}
// ... and from a node's three, where its filtered (peaks = 0) or peaks cloud lies in the log's points; *n: its points
static const float* odo_kf_cloud_span(const KfLog& L, int sequence, const int po[3], int peaks, int* n) {
  *n = peaks ? po[2] : po[1];
  return L.points + 3 * ((size_t)sequence * L.max_points + po[0] + (peaks ? po[1] : 0));
}
// entry i of a caller's list of keyframes of a sequence that has recorded `recorded`
static int odo_kf_index_check(cfear_ctx* ctx, const char* what, int i, int index, int sequence, int recorded) {
  if (index >= 0 && index < recorded) return CFEAR_OK;
  char msg[160];
  snprintf(msg, sizeof(msg), "%s: indices[%d] = %d, sequence %d has recorded %d keyframes", what, i, index, sequence, recorded);
  return cfear_fail(ctx, CFEAR_ERR_INVALID, msg);
}
// the one keyframe a caller reads into `capacity` records at `dst`
static int odo_kf_one_check(cfear_ctx* ctx, const char* what, int index, int sequence, int recorded, int capacity, const void* dst) {
  if (index >= 0 && index < recorded && capacity >= 0 && (capacity == 0 || dst)) return CFEAR_OK;
  char msg[160];
  snprintf(msg, sizeof(msg), "%s: keyframe %d of sequence %d (%d recorded), capacity %d", what, index, sequence, recorded, capacity);
  return cfear_fail(ctx, CFEAR_ERR_INVALID, msg);
}
// the cells of one recorded keyframe: n >= 1 cells from `first` on in its sequence's cells
struct KfSpan { int sequence, first, n; };
// m per-call scans from m spans of the log in one launch of keyframe_scans_kernel (cfear_odometry_keyframe_scans, and the distinct
// keyframes of cfear_odometry_keyframe_edges). Synchronous; on an error nothing is left allocated. blocks: their device blocks, if asked for.
static int odo_kf_build_scans(cfear_ctx* ctx, cfear_odometry* o, const KfLog& L, const KfSpan* spans, int m, cfear_scan** scans, const char* what,
                              std::vector<ScanDev*>* blocks = nullptr) {
  const bool kd = ctx->tune_nn_tie == 2;
  int nmax = 0;
  for (int i = 0; i < m; i++) nmax = std::max(nmax, spans[i].n);
  // working memory of the m workgroups (one block of the pool): the job table, the grid cursors and - parity mode - the kd build's stacks
  const size_t part_doubles = kd ? 7 * (size_t)std::max(nmax, ctx->A * ctx->par.k_strongest) : 0;
  const size_t jobs_b = align_up(sizeof(KfScanJob) * (size_t)m, 256), vcur_b = align_up(sizeof(int) * (CFEAR_GRID_CAP + 4), 256), part_b = align_up(sizeof(double) * part_doubles, 256);
  void* work = nullptr;
  size_t work_bytes = 0;
  CFEAR_TRY(cfear_pool_alloc(ctx, jobs_b + (vcur_b + part_b) * (size_t)m, &work, &work_bytes));
  unsigned char* wb = static_cast<unsigned char*>(work);
  std::vector<KfScanJob> jobs((size_t)m);
  int rc = CFEAR_OK;
  for (int i = 0; i < m && rc == CFEAR_OK; i++) {
    const int nc = spans[i].n;
    KfScanJob& J = jobs[(size_t)i];
    rc = cfear_scan_alloc(ctx, nc, nc, kd, nc, &scans[i], &J.dst, &J.hdr);
    if (rc != CFEAR_OK) break;
    J.src = L.cells + (size_t)spans[i].sequence * L.max_cells + spans[i].first;
    J.n = nc; J.part_doubles = (int)part_doubles;
    J.vcur = reinterpret_cast<int*>(wb + jobs_b + (vcur_b + part_b) * (size_t)i);
    J.part = kd ? reinterpret_cast<double*>(wb + jobs_b + (vcur_b + part_b) * (size_t)i + vcur_b) : nullptr;
  }
  hipError_t e = hipSuccess;
  if (rc == CFEAR_OK) {
    e = hipMemcpyAsync(wb, jobs.data(), sizeof(KfScanJob) * (size_t)m, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
      cfear_launch_keyframe_scans(reinterpret_cast<const KfScanJob*>(wb), m, odo_params(ctx, o).fp /* the context's feature parameters */, ctx->stream);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // the job table is read until here
    if (e != hipSuccess) rc = cfear_fail(ctx, CFEAR_ERR_HIP, what, e);
  }
  cfear_pool_free(ctx, work, work_bytes);
  if (rc != CFEAR_OK)
    for (int i = 0; i < m; i++) { cfear_scan_release(ctx, scans[i]); scans[i] = nullptr; }
  else if (blocks) {
    blocks->resize((size_t)m);
    for (int i = 0; i < m; i++) (*blocks)[(size_t)i] = jobs[(size_t)i].dst;
  }
  return rc;
}

extern "C" {

int cfear_odometry_set_keyframe_recording(cfear_ctx* ctx, cfear_odometry* o, int what, int max_keyframes, int max_cells) {
  if (!ctx || !o) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_set_keyframe_recording: bad argument");
  if (what != 0 && what != CFEAR_KF_NODES && what != (CFEAR_KF_NODES | CFEAR_KF_CELLS))
    return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_set_keyframe_recording: what must be 0, CFEAR_KF_NODES or CFEAR_KF_NODES | CFEAR_KF_CELLS");
  const bool cells = (what & CFEAR_KF_CELLS) != 0;
  if (what && (max_keyframes < 1 || (cells && max_cells < 1)))
    return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_set_keyframe_recording: max_keyframes (and with CFEAR_KF_CELLS max_cells) must be at least 1");
  if (what) CFEAR_SEQ_TRY(ctx, cfear_seq_fresh_check(odo_seq_object(ctx, o), "odometry_set_keyframe_recording", msg));
  CFEAR_TRY(odo_drain(ctx, o));  // no recorder is running: the buffers may go
  if (o->kf.what && o->d_flags) {  // a full log is the log's condition, not the object's: its status bit goes with the log
    std::vector<int> f((size_t)o->B + 1);
    CFEAR_HIP_CHECK(ctx, hipMemcpy(f.data(), o->d_flags, sizeof(int) * f.size(), hipMemcpyDeviceToHost));
    for (int q = 1; q <= o->B; q++) f[(size_t)q] &= ~4;
    CFEAR_HIP_CHECK(ctx, hipMemcpy(o->d_flags, f.data(), sizeof(int) * f.size(), hipMemcpyHostToDevice));
  }
  KeyframeLog& K = o->kf;
  K.release();
  if (!what) return CFEAR_OK;
  const size_t B = (size_t)o->B;
  const char* msg = "hipMalloc keyframe log";
  CFEAR_TRY(odo_ensure_flags(ctx, o));  // (a full log is reported in the sequence's status word)
  CFEAR_TRY(K.d_nodes.ensure(ctx, B * (size_t)max_keyframes, msg));
  CFEAR_TRY(K.d_cell_off.ensure(ctx, B * (size_t)max_keyframes, msg));
  CFEAR_TRY(K.d_counts.ensure(ctx, 4 * B, msg));
  CFEAR_TRY(K.d_tmot.ensure(ctx, 6 * B, msg));
  if (cells) CFEAR_TRY(K.d_cells.ensure(ctx, B * (size_t)max_cells, msg));
  K.max_kf = max_keyframes; K.max_cells = cells ? max_cells : 0;
  CFEAR_TRY(K.clear(ctx, o->B));
  K.what = what;
  return CFEAR_OK;
}

// the point log: cloud_nopeaks_ / cloud_peaks_ of every node (types.h:93-143; keyframe_cloud_kernel)
int cfear_odometry_set_keyframe_clouds(cfear_ctx* ctx, cfear_odometry* o, int what, int max_points) {
  if (!ctx || !o) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_set_keyframe_clouds: bad argument");
  if (what != 0 && what != CFEAR_KF_CLOUD && what != (CFEAR_KF_CLOUD | CFEAR_KF_PEAKS))
    return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_set_keyframe_clouds: what must be 0, CFEAR_KF_CLOUD or CFEAR_KF_CLOUD | CFEAR_KF_PEAKS (the peaks cloud is recorded "
                      "beside the filtered cloud, not alone)");
  KeyframeLog& K = o->kf;
  if (what && !(K.what & CFEAR_KF_NODES))
    return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_set_keyframe_clouds: the clouds belong to recorded nodes - switch node recording on first "
                      "(cfear_odometry_set_keyframe_recording with CFEAR_KF_NODES)");
  if (what && max_points < 1) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_set_keyframe_clouds: max_points must be at least 1");
  if ((what & CFEAR_KF_PEAKS) && ctx->tune_k1_peaks == 0 && o->filter != CFEAR_FILTER_CACFAR)
    return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_set_keyframe_clouds: CFEAR_KF_PEAKS needs the filter's peak flag and cfear_tune FILTER_PEAKS = 0 forbids it: set the "
                      "knob to -1 or 1, or record without CFEAR_KF_PEAKS");
  if (what) CFEAR_SEQ_TRY(ctx, cfear_seq_fresh_check(odo_seq_object(ctx, o), "odometry_set_keyframe_clouds", msg));
  CFEAR_TRY(odo_drain(ctx, o));  // no cloud stage is running: the buffers may go
  K.release_points();
  if (!what) return CFEAR_OK;
  const size_t B = (size_t)o->B;
  {  // refuse what cannot fit with the numbers (as cfear_odometry_create does)
    size_t free_b = 0, total_b = 0;
    const size_t per_seq = sizeof(float) * 3 * (size_t)max_points + sizeof(int) * (3 * (size_t)K.max_kf + 4);
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && per_seq * B > free_b) {
      char msg[384];
      snprintf(msg, sizeof(msg), "odometry_set_keyframe_clouds: %d sequences x %.2f MB (%d points of 12 bytes + the offsets of %d nodes per sequence) = %.2f GB, %.2f GB "
               "free: at most %zu points per sequence fit", o->B, per_seq / 1048576.0, max_points, K.max_kf, per_seq * (double)B / 1073741824.0,
               free_b / 1073741824.0, free_b / B / 12);
      return cfear_fail(ctx, CFEAR_ERR_NOMEM, msg);
    }
  }
  const char* msg = "hipMalloc keyframe point log";
  // (+ one point: cloud_step_block's general branch reads the first point of its output back whatever it wrote - at the log's very end too)
  CFEAR_TRY(K.d_points.ensure(ctx, 3 * (B * (size_t)max_points + 1), msg));
  CFEAR_TRY(K.d_point_off.ensure(ctx, 3 * B * (size_t)K.max_kf, msg));
  CFEAR_TRY(K.d_cloud_word.ensure(ctx, 4 * B, msg));
  K.max_points = max_points;
  CFEAR_TRY(K.clear(ctx, o->B));  // (no sweep has run: the rest of the log is empty already)
  K.what |= what;
  return CFEAR_OK;
}

int cfear_odometry_keyframe_counts(cfear_ctx* ctx, cfear_odometry* o, int32_t* recorded, int32_t* dropped) {
  CFEAR_TRY(odo_kf_read(ctx, o, "odometry_keyframe_counts", -1, nullptr));
  std::vector<int> c(4 * (size_t)o->B);
  CFEAR_HIP_CHECK(ctx, hipMemcpy(c.data(), o->kf.view().counts, sizeof(int) * c.size(), hipMemcpyDeviceToHost));
  for (int q = 0; q < o->B; q++) {
    if (recorded) recorded[q] = c[4 * (size_t)q];
    if (dropped) dropped[q] = c[4 * (size_t)q + 1];
  }
  return CFEAR_OK;
}

int cfear_odometry_keyframe_nodes(cfear_ctx* ctx, cfear_odometry* o, int sequence, int first, cfear_keyframe_node* nodes, int capacity, int* n) {
  int cnt[4];
  CFEAR_TRY(odo_kf_read(ctx, o, "odometry_keyframe_nodes", sequence, cnt));
  if (first < 0 || capacity < 0 || (capacity > 0 && !nodes)) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_keyframe_nodes: bad argument");
  if (n) *n = cnt[0];
  const KfLog L = o->kf.view();
  const int m = std::min(capacity, cnt[0] - first);
  if (m > 0)
    CFEAR_HIP_CHECK(ctx, hipMemcpy(nodes, L.nodes + (size_t)sequence * L.max_kf + first, sizeof(cfear_keyframe_node) * (size_t)m, hipMemcpyDeviceToHost));
  return CFEAR_OK;
}

int cfear_odometry_keyframe_cells(cfear_ctx* ctx, cfear_odometry* o, int sequence, int index, cfear_keyframe_cell* cells, int capacity, int* n) {
  int cnt[4];
  CFEAR_TRY(odo_kf_read(ctx, o, "odometry_keyframe_cells", sequence, cnt));
  const KfLog L = o->kf.view();
  if (!(L.what & CFEAR_KF_CELLS)) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_keyframe_cells: the log was switched on without CFEAR_KF_CELLS");
  CFEAR_TRY(odo_kf_one_check(ctx, "odometry_keyframe_cells", index, sequence, cnt[0], capacity, cells));
  std::vector<int> off;
  CFEAR_TRY(odo_kf_offsets(ctx, L, sequence, cnt, off));
  const int nc = off[(size_t)index + 1] - off[(size_t)index];
  if (n) *n = nc;
  const int m = std::min(capacity, nc);
  if (m > 0)
    CFEAR_HIP_CHECK(ctx, hipMemcpy(cells, L.cells + (size_t)sequence * L.max_cells + off[(size_t)index], sizeof(cfear_keyframe_cell) * (size_t)m, hipMemcpyDeviceToHost));
  return CFEAR_OK;
}

int cfear_odometry_keyframe_scans(cfear_ctx* ctx, cfear_odometry* o, int sequence, const int32_t* indices, int m, cfear_scan** scans) {
  int cnt[4];
  CFEAR_TRY(odo_kf_read(ctx, o, "odometry_keyframe_scans", sequence, cnt));
  const KfLog L = o->kf.view();
  if (!(L.what & CFEAR_KF_CELLS)) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_keyframe_scans: the log was switched on without CFEAR_KF_CELLS");
  if (!indices || !scans || m < 1) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_keyframe_scans: bad argument");
  for (int i = 0; i < m; i++) scans[i] = nullptr;
  std::vector<int> off;
  CFEAR_TRY(odo_kf_offsets(ctx, L, sequence, cnt, off));
  std::vector<KfSpan> spans((size_t)m);
  for (int i = 0; i < m; i++) {
    CFEAR_TRY(odo_kf_index_check(ctx, "odometry_keyframe_scans", i, indices[i], sequence, cnt[0]));
    const int nc = off[(size_t)indices[i] + 1] - off[(size_t)indices[i]];
    if (nc < 1) {
      char msg[160];
      snprintf(msg, sizeof(msg), "odometry_keyframe_scans: keyframe %d of sequence %d has no cells (reference: 'error, cloud empty' + exit)", indices[i], sequence);
      return cfear_fail(ctx, CFEAR_ERR_EMPTY, msg);
    }
    spans[(size_t)i] = {sequence, off[(size_t)indices[i]], nc};
  }
  return odo_kf_build_scans(ctx, o, L, spans.data(), m, scans, "odometry_keyframe_scans");
}

// Constraints between any keyframes of a log, registered in one batch (keyframe_edges_kernel). On the host: the checks, the distinct
// keyframes of the job list rebuilt once (odo_kf_build_scans), every job's slice of the match / assoc arrays by a prefix sum, one block of
// the pool for all of it, one launch, the results back - and everything returned to the pool.
int cfear_odometry_keyframe_edges(cfear_ctx* ctx, cfear_odometry* o, const cfear_keyframe_edge_job* jobs, int m, cfear_keyframe_edge* edges, double* cov6,
                                  cfear_reg_summary* summaries) {
  const char* what = "odometry_keyframe_edges";
  CFEAR_TRY(odo_kf_read(ctx, o, what, -1, nullptr));
  const KfLog L = o->kf.view();
  if (!(L.what & CFEAR_KF_CELLS)) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_keyframe_edges: the log was switched on without CFEAR_KF_CELLS");
  if (!jobs || !edges || m < 1) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_keyframe_edges: bad argument");
  const auto refuse = [&](int code, int job, const char* field, int value, const char* text) {
    char msg[256];
    snprintf(msg, sizeof(msg), "%s: jobs[%d].%s = %d: %s", what, job, field, value, text);
    return cfear_fail(ctx, code, msg);
  };
  // ---- the checks: nothing is launched, and no edge written, before every job has passed ----
  const int B = o->B;
  std::vector<int> counts(4 * (size_t)B);
  CFEAR_HIP_CHECK(ctx, hipMemcpy(counts.data(), L.counts, sizeof(int) * counts.size(), hipMemcpyDeviceToHost));
  std::vector<std::vector<int>> off((size_t)B);  // the cell offsets of the sequences the jobs name
  for (int j = 0; j < m; j++) {
    const cfear_keyframe_edge_job& J = jobs[j];
    if (J.sequence < 0 || J.sequence >= B) return refuse(CFEAR_ERR_INVALID, j, "sequence", J.sequence, "no such sequence");
    if (J.n_from < 1 || J.n_from > CFEAR_KF_EDGE_MAX_FROM) return refuse(CFEAR_ERR_INVALID, j, "n_from", J.n_from, "1 .. CFEAR_KF_EDGE_MAX_FROM keyframes");
    if (J.ref < 0 || J.ref >= J.n_from) return refuse(CFEAR_ERR_INVALID, j, "ref", J.ref, "a position in from[0 .. n_from - 1]");
    const int* cnt = counts.data() + 4 * (size_t)J.sequence;
    if (J.to < 0 || J.to >= cnt[0]) return refuse(CFEAR_ERR_INVALID, j, "to", J.to, "outside the keyframes its sequence has recorded");
    for (int i = 0; i < J.n_from; i++)
      if (J.from[i] < 0 || J.from[i] >= cnt[0]) {
        char field[32];
        snprintf(field, sizeof(field), "from[%d]", i);
        return refuse(CFEAR_ERR_INVALID, j, field, J.from[i], "outside the keyframes its sequence has recorded");
      }
    if ((J.flags & 1) && !(std::isfinite(J.guess_xyt[0]) && std::isfinite(J.guess_xyt[1]) && std::isfinite(J.guess_xyt[2])))
      return refuse(CFEAR_ERR_INVALID, j, "guess_xyt", 0, "the guess is not finite");
    std::vector<int>& of = off[(size_t)J.sequence];
    if (of.empty()) CFEAR_TRY(odo_kf_offsets(ctx, L, J.sequence, cnt, of));
    for (int i = 0; i <= J.n_from; i++) {
      const int k = i < J.n_from ? J.from[i] : J.to;
      if (of[(size_t)k + 1] - of[(size_t)k] < 1) {
        char field[32];
        if (i < J.n_from) snprintf(field, sizeof(field), "from[%d]", i); else snprintf(field, sizeof(field), "to");
        return refuse(CFEAR_ERR_EMPTY, j, field, k, "the keyframe has no cells (reference: 'error, cloud empty' + exit)");
      }
    }
  }
  CFEAR_TRY(odo_seq_sync(ctx, o, what));  // (cfear_set_params since the rows' table was built: the table follows, as before a step)
  // ---- the distinct keyframes of the list, each rebuilt once; every job's slice of the match / assoc arrays ----
  std::vector<std::vector<int>> slot((size_t)B);  // [sequence][keyframe] -> position in the scan table, -1: not needed
  std::vector<KfSpan> spans;
  std::vector<KfEdgeJob> dj((size_t)m);
  unsigned long long pairs_total = 0;
  for (int j = 0; j < m; j++) {
    const cfear_keyframe_edge_job& J = jobs[j];
    const std::vector<int>& of = off[(size_t)J.sequence];
    std::vector<int>& sl = slot[(size_t)J.sequence];
    if (sl.empty()) sl.assign(of.size(), -1);
    const auto scan_of = [&](int k) {
      if (sl[(size_t)k] < 0) { sl[(size_t)k] = (int)spans.size(); spans.push_back({J.sequence, of[(size_t)k], of[(size_t)k + 1] - of[(size_t)k]}); }
      return sl[(size_t)k];
    };
    KfEdgeJob& D = dj[(size_t)j];
    memset(&D, 0, sizeof(D));
    D.sequence = J.sequence; D.to = J.to; D.n_from = J.n_from; D.ref = J.ref; D.has_guess = J.flags & 1;
    for (int i = 0; i < J.n_from; i++) { D.from[i] = J.from[i]; D.from_scan[i] = scan_of(J.from[i]); }
    D.to_scan = scan_of(J.to);
    for (int i = 0; i < 3; i++) D.guess[i] = J.guess_xyt[i];
    // the job's own problem - max(n_from, 4) x cells(to) pairs, the rule of cfear_odo_capacities with the job's numbers: every pair's match
    // fits, the grouped association can always park (6 ints per (group of four, cell) <= 3 per pair), as under the per-call capacity - and
    // under a non-zero tie rule its 8192 pairs for the kd descent's stacks; a multiple of 64 pairs keeps every slice 256-byte aligned
    long long pairs = (long long)std::max(J.n_from, 4) * (of[(size_t)J.to + 1] - of[(size_t)J.to]);
    if (ctx->tune_nn_tie != 0) pairs = std::max(pairs, 8192LL);
    pairs = (pairs + 63) / 64 * 64;
    D.pair_cap = (int)pairs; D.pair_off = pairs_total;
    pairs_total += (unsigned long long)pairs;
  }
  const int u = (int)spans.size();
  std::vector<cfear_scan*> scans((size_t)u, nullptr);
  std::vector<ScanDev*> scan_blocks;
  CFEAR_TRY(odo_kf_build_scans(ctx, o, L, spans.data(), u, scans.data(), what, &scan_blocks));
  // one block of the pool: job table | scan table | match | assoc | covariances | summaries | edges
  const size_t jobs_b = align_up(sizeof(KfEdgeJob) * (size_t)m, 256), tab_b = align_up(sizeof(ScanDev*) * (size_t)u, 256);
  const size_t match_b = align_up(sizeof(double) * 8 * (size_t)pairs_total, 256), assoc_b = align_up(sizeof(int) * 3 * (size_t)pairs_total, 256);
  const size_t cov_b = align_up(sizeof(double) * 36 * (size_t)m, 256), sum_b = align_up(sizeof(cfear_reg_summary) * (size_t)m, 256);
  const size_t edge_b = align_up(sizeof(cfear_keyframe_edge) * (size_t)m, 256);
  void* work = nullptr;
  size_t work_bytes = 0;
  int rc = cfear_pool_alloc(ctx, jobs_b + tab_b + match_b + assoc_b + cov_b + sum_b + edge_b, &work, &work_bytes);
  if (rc == CFEAR_OK) {
    unsigned char* wb = static_cast<unsigned char*>(work);
    unsigned char* d_tab = wb + jobs_b;
    double* d_match = reinterpret_cast<double*>(d_tab + tab_b);
    int* d_assoc = reinterpret_cast<int*>(d_tab + tab_b + match_b);
    double* d_cov = reinterpret_cast<double*>(d_tab + tab_b + match_b + assoc_b);
    cfear_reg_summary* d_sum = reinterpret_cast<cfear_reg_summary*>(reinterpret_cast<unsigned char*>(d_cov) + cov_b);
    cfear_keyframe_edge* d_edges = reinterpret_cast<cfear_keyframe_edge*>(reinterpret_cast<unsigned char*>(d_sum) + sum_b);
    size_t scan_bytes = 0;
    for (int i = 0; i < u; i++) scan_bytes += cfear_scan_bytes(scans[(size_t)i]);
    static const bool stats = getenv("CFEAR_KF_EDGES_STATS") != nullptr;  // tools/gpu_keyframe_edges.py: what the call took from the pool
    if (stats)
      fprintf(stderr, "cfear_odometry_keyframe_edges: %d jobs, %d scans of %zu bytes, %llu pairs of match / assoc arrays in a block of %zu bytes\n", m, u, scan_bytes,
              pairs_total, work_bytes);
    std::vector<cfear_keyframe_edge> he((size_t)m);  // (the caller's array stays untouched unless the whole call succeeds)
    hipError_t e = hipMemcpyAsync(wb, dj.data(), sizeof(KfEdgeJob) * (size_t)m, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_tab, scan_blocks.data(), sizeof(ScanDev*) * (size_t)u, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(keyframe_edges_kernel, dim3(m), dim3(BLOCK_R), 0, ctx->stream, reinterpret_cast<const KfEdgeJob*>(wb), reinterpret_cast<ScanDev* const*>(d_tab), L,
                         odo_params(ctx, o), d_match, d_assoc, d_cov, d_sum, d_edges);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(he.data(), d_edges, sizeof(cfear_keyframe_edge) * (size_t)m, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && cov6) e = hipMemcpyAsync(cov6, d_cov, sizeof(double) * 36 * (size_t)m, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && summaries) e = hipMemcpyAsync(summaries, d_sum, sizeof(cfear_reg_summary) * (size_t)m, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);  // (the host tables are read, and the block is in use, until here)
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) rc = cfear_fail(ctx, CFEAR_ERR_HIP, what, e);
    else memcpy(edges, he.data(), sizeof(cfear_keyframe_edge) * (size_t)m);
    cfear_pool_free(ctx, work, work_bytes);
  }
  for (int i = 0; i < u; i++) cfear_scan_release(ctx, scans[(size_t)i]);
  return rc;
}

int cfear_odometry_keyframe_cloud_sizes(cfear_ctx* ctx, cfear_odometry* o, int sequence, int first, int32_t* n_cloud, int32_t* n_peaks, int capacity, int* n) {
  int cnt[4];
  CFEAR_TRY(odo_kf_read_points(ctx, o, "odometry_keyframe_cloud_sizes", sequence, 0, cnt));
  if (first < 0 || capacity < 0) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_keyframe_cloud_sizes: bad argument");
  if (n) *n = cnt[0];
  const int m = std::min(capacity, cnt[0] - first);
  std::vector<int> off;
  CFEAR_TRY(odo_kf_point_offsets(ctx, o->kf.view(), sequence, first, m, off));
  for (int i = 0; i < m; i++) {
    if (n_cloud) n_cloud[i] = off[3 * (size_t)i + 1];
    if (n_peaks) n_peaks[i] = off[3 * (size_t)i + 2];
  }
  return CFEAR_OK;
}

int cfear_odometry_keyframe_cloud(cfear_ctx* ctx, cfear_odometry* o, int sequence, int index, int peaks, float* xyi, int capacity, int* n) {
  int cnt[4];
  CFEAR_TRY(odo_kf_read_points(ctx, o, "odometry_keyframe_cloud", sequence, peaks, cnt));
  CFEAR_TRY(odo_kf_one_check(ctx, "odometry_keyframe_cloud", index, sequence, cnt[0], capacity, xyi));
  const KfLog L = o->kf.view();
  std::vector<int> off;
  CFEAR_TRY(odo_kf_point_offsets(ctx, L, sequence, index, 1, off));
  int np = 0;
  const float* src = odo_kf_cloud_span(L, sequence, off.data(), peaks, &np);
  if (n) *n = np;
  const int m = std::min(capacity, np);
  if (m > 0) CFEAR_HIP_CHECK(ctx, hipMemcpy(xyi, src, sizeof(float) * 3 * (size_t)m, hipMemcpyDeviceToHost));
  return CFEAR_OK;
}

int cfear_odometry_keyframe_clouds(cfear_ctx* ctx, cfear_odometry* o, int sequence, const int32_t* indices, int m, int peaks, cfear_cloud** clouds) {
  int cnt[4];
  CFEAR_TRY(odo_kf_read_points(ctx, o, "odometry_keyframe_clouds", sequence, peaks, cnt));
  if (!indices || !clouds || m < 1) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_keyframe_clouds: bad argument");
  for (int i = 0; i < m; i++) clouds[i] = nullptr;
  for (int i = 0; i < m; i++) CFEAR_TRY(odo_kf_index_check(ctx, "odometry_keyframe_clouds", i, indices[i], sequence, cnt[0]));
  const KfLog L = o->kf.view();
  std::vector<int> off;
  CFEAR_TRY(odo_kf_point_offsets(ctx, L, sequence, 0, cnt[0], off));
  std::vector<int> counts((size_t)m);  // (read by the copies until the synchronisation below)
  int rc = CFEAR_OK;
  hipError_t e = hipSuccess;
  for (int i = 0; i < m && rc == CFEAR_OK && e == hipSuccess; i++) {
    int& np = counts[(size_t)i];
    const float* src = odo_kf_cloud_span(L, sequence, off.data() + 3 * (size_t)indices[i], peaks, &np);
    rc = cfear_cloud_alloc(ctx, np, &clouds[i]);
    if (rc != CFEAR_OK) break;
    if (np > 0) e = hipMemcpyAsync(clouds[i]->d_xyi, src, sizeof(float) * 3 * (size_t)np, hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(clouds[i]->d_n, &counts[(size_t)i], sizeof(int), hipMemcpyHostToDevice, ctx->stream);
  }
  if (rc == CFEAR_OK) {
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) rc = cfear_fail(ctx, CFEAR_ERR_HIP, "odometry_keyframe_clouds", e);
  } else {
    (void)hipStreamSynchronize(ctx->stream);  // (counts is read until here)
  }
  if (rc != CFEAR_OK)
    for (int i = 0; i < m; i++) { cfear_cloud_release(ctx, clouds[i]); clouds[i] = nullptr; }
  return rc;
}

}  // extern "C"

extern "C" int cfear_keyframe_constraint(const double from_xyt[3], const double to_xyt[3], const double cov6[36], double t_be_xyt[3], double information[36]) {
  if (!from_xyt || !to_xyt || !cov6 || !t_be_xyt || !information) return CFEAR_ERR_INVALID;
  for (int i = 0; i < 3; i++)
    if (!std::isfinite(from_xyt[i]) || !std::isfinite(to_xyt[i])) return CFEAR_ERR_INVALID;
  for (int i = 0; i < 36; i++)
    if (!std::isfinite(cov6[i])) return CFEAR_ERR_INVALID;
  double w[72];
  return cfear_kf::keyframe_constraint(from_xyt, to_xyt, cov6, t_be_xyt, information, w) ? CFEAR_OK : CFEAR_ERR_INVALID;
}
