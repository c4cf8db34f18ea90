// keyframes.hip -- the keyframe graph of the batched odometry routes (gfx950 only). OdometryKeyframeFuser::processFrame ends a fused sweep
// with scan_ = RadarScan(Tcurrent, TprevMot, cloud_peaks, cloud, Pcurrent, t) and AddToGraph(keyframes_, scan_, cov_current)
// (odometrykeyframefuser.cpp:171-176, 234-248, 428-445): a node per keyframe (RadarScan, types.h:93-143) with its oriented surface
// points and one odometry Constraint3d (types.h:155-190) to the previous keyframe. Here:
//   keyframe_record_kernel  a stage of its own behind the registration stage, one workgroup per sequence: the sequences that fused
//                           append their node - and their scan's cells - to their own log. It reads what the stages left behind
//                           (SeqState, the scan in last_slot, cov_work); no other kernel knows of it.
//   keyframe_cloud_kernel   with a point log, in front of the recorder: the filtered and the peaks cloud of the sequences that fused.
//   keyframe_scans_kernel   the batched twin of scan_from_cells_kernel: a workgroup per scan rebuilds a per-call scan from the log.
//   cfear_keyframe_constraint  the rule of AddToGraph :435-440 for the host (keyframe_constraint.h: one function for both sides).
#include "common.h"
#include "keyframe_dev.h"
#include "keyframe_constraint.h"

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

}  // namespace

void cfear_launch_keyframe_record(const KfLog& L, const OdoParams& P, int count, hipStream_t st, const SeqState* states, const double* cov_work) {
  hipLaunchKernelGGL(keyframe_record_kernel, dim3(count), dim3(BLOCK_K), 0, st, L, P.scans_base, P.scan_stride, P.submap + 1, P.seq0, P.flags, states, cov_work);
}

void cfear_launch_keyframe_clouds(const KfLog& L, const OdoParams& P, int count, hipStream_t st, const SeqState* states, const uint32_t* slots, const double* trig) {
  hipLaunchKernelGGL(keyframe_cloud_kernel, dim3(count), dim3(BLOCK_F), 0, st, L, P, states, slots, trig);
}

void cfear_launch_keyframe_scans(const KfScanJob* d_jobs, int m, const FeatureParams& P, hipStream_t st) {
  hipLaunchKernelGGL(keyframe_scans_kernel, dim3(m), dim3(BLOCK_F), 0, st, d_jobs, P);
}

extern "C" int cfear_keyframe_constraint(const double from_xyt[3], const double to_xyt[3], const double cov6[36], double t_be_xyt[3], double information[36]) {
  if (!from_xyt || !to_xyt || !cov6 || !t_be_xyt || !information) return CFEAR_ERR_INVALID;
  for (int i = 0; i < 3; i++)
    if (!std::isfinite(from_xyt[i]) || !std::isfinite(to_xyt[i])) return CFEAR_ERR_INVALID;
  for (int i = 0; i < 36; i++)
    if (!std::isfinite(cov6[i])) return CFEAR_ERR_INVALID;
  double w[72];
  return cfear_kf::keyframe_constraint(from_xyt, to_xyt, cov6, t_be_xyt, information, w) ? CFEAR_OK : CFEAR_ERR_INVALID;
}
