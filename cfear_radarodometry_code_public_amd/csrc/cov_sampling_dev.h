// cov_sampling_dev.h -- the cost-sampling covariance of the batched routes (OdometryKeyframeFuser::approximateCovarianceBySampling,
// odometrykeyframefuser.cpp:261-380, called at :202-208 when estimate_cov_by_sampling is on): GetCost (n_scan_normal.cpp:188-213) at
// samples_per_axis^3 poses around the registered pose, a least-squares quadratic, Hessian -> covariance.
//
// One workgroup per sequence, after the sweep's registration and before the next sweep's features (pipeline.hip: a kernel of its own
// on the registration's stream; replay.hip: a stage of the persistent workgroup). Every term AddScanPairCost (:215-326) adds is local
// to one (source cell, target cell) pair, so a GetCost that builds its problem at the pose it evaluates at needs no residual-block
// storage: the fused path associates, weighs and evaluates 1/2 w rho(r^2) in one pass, threads over source cells, and reduces per
// sample in a fixed order (results repeat bit for bit). Under a non-production tie rule (NN_TIE_RULE != 0) - or in the A/B build
// CFEAR_COV_SAMPLING_NAIVE - every sample is a get_cost_block of its own through the registration's general path.
#pragma once
#include "odometry_step_dev.h"

#ifndef CFEAR_COV_SAMPLING_NAIVE
#define CFEAR_COV_SAMPLING_NAIVE 0
#endif

namespace cfear_dev {
// The fit's Hessian -> covariance (odometrykeyframefuser.cpp:340-373), shared by cfear_cov_by_sampling (host) and the sampling stage
// (device). c: the ten coefficients of the quadratic (:325-337). Returns the reference's bool; cov6 (36 doubles row-major) is written
// only on success.
__host__ __device__ inline bool cov_from_quadratic(const double c[10], double final_cost, int num_residuals, double covariance_scaler,
                                                   double* cov6) {
  const double H[9] = {2 * c[0], c[3], c[5], c[3], 2 * c[1], c[4], c[5], c[4], 2 * c[2]};  // :340-343
  // "all eigenvalues positive" (:355-358) of a symmetric matrix = positive definite = all leading principal minors positive
  // (Sylvester); the inverse by cofactors, as Eigen's Matrix3d::inverse() (:363)
  const double C00 = H[4] * H[8] - H[5] * H[7], C01 = H[5] * H[6] - H[3] * H[8], C02 = H[3] * H[7] - H[4] * H[6];
  const double det = H[0] * C00 + H[1] * C01 + H[2] * C02;
  const double minor2 = H[0] * H[4] - H[1] * H[3];
  if (!(H[0] > 0.0 && minor2 > 0.0 && det > 0.0)) return false;  // not convex: sampling not used for this scan
  if (num_residuals - 3 == 0) return false;                      // GetCovarianceScaler false (n_scan_normal.cpp:435-441)
  const double score_scale = final_cost / (double)(num_residuals - 3);
  const double id = 1.0 / det;
  const double Hi[9] = {C00 * id, (H[2] * H[7] - H[1] * H[8]) * id, (H[1] * H[5] - H[2] * H[4]) * id,
                        C01 * id, (H[0] * H[8] - H[2] * H[6]) * id, (H[2] * H[3] - H[0] * H[5]) * id,
                        C02 * id, (H[1] * H[6] - H[0] * H[7]) * id, minor2 * id};
  double C3[9];
  for (int i = 0; i < 9; i++) C3[i] = 2.0 * Hi[i] * score_scale * covariance_scaler;  // :363
  for (int i = 0; i < 36; i++) cov6[i] = (i % 7 == 0) ? 1.0 : 0.0;  // :366-373
  cov6[0] = C3[0]; cov6[1] = C3[1]; cov6[6] = C3[3]; cov6[7] = C3[4];
  cov6[35] = C3[8]; cov6[5] = C3[2]; cov6[11] = C3[5]; cov6[30] = C3[6]; cov6[31] = C3[7];
  return true;
}
}  // namespace cfear_dev

namespace {

// 1/2 sum w rho(|r|^2) of one sample and its residual count (AddScanPairCost :215-326 + ceres::Problem::Evaluate), fused: thread <->
// source cell, its keyframes four at a time through the registration's staged search (associate_cell: the searches of the four are in
// flight together, same matches as scan_closest + the gate of associate_pair). Trel / Ttar / kf / srs of `sh` hold the sample's problem
// (ctl_publish_build's transforms); the match values go through the thread's own 8-double slot of the LDS match array (write_match: the
// one statement of them).
__device__ __noinline__ void cov_sample_cost_fused(const ScanDev* const* scans, int nk, const ScanDev* src, int nsrc, const LRegShared* sh,
                                                   double curr_radius, double x0, double x1, double c, double s, double* cost_out, int* cnt_out) {
  const RegParams& P = CFEAR_GENERIC(const RegParams, sh->rp);
  const MatchPtrs mp = match_ptrs(lds_match_base(), (size_t)CFEAR_REG_BLOCK);
  const int o = threadIdx.x;
  double cost = 0.0;
  int cnt = 0;
  for (int j = threadIdx.x; j < nsrc; j += CFEAR_REG_BLOCK)
  for (int k0 = 0; k0 < nk; k0 += 4) {
    const Assoc4 a = associate_cell(src, sh, k0, min(4, nk - k0), j, curr_radius);  // (gated: -1 = no match)
    if (a.t0 < 0 && a.t1 < 0 && a.t2 < 0 && a.t3 < 0) continue;
    const RCell cs = rcell_src(src, j);
    for (int u = 0; u < 4 && k0 + u < nk; u++) {  // the pair order of a residual block (keyframe, cell) does not matter to a sum per cell
      const int i = k0 + u, ti = assoc_get(a, u);
      if (ti < 0) continue;
      const double* T = (const double*)sh->Trel[i];
      RCell ct;
      {
        const double2* r = reinterpret_cast<const double2*>(sh->kf[i].rtar + 8 * (size_t)ti);  // the LDS view: no pointer chase
        const double2 r0 = r[0], r1 = r[1], r2 = r[2];
        ct.mx = r0.x; ct.my = r0.y; ct.nx = r1.x; ct.ny = r1.y; ct.ns = r2.x; ct.scale = r2.y;
      }
      const double* ctf = (P.cost == CFEAR_COST_P2D) ? scans[i]->rcov + 3 * (size_t)ti : nullptr;
      write_match(mp, o, P, T, (const double*)sh->Ttar[i], cs, ct, ctf);
      const double sx = mp.sx[o], sy = mp.sy[o], tmx = mp.tmx[o], tmy = mp.tmy[o], wgt = mp.w[o];
      const double px = (c * sx - s * sy) + x0;
      const double py = (s * sx + c * sy) + x1;
      double sq;
      if (P.cost == CFEAR_COST_P2L) {
        const double r0 = (px - tmx) * mp.a0[o] + (py - tmy) * mp.a1[o];
        sq = r0 * r0;
      } else if (P.cost == CFEAR_COST_P2D) {
        const double dx = px - tmx, dy = py - tmy;
        const double r0 = mp.a0[o] * dx, r1 = mp.a1[o] * dx + mp.a2[o] * dy;
        sq = r0 * r0 + r1 * r1;
      } else {
        const double r0 = tmx - px, r1 = tmy - py;
        sq = r0 * r0 + r1 * r1;
      }
      const Rho rho = loss_eval(P.loss, P.loss_limit, sq);
      cost += 0.5 * (rho.v * wgt);  // ScaledLoss (n_scan_normal.cpp:277)
      cnt++;
    }
  }
  *cost_out = cost;
  *cnt_out = cnt;
}

// The sampling stage of sequence q (lds: RegLds::total bytes). Reads the context register_step_body left; cov_work[q] = cov_current
// becomes the sampled covariance on success. With cs.cov_out set, cov_current is copied there (every sweep, sampled or not).
// GENERAL: every sample through get_cost_block (cov_sample_general(): the launchers pick the instantiation; the fused one does not
// carry the general path's registers)
__device__ __forceinline__ bool cov_sample_general(const RegParams& rp) { return CFEAR_COV_SAMPLING_NAIVE || rp.nn_tie != 0; }
template <bool GENERAL>
__device__ inline void cov_sample_body(unsigned char* lds, int q, const OdoParams& OP, const BlockScratch* scratch, double* cov_work) {
  static_assert(8 * CFEAR_REG_BLOCK <= CFEAR_MATCH_LDS_DOUBLES, "the fused path keeps one match per thread in the LDS match array");
  const int tid = threadIdx.x;
  const CovSampling& CS = OP.cs;
  __shared__ double s_cost[CFEAR_REG_BLOCK / 64];
  __shared__ int s_cnt[CFEAR_REG_BLOCK / 64];
  __shared__ double s_fit[10];
  if (CS.ctx) {
    CovSampleCtx* cx = CS.ctx + q;
    const int n = cx->n;  // (block-uniform)
    if (n >= 2) {
      const int nk = n - 1, L = 3 * nk, m = CS.m, itr = cx->itr;
      const int nslots = OP.submap + 1;
      ScanDev** sp = reinterpret_cast<ScanDev**>(lds + RegLds::scanptr);
      double* par = reinterpret_cast<double*>(lds + RegLds::par);
      RegShared* sh = reinterpret_cast<RegShared*>(lds + RegLds::regsh);
      LRegShared* ls = (LRegShared*)sh;
      double* costs = CS.costs + (size_t)q * m;
      const double bx = cx->pose[L], by = cx->pose[L + 1], bt = cx->pose[L + 2];
      for (int i = tid; i < n; i += CFEAR_REG_BLOCK)
        sp[i] = reinterpret_cast<ScanDev*>(OP.scans_base + OP.scan_stride * ((size_t)q * nslots + cx->slot[i]));
      double last = 0.0;  // a failed GetCost leaves sample_cost at its previous value (:305: the return value is ignored), per call from 0
      if (GENERAL) {
        const RegScratch RW = make_rscratch(scratch[q], lds);
        for (int k = 0; k < m; k++) {
          __syncthreads();  // (the previous sample's problem is consumed)
          for (int i = tid; i < 3 * n; i += CFEAR_REG_BLOCK)
            par[i] = i < L ? cx->pose[i] : CS.offs[3 * k + (i - L)] + (i == L ? bx : (i == L + 1 ? by : bt));
          __syncthreads();
          // (the sample's poses are converted in place where get_cost_block keeps its parameter vectors: thread i reads and writes pose i)
          get_cost_block(sp, n, par, OP.rp, RW, par, sh, itr, &s_cost[0], nullptr, 0, &s_cnt[0], seq_row(OP, q));
          __syncthreads();
          if (tid == 0) { if (s_cnt[0] >= 0) last = s_cost[0]; costs[k] = last; }
        }
      } else {
        // the keyframes' side of the problem once: poses as get_cost_block converts them (Affine3dToVectorXYeZ of vectorToAffine3d,
        // :196), their affine maps (ctl_publish_build) and 1-NN views
        if (tid == 0) { sh->rp = OP.rp; seq_reg_params(sh->rp, seq_row(OP, q)); sh->srs = sp[nk]->rsrc; sh->scc = (long long)sp[nk]->cap_cells; }
        for (int i = tid; i < nk; i += CFEAR_REG_BLOCK) {
          Aff2 T = aff_from_xyt(cx->pose[3 * i], cx->pose[3 * i + 1], cx->pose[3 * i + 2]);
          double v[3]; aff_to_xyt(T, v);
          T = aff_from_xyt(v[0], v[1], v[2]);
          auto* a = sh->Ttar[i];
          a[0] = T.l0; a[1] = T.l1; a[2] = T.l2; a[3] = T.l3; a[4] = T.t0; a[5] = T.t1;
          sh->kf[i] = grid_view(sp[i]);
        }
        const double curr_radius = (itr == 1) ? 2 * OP.rp.assoc_radius : OP.rp.assoc_radius;  // :222
        for (int k = 0; k < m; k++) {
          double xc[3];
          {
            const Aff2 T = aff_from_xyt(CS.offs[3 * k] + bx, CS.offs[3 * k + 1] + by, CS.offs[3 * k + 2] + bt);
            aff_to_xyt(T, xc);
          }
          const Aff2 Tsrc = aff_from_xyt(xc[0], xc[1], xc[2]);
          __syncthreads();  // (the previous sample's transforms are consumed; the keyframes' are written)
          for (int i = tid; i < nk; i += CFEAR_REG_BLOCK) {
            Aff2 Tt;
            const auto* a = sh->Ttar[i];
            Tt.l0 = a[0]; Tt.l1 = a[1]; Tt.l2 = a[2]; Tt.l3 = a[3]; Tt.t0 = a[4]; Tt.t1 = a[5];
            const Aff2 Tr = aff_mul(aff_inv(Tt), Tsrc);  // Tsrctotar (:224)
            auto* b = sh->Trel[i];
            b[0] = Tr.l0; b[1] = Tr.l1; b[2] = Tr.l2; b[3] = Tr.l3; b[4] = Tr.t0; b[5] = Tr.t1;
          }
          __syncthreads();
          double sn, cs;
          sincos(xc[2], &sn, &cs);
          double cost; int cnt;
          cov_sample_cost_fused(sp, nk, sp[nk], sp[nk]->n_cells, ls, curr_radius, xc[0], xc[1], cs, sn, &cost, &cnt);
          cost = wave_sum(cost);
          cnt = wave_sum(cnt);
          if (lane_id() == 0) { s_cost[tid >> 6] = cost; s_cnt[tid >> 6] = cnt; }
          __syncthreads();
          if (tid == 0) {  // waves in order: a fixed summation order
            double tot = 0.0; int M = 0;
            for (int w = 0; w < CFEAR_REG_BLOCK / 64; w++) { tot += s_cost[w]; M += s_cnt[w]; }
            const int nres = M * ((sh->rp.cost == CFEAR_COST_P2L) ? 1 : 2);  // (the sequence's cost: seq_reg_params above)
            if (nres > 1) last = tot;  // GetCost false for <= 1 residuals (:205-208)
            costs[k] = last;
          }
        }
      }
      __syncthreads();
      // the fit: c = A^+ b (a 10 x m product with the design's pseudo-inverse, cfear_odometry_set_cov_sampling), one coefficient per
      // thread in a fixed order; the costs were written by thread 0
      if (tid < 10) {
        double acc = 0.0;
        for (int k = 0; k < m; k++) acc += CS.pinv[(size_t)tid * m + k] * costs[k];
        s_fit[tid] = acc;
      }
      __syncthreads();
      if (tid == 0) {
        double c10[10], cov[36];
        for (int i = 0; i < 10; i++) c10[i] = s_fit[i];
        const bool ok = cov_from_quadratic(c10, cx->final_cost, cx->num_residuals, CS.scaler, cov);
        if (ok) for (int i = 0; i < 36; i++) cov_work[(size_t)q * 36 + i] = cov[i];  // cov_current = cov_sampled (:205-206)
        cx->sampled = ok ? 1 : 0;
      }
    } else if (tid == 0) {
      cx->sampled = 0;
    }
  }
  if (CS.cov_out) {
    __syncthreads();
    if (tid < 36) CS.cov_out[(size_t)q * 36 + tid] = cov_work[(size_t)q * 36 + tid];
  }
}

}  // namespace
