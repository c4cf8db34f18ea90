// surface_dev.h -- cost surfaces: n_scan_normal_reg::GetSurface (n_scan_normal.cpp:29-65). The problem is built ONCE at the given poses
// (BuildOptimizationProblem with the caller's itr_, the soft prior when asked for and the problem has more than one residual,
// :370-377) and ceres::Problem::Evaluate is called at every pixel (x, y) of a grid around the last pose, yaw fixed - the
// associations are not rebuilt per pixel (the difference from GetCost and from the cost-sampling covariance).
//
// Two stages. The build stage (one registration-shaped workgroup per problem) runs build_problem_block at the round-tripped poses
// and leaves the residual blocks, in residual-block order, as SoA in the problem's match scratch: target mean and P2L normal / P2D
// square-root information as the registration forms them, and the source mean already rotated by the fixed yaw (so every residual
// is an affine function of the pixel's x, y); SurfHdr points at them. The evaluation kernel (the hot path) gives every thread one or
// two pixels of a tile; the tile's workgroup streams the blocks through LDS in chunks and each thread sums its pixels' blocks
// serially, in residual-block order, in double, through the registration's own loss_eval - no atomics, no reductions: a pixel's
// value depends on nothing but its own coordinates and the blocks, whatever the launch shape.
// CFEAR_SURFACE_NAIVE=1 (A/B build): one workgroup per problem evaluates pixel after pixel with the registration's evaluate_partial and
// its workgroup-wide reduction.
#pragma once
#include "odometry_step_dev.h"

#ifndef CFEAR_SURFACE_NAIVE
#define CFEAR_SURFACE_NAIVE 0
#endif
#define CFEAR_SURFACE_BLOCK 128  // threads of an evaluation workgroup
#define CFEAR_SURFACE_CHUNK 256  // residual blocks per LDS chunk (8 x 256 doubles = 16 KiB)

namespace cfear_dev {
// what the build stage leaves for the evaluation of one problem
struct SurfHdr {
  const double* blk;  // SoA, stride cap: tmx tmy a0 a1 a2 rx ry w (match_ptrs() order; rx, ry = the source mean rotated by the fixed yaw)
  long long cap;
  int nblk;           // residual blocks
  int prior_on;       // the soft prior joins (mahalanobisDistanceError, n_scan_normal.h:259-290)
  int loss;           // the robust loss the problem was built under (a sequence's own on the batched route) and its limit
  double loss_limit;
  double pL[9], pguess[3], palpha, yaw;
};
}  // namespace cfear_dev

namespace {

// The build stage of one problem: BuildOptimizationProblem (n_scan_normal.cpp:344-391) at the round-tripped poses (Affine3dToVectorXYeZ,
// :35-38) with the object's itr_ (:222), through the registration's association (tie rules, weights, radius rule). prior_cov6: the
// soft prior's covariance (reg_cov.back()), null: soft_constraints false. Every thread of the workgroup calls it.
__device__ inline void surface_build_block(ScanDev* const* scans, int n, const double* poses, const RegParams& P_in, const RegScratch& W_in,
                                           double* par_lds, RegShared* sh, int itr, const double* prior_cov6, SurfHdr* hdr,
                                           SeqRow row = nullptr) {
  const int tid = threadIdx.x;
  LRegShared* ls = (LRegShared*)sh;
  if (tid == 0) {
    sh->rp = P_in; sh->rw = W_in;
    seq_reg_params(sh->rp, row);
    sh->rio.poses = nullptr; sh->rio.cov6 = nullptr; sh->rio.out = nullptr; sh->rio.par = par_lds; sh->rio.n = n;
  }
  for (int i = tid; i < n; i += CFEAR_REG_BLOCK) {  // Affine3dToVectorXYeZ (:35-38)
    const Aff2 T = aff_from_xyt(poses[3 * i], poses[3 * i + 1], poses[3 * i + 2]);
    double v[3]; aff_to_xyt(T, v);
    par_lds[3 * i] = v[0]; par_lds[3 * i + 1] = v[1]; par_lds[3 * i + 2] = v[2];
    sh->kf[i] = grid_view(scans[i]);
  }
  if (tid == 64) { sh->srs = scans[n - 1]->rsrc; sh->scc = (long long)scans[n - 1]->cap_cells; }
  __syncthreads();
  if ((tid >> 6) == 0) {
    const int L = 3 * (n - 1);
    sh->xcur[0] = par_lds[L]; sh->xcur[1] = par_lds[L + 1]; sh->xcur[2] = par_lds[L + 2];
    sh->prior_on = 0;
    ctl_publish_build(ls, true);
  }
  __syncthreads();
  const int M = build_problem_block(scans, n, ls, itr);
  __syncthreads();
  // the blocks as SoA in the match scratch in memory: the part build_problem_block kept in LDS is copied out, the source means are
  // rotated in place (thread i reads and writes block i only)
  const RegParams& P = CFEAR_GENERIC(const RegParams, sh->rp);
  const MatchPtrs g = match_ptrs(ls->rw.tmx, (size_t)ls->rw.cap);
  const int mode = ls->lds_match;
  const int lcap = match_lds_cap(P.cost);
  const MatchPtrs l = match_ptrs_lds(P.cost);
  const double c = ls->c, s = ls->s;  // cos / sin of the fixed yaw (ctl_publish_build)
  for (int i = tid; i < M; i += CFEAR_REG_BLOCK) {
    double sx, sy;
    if (mode != 0 && i < lcap) {
      g.tmx[i] = l.tmx[i]; g.tmy[i] = l.tmy[i]; g.w[i] = l.w[i];
      if (l.a0) g.a0[i] = l.a0[i];
      if (l.a1) g.a1[i] = l.a1[i];
      if (l.a2) g.a2[i] = l.a2[i];
      sx = l.sx[i]; sy = l.sy[i];
    } else {
      sx = g.sx[i]; sy = g.sy[i];
    }
    g.sx[i] = c * sx - s * sy;  // (the first terms of px, py in evaluate_partial: px = rx + x, py = ry + y)
    g.sy[i] = s * sx + c * sy;
  }
  if (tid == 0) {
    hdr->blk = ls->rw.tmx; hdr->cap = (long long)ls->rw.cap; hdr->nblk = M; hdr->yaw = ls->xcur[2];
    hdr->loss = P.loss; hdr->loss_limit = P.loss_limit;
    const int nres = M * ((P.cost == CFEAR_COST_P2L) ? 1 : 2);
    hdr->prior_on = 0;
    if (prior_cov6 && nres > 1) {  // the prior is added after the residual-count check (:370-377)
      prior_sqrt_info(prior_cov6, hdr->pL);
      const int L = 3 * (n - 1);
      hdr->pguess[0] = par_lds[L]; hdr->pguess[1] = par_lds[L + 1]; hdr->pguess[2] = par_lds[L + 2];  // Affine3dToEigVectorXYeZ(Tsrc.back()) (:41-42)
      hdr->palpha = sqrt((double)scans[n - 1]->n_cells);
      hdr->prior_on = 1;
    }
  }
}

// One problem of the evaluation: the cost (ceres::Problem::Evaluate, 1/2 sum w rho(|r|^2) + the prior) at PPT pixels per thread.
// coords: the x values (rows) then the y values (columns) the reference's accumulating loops visit, pixels each; nx, ny of them
// are visited, the other cells are NaN. Tile t of the problem covers pixels t * BLOCK * PPT .. + BLOCK * PPT - 1 (row-major).
template <int COST, int PPT>
__device__ __forceinline__ void surface_eval_tile(const SurfHdr* hdr, const double* coords, int nx, int ny, int pixels, double* out, int tile) {
  typedef __attribute__((address_space(3))) double lds_f64_t;
  __shared__ double s_blk[8 * CFEAR_SURFACE_CHUNK];
  lds_f64_t* lb = (lds_f64_t*)s_blk;
  const int tid = threadIdx.x;
  const int M = hdr->nblk;
  const long long cap = hdr->cap;
  const double* blk = hdr->blk;
  const int loss = hdr->loss;  // (what the build stage recorded: uniform over the workgroup)
  const double loss_limit = hdr->loss_limit;
  const int np = pixels * pixels;
  double px[PPT], py[PPT], cost[PPT];
  int pix[PPT];
  bool on[PPT];
#pragma unroll
  for (int k = 0; k < PPT; k++) {
    pix[k] = tile * (CFEAR_SURFACE_BLOCK * PPT) + k * CFEAR_SURFACE_BLOCK + tid;
    const int i = pix[k] / pixels, j = pix[k] - (pix[k] / pixels) * pixels;
    on[k] = pix[k] < np && i < nx && j < ny;
    px[k] = on[k] ? coords[i] : 0.0;
    py[k] = on[k] ? coords[pixels + j] : 0.0;
    cost[k] = 0.0;
  }
  // the arrays the cost reads (match_ptrs() order: 0 tmx 1 tmy 2 a0 3 a1 4 a2 5 rx 6 ry 7 w)
  constexpr unsigned used = COST == CFEAR_COST_P2D ? 0xFFu : (COST == CFEAR_COST_P2L ? 0xEFu : 0xE3u);
  for (int b0 = 0; b0 < M; b0 += CFEAR_SURFACE_CHUNK) {
    const int nb = min(CFEAR_SURFACE_CHUNK, M - b0);
    __syncthreads();  // (the previous chunk is consumed)
    for (int e = tid; e < 8 * CFEAR_SURFACE_CHUNK; e += CFEAR_SURFACE_BLOCK) {
      const int q = e / CFEAR_SURFACE_CHUNK, b = e - q * CFEAR_SURFACE_CHUNK;
      if (((used >> q) & 1u) && b < nb) lb[e] = blk[q * cap + b0 + b];
    }
    __syncthreads();
#pragma unroll 1
    for (int b = 0; b < nb; b++) {  // every lane reads the same block: LDS broadcasts
      const double tmx = lb[b], tmy = lb[CFEAR_SURFACE_CHUNK + b];
      const double rx = lb[5 * CFEAR_SURFACE_CHUNK + b], ry = lb[6 * CFEAR_SURFACE_CHUNK + b], wgt = lb[7 * CFEAR_SURFACE_CHUNK + b];
      const double a0 = (used & 4u) ? lb[2 * CFEAR_SURFACE_CHUNK + b] : 0.0;
      const double a1 = (used & 8u) ? lb[3 * CFEAR_SURFACE_CHUNK + b] : 0.0;
      const double a2 = (used & 16u) ? lb[4 * CFEAR_SURFACE_CHUNK + b] : 0.0;
#pragma unroll
      for (int k = 0; k < PPT; k++) {
        const double ppx = rx + px[k], ppy = ry + py[k];  // residuals: n_scan_normal.h:190-201 (P2L), :224-243 (P2D), :336-350 (P2P)
        double sq;
        if (COST == CFEAR_COST_P2L) {
          const double r0 = (ppx - tmx) * a0 + (ppy - tmy) * a1;
          sq = r0 * r0;
        } else if (COST == CFEAR_COST_P2D) {
          const double dx = ppx - tmx, dy = ppy - tmy;
          const double r0 = a0 * dx, r1 = a1 * dx + a2 * dy;
          sq = r0 * r0 + r1 * r1;
        } else {
          const double r0 = tmx - ppx, r1 = tmy - ppy;
          sq = r0 * r0 + r1 * r1;
        }
        const Rho rho = loss_eval(loss, loss_limit, sq);
        cost[k] += 0.5 * (rho.v * wgt);  // ScaledLoss (n_scan_normal.cpp:277)
      }
    }
  }
  const bool prior = hdr->prior_on != 0;
#pragma unroll
  for (int k = 0; k < PPT; k++) {
    if (pix[k] >= np) continue;
    double v = cost[k];
    if (prior) {  // mahalanobisDistanceError (n_scan_normal.h:259-290): r = L (alpha (guess - x)), no loss; after the pair blocks
      const double a = hdr->palpha;
      const double d0 = a * (hdr->pguess[0] - px[k]), d1 = a * (hdr->pguess[1] - py[k]), d2 = a * (hdr->pguess[2] - hdr->yaw);
      double r[3];
      for (int i = 0; i < 3; i++) r[i] = hdr->pL[3 * i] * d0 + hdr->pL[3 * i + 1] * d1 + hdr->pL[3 * i + 2] * d2;
      v += 0.5 * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    }
    out[pix[k]] = on[k] ? v : __builtin_nan("");  // cells the reference's loops never reach: NaN
  }
}

}  // namespace
