// scan_layout.h -- where the arrays of a scan block and of a scratch block lie, their device headers, the kernel parameter blocks of a
// context and the per-call scan handle. Host code only, shared by pipeline.hip (the batched object's blocks: odo_block_bytes,
// odo_upload_headers, odo_params) and percall.hip (the per-call scans and the context scratch).
#pragma once
#include "common.h"
#include "odometry_step_dev.h"

namespace {

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
