// odometry_plan.h -- what a batched odometry object is sized and scheduled by, as functions of plain numbers: its capacities, the
// overlap clamp, the compute-unit masks of cfear_tune FILTER_CUS and the replay's chunk size. No HIP here: odometry_run.hip and
// pipeline.hip call these, host/odometry_plan_check.cpp prints them and tests/test_odometry_plan_cpu.py pins them without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

// ---- capacities ---------------------------------------------------------------------------------------------------------------
// points per scan: every slot of the k-strongest filter, or cfar_max_points detections of CA-CFAR (0: 32768)
inline int cfear_odo_cap_points(bool cfar, int A, int k_strongest, int cfar_max_points) {
  return cfar ? (cfar_max_points > 0 ? cfar_max_points : 32768) : A * k_strongest;
}
struct cfear_odo_caps { int cap_points, cap_cells, pair_cap; };
inline cfear_odo_caps cfear_odo_capacities(bool cfar, int A, int k_strongest, int cfar_max_points, int submap_scan_size, int tune_max_cells, int tune_nn_tie) {
  cfear_odo_caps C;
  const int s = submap_scan_size;
  C.cap_points = cfear_odo_cap_points(cfar, A, k_strongest, cfar_max_points);
  // cells per scan the blocks are sized for: cfear_tune MAX_CELLS; by default every filtered point (cannot overflow) - except for a submap of
  // more than seven keyframes, where that default would be hundreds of MB per sequence (280 MB at submap_scan_size 50, k 40) for scans of a
  // few hundred to ~1500 cells: 4096 then (launch/oxford_demo:62-71 works without a tune call; an overflow is loud, CFEAR_ERR_CAPACITY)
  C.cap_cells = tune_max_cells > 0 ? std::min(tune_max_cells, C.cap_points) : (s > 7 ? std::min(C.cap_points, 4096) : C.cap_points);
  // residual blocks of a registration <= keyframes x cells of the current scan (one match per source cell and keyframe,
  // n_scan_normal.cpp:242,258); the association parks four results per source cell in the same scratch
  C.pair_cap = std::max(s, 4) * C.cap_cells;
  if (tune_nn_tie != 0) C.pair_cap = std::max(C.pair_cap, 8192);  // room for the kd descent's per-thread stacks (associate_pair_rule, 512-thread kernels)
  return C;
}
// odometry streams of an object (cfear_tune ODOMETRY_OVERLAP): 0 .. 8, no more than sequences, none with CA-CFAR (the filter-ahead
// streams are the k-strongest filter's)
inline int cfear_odo_overlap(int tune_odo_overlap, int B, bool cfar) {
  int n = tune_odo_overlap < 0 ? 0 : (tune_odo_overlap > 8 ? 8 : tune_odo_overlap);
  if (n > B) n = B;
  return cfar ? 0 : n;
}

// ---- compute-unit masks -------------------------------------------------------------------------------------------------------
// CFEAR_TUNE_FILTER_CUS = F: the filter gets F compute units of its own, the odometry streams the others: the HBM-bound
// kernel and the latency-bound ones stop competing for a unit's registers and LDS. What the mask bits select was measured
// (tools/cu_mask_probe.py): the unit of masking on this GPU is a group of 8 consecutive bits - any bit set enables the
// whole group, 32 groups in all - so F is rounded to groups, and the groups are taken in a spread order (0, 4, 8, ...,
// then 2, 6, ..., then the odd ones) so that every quarter of the bit range contributes alike.
// ncu: compute units of the device. Both masks come back empty (no masked streams) without F or on a device of fewer than 16 units.
inline void cfear_cu_masks(int ncu, int filter_cus, std::vector<uint32_t>& mask_f, std::vector<uint32_t>& mask_o) {
  mask_f.clear(); mask_o.clear();
  if (filter_cus <= 0 || ncu < 16) return;
  const int ngroups = ncu / 8;
  const int gf = std::max(1, std::min(ngroups - 1, (filter_cus + 4) / 8));
  std::vector<int> order;
  for (int phase : {0, 2, 1, 3}) for (int g = phase; g < ngroups; g += 4) order.push_back(g);
  mask_f.assign((size_t)(ncu + 31) / 32, 0u); mask_o.assign((size_t)(ncu + 31) / 32, 0u);
  for (int r = 0; r < ngroups; r++) {
    std::vector<uint32_t>& m = r < gf ? mask_f : mask_o;
    for (int b = 0; b < 8; b++) { const int i = order[(size_t)r] * 8 + b; m[(size_t)i / 32] |= 1u << (i % 32); }
  }
  for (int i = ngroups * 8; i < ncu; i++) mask_o[(size_t)i / 32] |= 1u << (i % 32);
}

// ---- the replay's chunk -------------------------------------------------------------------------------------------------------
// Sweeps per chunk of a replay of n_sweeps: enough for the filter to run at its streaming rate (>= ~16 k azimuth rows per launch) and
// for the copy of the next chunk to hide behind the odometry kernels of this one, at most 64 sweeps and 256 MB per buffer (host route:
// of staged sweeps; device route: of filter slots - there is no staging). sweep_bytes: the input images of one sweep; slots: the
// filter's output elements per sweep (slots, or points of CA-CFAR clouds). Buffers of an earlier call (have_chunk sweeps of slots,
// have_polar_chunk of staging, which only the host route needs) may hold more sweeps per chunk: at least as good.
inline int cfear_replay_chunk(bool on_device, bool cfar, size_t sweep_bytes, size_t slots, int n_sweeps, int have_chunk, int have_polar_chunk) {
  const size_t filt_bytes = cfar ? sizeof(float) * 3 * slots : sizeof(uint32_t) * slots;  // the filter's output per sweep
  const size_t per_sweep = on_device ? filt_bytes : std::max(sweep_bytes, filt_bytes);
  int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)64, ((size_t)256 << 20) / per_sweep));
  chunk = std::min(chunk, n_sweeps);
  const int have = on_device ? have_chunk : std::min(have_chunk, have_polar_chunk);
  return std::max(chunk, std::min(have, n_sweeps));
}
