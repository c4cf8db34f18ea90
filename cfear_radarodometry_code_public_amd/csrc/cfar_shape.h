// cfar_shape.h -- launch plan of the CA-CFAR detectors (cfar.hip): host only, plain C++, no HIP.
// The one copy of the host arithmetic that shapes a detector launch: the launcher launches what these functions return,
// cfear_cfar_launch_plan (include/cfear_hip.h) reads it back, host/cfar_shape_check.cpp prints it for tests/test_cfar_shape_cpu.py.
// (The profiling overrides read from the environment stay in cfar.hip and come in here as arguments.)
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/cfear_hip.h"

constexpr int CFEAR_CFAR_BLOCK = 256;   // threads of the round-5 kernels' workgroups
constexpr int CFEAR_CFAR_SEG_CAP = 64;  // records per (row, wave) segment of the owner-layout detector

// CFARFilter::getCAScalingFactor (cfar.cpp:12-16) by host libm
static inline double cfear_cfar_scaling(int window_size, float false_alarm_rate) {
  const double N = (double)(window_size * 2);
  return N * (pow((double)false_alarm_rate, -1. / N) - 1.);
}

// owner-layout detector: the scale of the integer test. Prefix sums are kept as P << sh, a bin is worth a closer look when
// (S << sh) - I^2 * kopen <= 0. sh < 0: not usable - the round-5 kernels run.
static inline void cfear_cfar_int_scale(int window_size, double scaling, int* sh_out, int* kopen_out) {
  *sh_out = -1; *kopen_out = 0;
  const double smax = 2.0 * (double)window_size * 65025.0, kf = scaling * 0.5 / (double)window_size;
  for (int sh = 12; sh >= 0 && *sh_out < 0; sh--) {
    if (smax * (double)(1 << sh) >= 2147483648.0) continue;
    const double k = ceil((1.0 + 4e-6) * (double)(1 << sh) / kf);
    if (k >= 64.0 && k <= 33025.0) { *sh_out = sh; *kopen_out = (int)k; }  // I^2 kopen < 2^31; at least six bits of the threshold
  }
}

// ---- which instantiation of the owner-layout detector a row length takes (threads x bins per thread just above R) ----
struct CfarOwnerShape { int TB, NW; };

// reach: guard + window, or 0: the shape with the largest scratch for this row length. forced_tb: bins per thread of a forced shape (profiling), 0: none
static inline const CfarOwnerShape* cfear_cfar_owner_shape(int R, int reach, int forced_tb) {
  static const CfarOwnerShape shapes[4] = {{28, 2}, {20, 3}, {16, 4}, {32, 4}};
  // Measured at 3360 bins (profiles/r06_cfar_shapes.txt): two waves x 28 bins per thread is the fastest shape while the windows are short; with long
  // windows (the reference's sweep goes to 500 bins) the bins a row end clips are hundreds, the integer test is loose for them, and a wave of 1792
  // bins collects more than the 64 candidates one pass decides - four waves x 16 bins then.
  const CfarOwnerShape* best = nullptr;
  for (const CfarOwnerShape& s : shapes) {
    if (R >= 64 * s.NW * s.TB) continue;
    if (forced_tb ? s.TB == forced_tb : false) return &s;
    if (reach > 128 && s.NW < 4) continue;
    if (reach == 0 ? (!best || s.NW > best->NW) : (!best || s.NW * s.TB < best->NW * best->TB)) best = &s;
  }
  return best;
}
static inline size_t cfear_cfar_owner_ints_per_row(const CfarOwnerShape& s) { return (size_t)s.NW * (2 + CFEAR_CFAR_SEG_CAP) + 64 * (size_t)s.NW; }
static inline size_t cfear_cfar_owner_lds_bytes(int nrows, int NW, int RS) {
  return sizeof(uint32_t) * ((size_t)nrows * RS + 64 * NW + (size_t)NW * CFEAR_CFAR_SEG_CAP + 16);
}

// (row, column) offsets of the four window bounds for TB bins per thread: r in (-TB, TB), the combination with the fewest rows
struct CfarOwnerOffsets { int cr[4], cq[4], rmin, rmax; };
static inline CfarOwnerOffsets cfear_cfar_owner_offsets(int guard, int window, int TB) {
  CfarOwnerOffsets O = {};
  const int off[4] = {-guard - window, -guard, guard, guard + window};
  int best = 1 << 30;
  for (int m = 0; m < 16; m++) {
    int r[4], lo = 0, hi = 0;
    for (int c = 0; c < 4; c++) {
      r[c] = ((off[c] % TB) + TB) % TB;
      if (((m >> c) & 1) && r[c] > 0) r[c] -= TB;
      lo = r[c] < lo ? r[c] : lo; hi = r[c] > hi ? r[c] : hi;
    }
    if (hi - lo < best) {
      best = hi - lo; O.rmin = lo; O.rmax = hi;
      for (int c = 0; c < 4; c++) { O.cr[c] = r[c]; O.cq[c] = (off[c] - r[c]) / TB; }
    }
  }
  return O;
}

// columns of the transposed prefix array this configuration needs: one per thread that holds bins (and the one that holds bin R), and on either
// side the window's reach in threads + 1; rounded up to a multiple of 64
static inline int cfear_cfar_owner_columns(int R, int guard, int window, int TB, int* padl) {
  const int pad = (guard + window + TB - 1) / TB + 1, data = R / TB + 1;
  const int rs = (data + 2 * pad + 63) / 64 * 64;
  *padl = (rs - data) / 2;
  return rs;
}
// the instantiation's column count for `rs` needed columns (64 NW, 64 NW + 64 or 64 NW + 128; 0: none is wide enough) and the left pad that centres the data in it
static inline int cfear_cfar_owner_rs(int rs, int NW, int* padl) {
  for (int RS = 64 * NW; RS <= 64 * NW + 128; RS += 64)
    if (rs <= RS) { *padl += (RS - rs) / 2; return RS; }
  return 0;
}
// the last thread whose column the kernel's threads write (cfar_detect_owner_kernel states the same expression); when it is the workgroup's last
// thread - a row that nearly fills the workgroup - a loop fills the columns to its right
static inline int cfear_cfar_owner_last_col_thread(int R, int guard, int window, int TB, int RS, int padl) {
  const int tR = R / TB, padr = (guard + window + TB - 1) / TB + 1;
  return tR + padr < RS - 1 - padl ? tR + padr : RS - 1 - padl;
}
// persistent workgroups per compute unit: what its LDS holds, up to 32 waves. force: a smaller number (profiling), 0: none
static inline int cfear_cfar_owner_per_cu(size_t lds, int NW, int force) {
  int per_cu = (int)((160 * 1024) / (lds + 512));
  if (per_cu * NW > 32) per_cu = 32 / NW;
  if (per_cu < 1) per_cu = 1;
  if (force > 0 && force < per_cu) per_cu = force;
  return per_cu;
}
static inline size_t cfear_cfar_owner_grid(int compute_units, int per_cu, size_t rows) {
  const size_t grid = (size_t)compute_units * per_cu;
  return grid > rows ? rows : grid;
}

// true when the owner-layout detector takes this configuration (dword rows and base, a usable integer scale, an instantiation for its columns)
static inline bool cfear_cfar_owner_usable(int R, int guard, int window, int sh, bool dword_base, bool static_passable, int forced_tb, const CfarOwnerShape** shape) {
  if ((R & 3) != 0 || !dword_base || sh < 0 || !static_passable) return false;
  const CfarOwnerShape* s = cfear_cfar_owner_shape(R, guard + window, forced_tb);
  if (!s) return false;
  int padl;
  if (cfear_cfar_owner_columns(R, guard, window, s->TB, &padl) > 64 * s->NW + 128) return false;
  *shape = s;
  return true;
}
// the round-5 kernel of a configuration the owner-layout detector does not take: the lean kernel when the rows are dword-aligned, fit 256 threads
// x 16 (32) bins, and the window is not enormous (its pads live in LDS)
static inline int cfear_cfar_round5_kernel(int R, int guard, int window, bool dword_base, bool static_passable) {
  if ((R & 3) == 0 && dword_base && guard + window <= 2048 && static_passable) {
    if (R <= CFEAR_CFAR_BLOCK * 16) return CFEAR_CFAR_KERNEL_FAST16;
    if (R <= CFEAR_CFAR_BLOCK * 32) return CFEAR_CFAR_KERNEL_FAST32;
  }
  return CFEAR_CFAR_KERNEL_GENERAL;
}
static inline size_t cfear_cfar_fast_pad(int guard, int window) { return (size_t)((guard + window + 3) & ~3); }
static inline size_t cfear_cfar_fast_lds_bytes(int guard, int window, int TB) {
  const size_t pad = cfear_cfar_fast_pad(guard, window);
  return sizeof(uint32_t) * (pad + (size_t)CFEAR_CFAR_BLOCK * TB + pad + 4);  // the padded prefix array
}
static inline size_t cfear_cfar_general_lds_bytes(int R) { return sizeof(uint32_t) * (size_t)(R + 1) + (size_t)((R + 3 + 7) & ~3); }

// the whole plan of one detector launch over `rows` azimuth rows of R bins on a device of `compute_units`, for an image whose base is 4-byte aligned.
// static_passable: some intensity passes the static threshold (z_min < 255)
static inline cfear_cfar_plan cfear_cfar_plan_of(int R, int window, int guard, float false_alarm_rate, bool static_passable, int compute_units, size_t rows) {
  cfear_cfar_plan p = {};
  int sh, kopen;
  cfear_cfar_int_scale(window, cfear_cfar_scaling(window, false_alarm_rate), &sh, &kopen);
  p.sh = sh; p.kopen = kopen;
  const CfarOwnerShape* s = nullptr;
  if (!cfear_cfar_owner_usable(R, guard, window, sh, true, static_passable, 0, &s)) {
    p.kernel = cfear_cfar_round5_kernel(R, guard, window, true, static_passable);
    p.lds_bytes = (int32_t)(p.kernel == CFEAR_CFAR_KERNEL_GENERAL ? cfear_cfar_general_lds_bytes(R)
                                                                  : cfear_cfar_fast_lds_bytes(guard, window, p.kernel == CFEAR_CFAR_KERNEL_FAST16 ? 16 : 32));
    p.workgroups = (int32_t)rows;  // one workgroup per row
    return p;
  }
  p.kernel = CFEAR_CFAR_KERNEL_OWNER;
  p.TB = s->TB; p.NW = s->NW; p.full = R % s->TB == 0;
  int padl;
  const int rs = cfear_cfar_owner_columns(R, guard, window, s->TB, &padl);
  p.RS = cfear_cfar_owner_rs(rs, s->NW, &padl);
  p.padl = padl;
  const CfarOwnerOffsets O = cfear_cfar_owner_offsets(guard, window, s->TB);
  p.rmin = O.rmin; p.rmax = O.rmax;
  for (int c = 0; c < 4; c++) { p.cr[c] = O.cr[c]; p.cq[c] = O.cq[c]; }
  p.fill = cfear_cfar_owner_last_col_thread(R, guard, window, s->TB, p.RS, padl) >= 64 * s->NW - 1;
  const size_t lds = cfear_cfar_owner_lds_bytes(s->TB + O.rmax - O.rmin, s->NW, p.RS);
  p.lds_bytes = (int32_t)lds;
  p.per_cu = cfear_cfar_owner_per_cu(lds, s->NW, 0);
  p.workgroups = (int32_t)cfear_cfar_owner_grid(compute_units, p.per_cu, rows);
  return p;
}
