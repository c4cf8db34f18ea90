// keyframe_constraint.h -- the odometry constraint between two consecutive keyframes, OdometryKeyframeFuser::AddToGraph
// (odometrykeyframefuser.cpp:428-445, the lines :435-440) as written, once for the host entry (cfear_keyframe_constraint) and for the
// recorder kernel (keyframes.hip). Nothing here needs a device header: plain C++ with <math.h>.
#pragma once
#include <math.h>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

namespace cfear_kf {

// a general 6x6 inverse in double (Eigen's inverse() at this size is a partial-pivot LU): Gauss-Jordan with row pivoting on [A | I] in
// the caller's 72 doubles (the recorder hands over LDS: the pivot row is found at run time, and registers cannot be indexed by it).
// false: a pivot that is zero or not finite - the quotients then hold what the divisions gave (inf / NaN, as Eigen would leave them).
__host__ __device__ inline bool inverse6(const double* A, double* inv, double* w /*[72]*/) {
  for (int r = 0; r < 6; r++)
    for (int c = 0; c < 12; c++) w[12 * r + c] = c < 6 ? A[6 * r + c] : (c - 6 == r ? 1.0 : 0.0);
  bool ok = true;
  for (int k = 0; k < 6; k++) {
    int p = k;
    double best = fabs(w[12 * k + k]);
    for (int r = k + 1; r < 6; r++) {
      const double v = fabs(w[12 * r + k]);
      if (v > best) { best = v; p = r; }
    }
    if (!(best > 0.0) || !isfinite(best)) ok = false;
    if (p != k)
      for (int c = 0; c < 12; c++) { const double t = w[12 * k + c]; w[12 * k + c] = w[12 * p + c]; w[12 * p + c] = t; }
    const double d = w[12 * k + k];
    for (int c = 0; c < 12; c++) w[12 * k + c] = w[12 * k + c] / d;
    for (int r = 0; r < 6; r++) {
      if (r == k) continue;
      const double f = w[12 * r + k];
      if (f == 0.0) continue;
      for (int c = 0; c < 12; c++) w[12 * r + c] = w[12 * r + c] - f * w[12 * k + c];
    }
  }
  for (int r = 0; r < 6; r++)
    for (int c = 0; c < 6; c++) inv[6 * r + c] = w[12 * r + 6 + c];
  return ok;
}

// AddToGraph :435-440. from: the NEW keyframe's pose (x, y, theta), to: the previous keyframe's; cov6: cov_current of the sweep that
// fused, row-major over (x, y, z, roll, pitch, yaw).
//   t_be        = Tfrom^-1 * Tto as (x, y, theta)                                                     (:436)
//   C           = Cov with C.block<3,3>(0,0) = R C.block<3,3>(0,0) R^T, R the rotation of Tfrom^-1    (:437-439)
//   information = C^-1                                                                                (:440)
// Only the leading 3x3 block turns: the (0,5) / (5,0) cross terms GetCovariance (n_scan_normal.cpp:426-430) leaves between x and yaw
// stay where they are. That is the reference's behaviour and is restated, not repaired.
__host__ __device__ inline bool keyframe_constraint(const double from[3], const double to[3], const double cov6[36], double t_be[3],
                                                    double information[36], double* w /*[72]*/) {
  const double cf = cos(from[2]), sf = sin(from[2]), ct = cos(to[2]), st = sin(to[2]);
  // Tfrom^-1 = [R(-theta_f) | -R(-theta_f) t_f]
  const double dx = to[0] - from[0], dy = to[1] - from[1];
  t_be[0] = cf * dx + sf * dy;
  t_be[1] = -sf * dx + cf * dy;
  t_be[2] = atan2(cf * st - sf * ct, cf * ct + sf * st);  // the rotation of the product, as Affine3dToVectorXYeZ reads it (utils.cpp:115-122)
  const double R[9] = {cf, sf, 0.0, -sf, cf, 0.0, 0.0, 0.0, 1.0};
  double* C = information;  // (built in place: inverse6 has read all of it before it writes the inverse)
  for (int i = 0; i < 36; i++) C[i] = cov6[i];
  double RC[9];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) RC[3 * r + c] = R[3 * r] * cov6[c] + R[3 * r + 1] * cov6[6 + c] + R[3 * r + 2] * cov6[12 + c];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) C[6 * r + c] = RC[3 * r] * R[3 * c] + RC[3 * r + 1] * R[3 * c + 1] + RC[3 * r + 2] * R[3 * c + 2];
  return inverse6(C, information, w);
}

}  // namespace cfear_kf
