// cov_design.h -- the host side of the cost-sampling covariance (odometrykeyframefuser.cpp:261-380): the reference's sample design and the
// least-squares fit of the quadratic through the sampled costs. Plain C++ (no HIP header, no device, no context): percall.hip
// (cfear_cov_by_sampling) fits with lstsq10_svd, odometry_cov.hip (cfear_odometry_set_cov_sampling) uploads pinv10_svd's pseudo-inverse for
// the device fit (cov_sampling_dev.h), host/cov_design_check.cpp prints all of it and tests/test_cov_design_cpu.py compares it with numpy
// without a GPU.
#pragma once
#include <math.h>
#include <stddef.h>

#include <vector>

// Minimum-norm least squares of A c = b (A: m x 10), what Eigen's bdcSvd().solve() returns (odometrykeyframefuser.cpp:337), by a
// one-sided Jacobi (Hestenes) singular value decomposition: plane rotations from the right make the columns of W = A V
// mutually orthogonal; then the singular values are the column norms, U = W / sigma, and c = V diag(1 / sigma) U^T b over the
// singular values above the rank threshold (Eigen's SVDBase::threshold(): diagSize = min(m, n) times epsilon, times sigma_max; numpy's lstsq
// default is max(m, n) - with 27-125 samples 3-12 x higher, which would cut a weakly observed yaw direction Eigen keeps). Works on A itself - no normal
// equations - so nothing is lost to squaring the condition number (the yaw column is ~1e-5 of the others).
static void jacobi10(int m, const double* A, std::vector<double>& W, double V[100], double sig[10], double* thr_out) {
  const int n = 10;
  W.assign((size_t)m * n, 0.0);
  for (int i = 0; i < m * n; i++) W[i] = A[i];
  for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) V[i * n + j] = (i == j) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 60; sweep++) {
    bool rotated = false;
    for (int p = 0; p < n - 1; p++)
      for (int q = p + 1; q < n; q++) {
        double al = 0, be = 0, ga = 0;
        for (int i = 0; i < m; i++) { const double x = W[(size_t)i * n + p], y = W[(size_t)i * n + q]; al += x * x; be += y * y; ga += x * y; }
        if (ga == 0.0 || fabs(ga) <= 1e-15 * sqrt(al * be)) continue;
        rotated = true;
        const double zeta = (be - al) / (2.0 * ga);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
        for (int i = 0; i < m; i++) {
          const double x = W[(size_t)i * n + p], y = W[(size_t)i * n + q];
          W[(size_t)i * n + p] = cs * x - sn * y; W[(size_t)i * n + q] = sn * x + cs * y;
        }
        for (int i = 0; i < n; i++) {
          const double x = V[i * n + p], y = V[i * n + q];
          V[i * n + p] = cs * x - sn * y; V[i * n + q] = sn * x + cs * y;
        }
      }
    if (!rotated) break;
  }
  double smax = 0;
  for (int j = 0; j < n; j++) {
    double q = 0;
    for (int i = 0; i < m; i++) q += W[(size_t)i * n + j] * W[(size_t)i * n + j];
    sig[j] = sqrt(q);
    if (sig[j] > smax) smax = sig[j];
  }
  *thr_out = (double)(m < n ? m : n) * 2.220446049250313e-16 * smax;
}
static void lstsq10_svd(int m, const double* A, const double* b, double c[10]) {
  const int n = 10;
  std::vector<double> W;
  double V[100], sig[10], thr;
  jacobi10(m, A, W, V, sig, &thr);
  for (int k = 0; k < n; k++) c[k] = 0.0;
  for (int j = 0; j < n; j++) {
    if (!(sig[j] > thr)) continue;
    double q = 0;
    for (int i = 0; i < m; i++) q += W[(size_t)i * n + j] * b[i];  // sigma_j * (u_j . b)
    q /= sig[j] * sig[j];
    for (int k = 0; k < n; k++) c[k] += V[k * n + j] * q;
  }
}
// The same decomposition as the minimum-norm pseudo-inverse P (10 x m, row-major): c = P b for every b (the batched routes' sample design
// is fixed by (xy_range, yaw_range, samples_per_axis), so the device fit is a 10 x m product). Same rank threshold as lstsq10_svd.
static void pinv10_svd(int m, const double* A, double* P) {
  const int n = 10;
  std::vector<double> W;
  double V[100], sig[10], thr;
  jacobi10(m, A, W, V, sig, &thr);
  for (size_t i = 0; i < (size_t)n * m; i++) P[i] = 0.0;
  for (int j = 0; j < n; j++) {
    if (!(sig[j] > thr)) continue;
    const double s2 = sig[j] * sig[j];
    for (int k = 0; k < n; k++) {
      const double v = V[k * n + j];
      for (int i = 0; i < m; i++) P[(size_t)k * m + i] += v * (W[(size_t)i * n + j] / s2);
    }
  }
}
static void linspace(double start, double end, int num, std::vector<double>& v) {  // odometrykeyframefuser.cpp:497-524
  v.clear();
  if (num <= 0) return;
  if (num == 1) { v.push_back(start); return; }
  const double delta = (end - start) / ((double)num - 1);
  for (int i = 0; i < num - 1; i++) v.push_back(start + delta * i);
  v.push_back(end);
}
// the reference's sample design (odometrykeyframefuser.cpp:277-336): offsets [m][3] (x, y, yaw) in its loop order (:294-296) and the
// rows [m][10] of the least-squares quadratic
static void cov_sample_design(double xy_range, double yaw_range, int steps, std::vector<double>& offs, std::vector<double>& A) {
  std::vector<double> xs, ths;  // :277-290
  linspace(-xy_range * 0.5, xy_range * 0.5, steps, xs);
  linspace(-yaw_range * 0.5, yaw_range * 0.5, steps, ths);
  const size_t m = (size_t)steps * steps * steps;
  offs.assign(3 * m, 0.0); A.assign(10 * m, 0.0);
  int k = 0;
  for (int it = 0; it < steps; it++)  // the reference's loop order (:294-296)
    for (int ix = 0; ix < steps; ix++)
      for (int iy = 0; iy < steps; iy++, k++) {
        const double x = xs[ix], y = xs[iy], z = ths[it];
        offs[3 * k] = x; offs[3 * k + 1] = y; offs[3 * k + 2] = z;
        double* r = &A[10 * (size_t)k];
        r[0] = x * x; r[1] = y * y; r[2] = z * z; r[3] = x * y; r[4] = y * z; r[5] = z * x; r[6] = x; r[7] = y; r[8] = z; r[9] = 1.0;  // :325-336
      }
}
