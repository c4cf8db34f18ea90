// drift_check -- scores a batch of trajectories through cfear_drift_host (the device kernels of csrc/drift.hip) and through
// kitti_drift_by_length (kitti_metric.hpp, one row at a time on the host) and compares. The inputs have the shape of
// tests/test_drift_gpu.py: a 400-pose planar ground truth of ~3 m per pose with a slowly wandering heading, and 257 estimates that
// leave it by a random walk (0.02 m, 0.02 m, 2e-3 rad per pose). Prints the largest relative differences of the totals and of the
// per-length table; exits 1 above the tolerances derived in that test (translation 1e-10, rotation 1e-7, counts exact), 2 on an error.
// usage: drift_check [n_poses rows seed]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "cfear_hip.h"
#include "cfear_hip/kitti_metric.hpp"

using namespace cfear_host;

namespace {
struct Gauss {  // Box-Muller on mt19937_64: the same numbers on every standard library
  std::mt19937_64 gen;
  explicit Gauss(uint64_t seed) : gen(seed) {}
  double uniform() { return ((gen() >> 11) + 0.5) * (1.0 / 9007199254740992.0); }
  double normal(double sigma) { return sigma * std::sqrt(-2.0 * std::log(uniform())) * std::cos(6.283185307179586 * uniform()); }
};
Pose34 planar(double x, double y, double th) {
  Pose34 p = {};
  p.m[0][0] = std::cos(th); p.m[0][1] = -std::sin(th); p.m[1][0] = std::sin(th); p.m[1][1] = std::cos(th); p.m[2][2] = 1.0;
  p.m[0][3] = x; p.m[1][3] = y;
  return p;
}
double rel(double a, double b) { return b != 0.0 ? std::fabs(a - b) / std::fabs(b) : std::fabs(a); }
}  // namespace

int main(int argc, char** argv) {
  const int n = argc > 1 ? atoi(argv[1]) : 400, B = argc > 2 ? atoi(argv[2]) : 257;
  const uint64_t seed = argc > 3 ? strtoull(argv[3], nullptr, 10) : 1234;
  if (n < 1 || B < 1) { std::fprintf(stderr, "usage: %s [n_poses rows seed]\n", argv[0]); return 2; }
  Gauss rng(seed);
  std::vector<double> g(3 * (size_t)n), est(3 * (size_t)n * B);
  double x = 0, y = 0, th = 0;
  for (int t = 0; t < n; t++) {
    th += rng.normal(0.02);
    const double v = 3.0 * (0.8 + 0.4 * rng.uniform());
    x += v * std::cos(th); y += v * std::sin(th);
    g[3 * t] = x; g[3 * t + 1] = y; g[3 * t + 2] = th;
  }
  std::vector<double> walk(3 * (size_t)B, 0.0);
  for (int t = 0; t < n; t++)
    for (int q = 0; q < B; q++)
      for (int k = 0; k < 3; k++) {
        walk[3 * q + k] += rng.normal(k < 2 ? 0.02 : 2e-3);
        est[((size_t)t * B + q) * 3 + k] = g[3 * t + k] + walk[3 * q + k];
      }
  std::vector<Pose34> gt(n);
  for (int t = 0; t < n; t++) gt[t] = planar(g[3 * t], g[3 * t + 1], g[3 * t + 2]);

  cfear_params par;
  cfear_default_params(&par);
  cfear_ctx* ctx = nullptr;
  if (cfear_create(&ctx, 0, nullptr, &par, 400, 3360) != CFEAR_OK) { std::fprintf(stderr, "cfear_create failed (is a gfx950 GPU visible?)\n"); return 2; }
  cfear_drift_plan* plan = nullptr;
  std::vector<cfear_drift> dev(B);
  int rc = cfear_drift_plan_create(ctx, &gt[0].m[0][0], n, &plan);
  if (rc == CFEAR_OK) rc = cfear_drift_host(ctx, plan, est.data(), (size_t)B * 24, 24, n, B, dev.data());
  if (rc != CFEAR_OK) { std::fprintf(stderr, "error %d: %s\n", rc, cfear_last_error(ctx)); cfear_destroy(ctx); return 2; }

  double worst_t = 0, worst_r = 0, worst_tl = 0, worst_rl = 0;
  bool counts_equal = true;
  int segments = 0;
  std::vector<Pose34> row(n);
  for (int q = 0; q < B; q++) {
    for (int t = 0; t < n; t++) { const double* p = &est[((size_t)t * B + q) * 3]; row[t] = planar(p[0], p[1], p[2]); }
    const KittiDriftByLength h = kitti_drift_by_length(gt, row);
    const cfear_drift& d = dev[q];
    segments = h.segments;
    counts_equal = counts_equal && d.segments == h.segments && d.reserved == 0;
    worst_t = std::fmax(worst_t, rel(d.translation_percent, h.translation_percent));
    worst_r = std::fmax(worst_r, rel(d.rotation_deg_per_100m, h.rotation_deg_per_100m));
    for (int li = 0; li < kKittiLengths; li++) {
      counts_equal = counts_equal && d.segments_by_length[li] == h.segments_by_length[li];
      worst_tl = std::fmax(worst_tl, rel(d.translation_percent_by_length[li], h.translation_percent_by_length[li]));
      worst_rl = std::fmax(worst_rl, rel(d.rotation_deg_per_100m_by_length[li], h.rotation_deg_per_100m_by_length[li]));
    }
  }
  cfear_drift_plan_release(ctx, plan);
  cfear_destroy(ctx);
  std::printf("{\"poses\": %d, \"rows\": %d, \"segments\": %d, \"counts_equal\": %d, \"translation_rel\": %.3g, \"rotation_rel\": %.3g, "
              "\"translation_by_length_rel\": %.3g, \"rotation_by_length_rel\": %.3g}\n",
              n, B, segments, counts_equal ? 1 : 0, worst_t, worst_r, worst_tl, worst_rl);
  const bool ok = counts_equal && worst_t <= 1e-10 && worst_tl <= 1e-10 && worst_r <= 1e-7 && worst_rl <= 1e-7;
  return ok ? 0 : 1;
}
