// drift_host_time -- time of kitti_drift_by_length (include/cfear_hip/kitti_metric.hpp) looped over the rows of a grid on the host: the
// comparison for tools/gpu_drift.py. Same shape: n poses of 0.9-1.1 m, B rows that leave the ground truth by a random walk.
// build: g++ -O3 -std=c++17 -pthread -I include -o tools/micro/drift_host_time tools/micro/drift_host_time.cpp
// usage: drift_host_time [n_poses rows threads]
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <thread>
#include <vector>

#include "cfear_hip/kitti_metric.hpp"

using namespace cfear_host;

static Pose34 planar(double x, double y, double th) {
  Pose34 p = {};
  p.m[0][0] = std::cos(th); p.m[0][1] = -std::sin(th); p.m[1][0] = std::sin(th); p.m[1][1] = std::cos(th); p.m[2][2] = 1.0;
  p.m[0][3] = x; p.m[1][3] = y;
  return p;
}

int main(int argc, char** argv) {
  const int n = argc > 1 ? atoi(argv[1]) : 8800, B = argc > 2 ? atoi(argv[2]) : 1536, threads = argc > 3 ? atoi(argv[3]) : 1;
  std::mt19937_64 gen(7);
  std::normal_distribution<double> N01(0.0, 1.0);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  std::vector<Pose34> gt(n);
  std::vector<double> g(3 * (size_t)n);
  double x = 0, y = 0, th = 0;
  for (int t = 0; t < n; t++) {
    th += 0.01 * N01(gen);
    const double v = 0.9 + 0.2 * U(gen);
    x += v * std::cos(th); y += v * std::sin(th);
    g[3 * t] = x; g[3 * t + 1] = y; g[3 * t + 2] = th;
    gt[t] = planar(x, y, th);
  }
  std::vector<std::vector<Pose34>> rows(B, std::vector<Pose34>(n));
  for (int q = 0; q < B; q++) {
    double w[3] = {0, 0, 0};
    for (int t = 0; t < n; t++) {
      w[0] += 0.01 * N01(gen); w[1] += 0.01 * N01(gen); w[2] += 1e-3 * N01(gen);
      rows[q][t] = planar(g[3 * t] + w[0], g[3 * t + 1] + w[1], g[3 * t + 2] + w[2]);
    }
  }
  std::vector<KittiDriftByLength> out(B);
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<std::thread> pool;
  for (int k = 0; k < threads; k++)
    pool.emplace_back([&, k] { for (int q = k; q < B; q += threads) out[q] = kitti_drift_by_length(gt, rows[q]); });
  for (auto& t : pool) t.join();
  const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  std::printf("{\"poses\": %d, \"rows\": %d, \"threads\": %d, \"segments\": %d, \"seconds\": %.6f, \"per_row_ms\": %.4f, \"row0_translation_percent\": %.6f}\n", n, B, threads,
              out[0].segments, s, 1e3 * s / B, out[0].translation_percent);
  return 0;
}
