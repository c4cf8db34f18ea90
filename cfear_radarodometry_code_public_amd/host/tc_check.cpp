// tc_check -- drives RegisterTimeContinuous through the C++ mirror classes of cfear_host.hpp the way reference code would: radarDriver,
// MapPointNormal on three sweeps (not motion compensated), n_scan_normal_reg::RegisterTimeContinuous with the sweep velocity given on
// the command line. Prints the poses, the covariance and the summary as one JSON object (doubles to 17 significant digits);
// tests/test_tc_gpu.py runs the same problem through the Python binding and compares bit for bit.
// usage: tc_check <sweeps.u8> vx vy vtheta [ccw soft cost]     cost: the C ABI's numbers - 0 P2P, 1 P2L (default), 2 P2D
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "cfear_hip/cfear_host.hpp"

using namespace CFEAR_Radarodometry;

int main(int argc, char** argv) {
  if (argc < 5) { std::fprintf(stderr, "usage: %s <sweeps.u8> vx vy vtheta [ccw soft cost]\n", argv[0]); return 2; }
  const int A = 400, R = 3360;
  const float rr = 0.0595238f;
  const double vx = atof(argv[2]), vy = atof(argv[3]), vth = atof(argv[4]);
  const bool ccw = argc > 5 && atoi(argv[5]) != 0;
  const bool soft = argc > 6 && atoi(argv[6]) != 0;
  const int cost = argc > 7 ? atoi(argv[7]) : CFEAR_COST_P2L;
  std::ifstream in(argv[1], std::ios::binary);
  std::vector<std::vector<uint8_t>> imgs;
  for (;;) { std::vector<uint8_t> img((size_t)A * R); if (!in.read(reinterpret_cast<char*>(img.data()), (std::streamsize)img.size())) break; imgs.push_back(img); }
  if (imgs.size() < 3) { std::fprintf(stderr, "need three sweeps\n"); return 2; }
  try {
    radarDriver::Parameters rp; rp.range_res = rr; rp.z_min = 60; rp.k_strongest = 12; rp.min_distance = 2.5f;
    radarDriver driver(rp, true);
    std::vector<MapNormalPtr> scans;
    for (int t = 0; t < 3; t++) {
      PolarImage pi; pi.rows = A; pi.cols = R; pi.data = imgs[t].data(); pi.stamp = (uint64_t)t;
      CloudPtr cloud, peaks;
      driver.CallbackOffline(pi, cloud, peaks);
      scans.push_back(MapNormalPtr(new MapPointNormal(cloud, 3.0f, Vector2d(0, 0), true, false)));
    }
    n_scan_normal_reg reg(cost == CFEAR_COST_P2D ? P2D : (cost == CFEAR_COST_P2P ? P2P : P2L), Huber, 0.1, Combined_weights);
    std::vector<Affine3d> T = {cfear_from_xyt(0, 0, 0), cfear_from_xyt(1.0, 0.02, 0.02), cfear_from_xyt(2.2, 0.1, 0.05)};
    std::vector<Matrix6d> cov(3);
    for (int i = 0; i < 3; i++) { cov[i] = cfear_mat6_identity(); for (int a = 0; a < 6; a++) cov[i](a, a) = 0; cov[i](0, 0) = cov[i](1, 1) = 0.1 * 0.1; cov[i](5, 5) = 0.01 * 0.01; }
    const bool ok = reg.RegisterTimeContinuous(scans, T, cov, cfear_from_xyt(vx, vy, vth), soft, ccw);
    const RegSummary& s = reg.summary_;
    std::printf("{\"ok\": %d, \"itr\": %d, \"usable\": %d, \"num_residuals\": %d, \"num_residual_blocks\": %d, \"assoc_path\": %d, \"final_cost\": %.17g, \"score\": %.17g, \"poses\": [",
                ok ? 1 : 0, (int)reg.itr_, s.usable, s.num_residuals, s.num_residual_blocks, s.assoc_path, s.final_cost, reg.getScore());
    for (int i = 0; i < 3; i++) std::printf("%s[%.17g, %.17g, %.17g]", i ? ", " : "", cfear_tx(T[i]), cfear_ty(T[i]), cfear_yaw(T[i]));
    std::printf("], \"cov\": [");
    for (int a = 0; a < 6; a++) for (int b = 0; b < 6; b++) std::printf("%s%.17g", a + b ? ", " : "", cov.back()(a, b));
    std::printf("], \"inner_iterations\": [");
    for (int i = 0; i < s.outer_iterations - 1 && i < CFEAR_MAX_OUTER; i++) std::printf("%s%d", i ? ", " : "", s.inner_iterations[i]);
    std::printf("], \"termination\": [");
    for (int i = 0; i < s.outer_iterations - 1 && i < CFEAR_MAX_OUTER; i++) std::printf("%s%d", i ? ", " : "", s.termination[i]);
    std::printf("]}\n");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
