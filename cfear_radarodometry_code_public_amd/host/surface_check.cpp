// surface_check -- drives GetSurface through the C++ mirror classes of cfear_host.hpp the way reference code would: radarDriver,
// MapPointNormal on three sweeps, n_scan_normal_reg::Register, GetSurface around the registered pose with the object's itr_, and
// OdometryKeyframeFuser::PrintSurface into <surface.txt>. Prints what the surface was evaluated at as one JSON object (poses to 17
// significant digits, itr_, the grid); tests/test_surface_gpu.py rebuilds the surface through the Python binding and compares the file
// token for token.   usage: surface_check <sweeps.u8> <surface.txt> [res width soft]
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "cfear_hip/cfear_host.hpp"

using namespace CFEAR_Radarodometry;

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: %s <sweeps.u8> <surface.txt> [res width soft]\n", argv[0]); return 2; }
  const int A = 400, R = 3360;
  const float rr = 0.0595238f;
  const double res = argc > 3 ? atof(argv[3]) : 0.1;
  const int width = argc > 4 ? atoi(argv[4]) : 1;
  const bool soft = argc > 5 && atoi(argv[5]) != 0;
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
    n_scan_normal_reg reg(P2L, Huber, 0.1, Combined_weights);
    std::vector<Affine3d> T = {cfear_from_xyt(0, 0, 0), cfear_from_xyt(1.0, 0.02, 0.02), cfear_from_xyt(2.2, 0.1, 0.05)};
    std::vector<Matrix6d> cov(3);
    const bool ok = reg.Register(scans, T, cov, false);
    MatrixXd surface;
    reg.GetSurface(scans, T, cov, soft, surface, res, width);
    OdometryKeyframeFuser::Parameters fp;
    OdometryKeyframeFuser fuser(fp, true);
    fuser.PrintSurface(argv[2], surface);
    std::printf("{\"ok\": %d, \"itr\": %d, \"pixels\": %ld, \"poses\": [", ok ? 1 : 0, (int)reg.itr_, surface.rows());
    for (int i = 0; i < 3; i++) std::printf("%s[%.17g, %.17g, %.17g]", i ? ", " : "", cfear_tx(T[i]), cfear_ty(T[i]), cfear_yaw(T[i]));
    std::printf("], \"cov\": [");
    for (int a = 0; a < 6; a++) for (int b = 0; b < 6; b++) std::printf("%s%.17g", a + b ? ", " : "", cov.back()(a, b));
    std::printf("]}\n");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
