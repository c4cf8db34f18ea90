// scan_context_check -- the Scan-Context rules of csrc/scan_context_dev.h (what scan_context.hip's kernels run) with no library and no
// device: the layout table (the four axes exact, the rest against cos / sin), the bin of a point on points whose bin is known by
// construction and on the special ones (origin, -0.0, the outer edge, NaN / inf, intensities outside 0 .. 255), the ring-key distance,
// and the float32 pair distance against the float64 definition written out here (identical, rotated, constant and empty descriptors).
// Prints one line per check and "ok"; the exit code is the number of failed checks. Built plain and under -fsanitize=address,undefined
// (make scan_context_check_san): tests/test_scan_context_cpu.py runs both.
//   scan_context_check bins FILE   prints "status ring sector v" for every point of FILE instead: int32 n_rings, n_sectors, n_points, then
//                                  doubles ring_edge2[n_rings + 1], sector_dir[n_sectors][2], then floats xyi[n_points][3] (the test's
//                                  comparison of this bin rule with the numpy twin's, on the library's table)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../csrc/scan_context_dev.h"

using namespace cfear_sc;

static int failed = 0;
static void check(const char* what, double got, double bound) {
  const bool ok = got <= bound;  // (a NaN fails)
  printf("%-60s %.3e (<= %.1e) %s\n", what, got, bound, ok ? "ok" : "FAILED");
  if (!ok) failed++;
}

// the definition in float64: min over shifts of 1 - mean cosine over the columns that are nonzero in both
static double distance_f64(const std::vector<uint32_t>& a, const std::vector<uint32_t>& b, int nr, int ns, int* shift) {
  std::vector<double> na(ns), nb(ns);
  for (int j = 0; j < ns; j++) {
    double sa = 0.0, sb = 0.0;
    for (int r = 0; r < nr; r++) { sa += (double)a[j * nr + r] * a[j * nr + r]; sb += (double)b[j * nr + r] * b[j * nr + r]; }
    na[j] = sqrt(sa); nb[j] = sqrt(sb);
  }
  double best = 2.0;
  for (int s = 0; s < ns; s++) {
    double sum = 0.0;
    int n = 0;
    for (int j = 0; j < ns; j++) {
      const int jb = (j + s) % ns;
      if (!(na[j] > 0.0 && nb[jb] > 0.0)) continue;
      double dot = 0.0;
      for (int r = 0; r < nr; r++) dot += (double)a[j * nr + r] * b[jb * nr + r];
      sum += dot / (na[j] * nb[jb]);
      n++;
    }
    const double d = n ? 1.0 - sum / n : 1.0;
    if (d < best) { best = d; *shift = s; }
  }
  return best;
}

static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

static int bins_mode(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "scan_context_check: cannot open %s\n", path); return 2; }
  int32_t h[3];
  if (fread(h, sizeof(int32_t), 3, f) != 3 || h[0] < 1 || h[0] > MAX_RINGS || h[1] < 1 || h[1] > MAX_SECTORS || h[2] < 0) { fclose(f); return 2; }
  std::vector<double> edge((size_t)h[0] + 1), dir(2 * (size_t)h[1]);
  std::vector<float> xyi(3 * (size_t)h[2]);
  const bool got = fread(edge.data(), sizeof(double), edge.size(), f) == edge.size() && fread(dir.data(), sizeof(double), dir.size(), f) == dir.size() &&
                   fread(xyi.data(), sizeof(float), xyi.size(), f) == xyi.size();
  fclose(f);
  if (!got) return 2;
  for (int i = 0; i < h[2]; i++) {
    int ring = 0, sector = 0;
    unsigned v = 0;
    const int rc = bin_of_point(xyi[3 * (size_t)i], xyi[3 * (size_t)i + 1], xyi[3 * (size_t)i + 2], h[0], h[1], edge.data(), dir.data(), &ring, &sector, &v);
    printf("%d %d %d %u\n", rc, rc == BIN_OK ? ring : -1, rc == BIN_OK ? sector : -1, rc == BIN_OK ? v : 0u);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && strcmp(argv[1], "bins") == 0) return bins_mode(argv[2]);

  // ---- the layout: axes exact, the rest the library's cosine ----
  const int shapes[][2] = {{1, 1}, {20, 60}, {20, 40}, {40, 120}, {3, 7}, {20, 64}, {20, 65}};
  for (const auto& sh : shapes) {
    const int nr = sh[0], ns = sh[1];
    std::vector<double> edge((size_t)nr + 1), dir(2 * (size_t)ns);
    make_layout(nr, ns, 80.0, edge.data(), dir.data());
    double worst = 0.0, axes = 0.0;
    for (int j = 0; j < ns; j++) {
      const double t = 2.0 * SC_PI * j / ns;
      worst = fmax(worst, fmax(fabs(dir[2 * j] - cos(t)), fabs(dir[2 * j + 1] - sin(t))));
      if ((4 * j) % ns == 0) {
        const int k = 4 * j / ns;
        const double cx[4] = {1.0, 0.0, -1.0, 0.0}, sy[4] = {0.0, 1.0, 0.0, -1.0};
        axes += (dir[2 * j] == cx[k] && dir[2 * j + 1] == sy[k]) ? 0.0 : 1.0;
      }
    }
    char what[96];
    snprintf(what, sizeof(what), "layout %d x %d: table against cos / sin", nr, ns);
    check(what, worst, 1e-15);
    snprintf(what, sizeof(what), "layout %d x %d: entries on the axes not exact", nr, ns);
    check(what, axes, 0.0);
    check("  outer ring edge against max_range^2", fabs(edge[nr] - 6400.0), 0.0);

    // points in the middle of every bin: the bin is known by construction
    double wrong = 0.0;
    for (int j = 0; j < ns; j++)
      for (int r = 0; r < nr; r++) {
        const double t = 2.0 * SC_PI * (j + 0.5) / ns, rad = 80.0 * (r + 0.5) / nr;
        int ring = -1, sector = -1;
        unsigned v = 0;
        const int rc = bin_of_point((float)(rad * cos(t)), (float)(rad * sin(t)), 77.9f, nr, ns, edge.data(), dir.data(), &ring, &sector, &v);
        wrong += (rc == BIN_OK && ring == r && sector == j && v == 77u) ? 0.0 : 1.0;
      }
    snprintf(what, sizeof(what), "bins %d x %d: bin centres in another bin", nr, ns);
    check(what, wrong, 0.0);
    // pseudo-random points against atan2 / hypot, away from the boundaries by more than float rounding
    uint32_t seed = 12345u + (uint32_t)ns;
    double mism = 0.0;
    int tried = 0;
    for (int i = 0; i < 20000; i++) {
      const float x = ((int)(lcg(seed) % 200001) - 100000) * 1e-3f, y = ((int)(lcg(seed) % 200001) - 100000) * 1e-3f;
      const double rad = hypot((double)x, (double)y);
      double ang = atan2((double)y, (double)x);
      if (ang < 0.0) ang += 2.0 * SC_PI;
      const double fs = ang / (2.0 * SC_PI) * ns, fr = rad / 80.0 * nr;
      if (fabs(fs - round(fs)) < 1e-6 || fabs(fr - round(fr)) < 1e-6) continue;
      tried++;
      int ring = -1, sector = -1;
      unsigned v = 0;
      const int rc = bin_of_point(x, y, 1.0f, nr, ns, edge.data(), dir.data(), &ring, &sector, &v);
      if (rad >= 80.0) mism += rc == BIN_OUT_OF_RANGE ? 0.0 : 1.0;
      else mism += (rc == BIN_OK && ring == (int)floor(fr) && sector == (int)floor(fs)) ? 0.0 : 1.0;
    }
    snprintf(what, sizeof(what), "bins %d x %d: random points against atan2 / hypot", nr, ns);
    check(what, mism, 0.0);
    check("  (too few points tried)", tried > 15000 ? 0.0 : 1.0, 0.0);
  }

  // ---- the special points, 20 x 60 ----
  {
    const int nr = 20, ns = 60;
    std::vector<double> edge((size_t)nr + 1), dir(2 * (size_t)ns);
    make_layout(nr, ns, 80.0, edge.data(), dir.data());
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    struct Case { float x, y, w; int rc, ring, sector; unsigned v; const char* what; };
    const Case cases[] = {
        {0.0f, 0.0f, 5.0f, BIN_OK, 0, 0, 5u, "the origin"},
        {-0.0f, -0.0f, 5.0f, BIN_OK, 0, 0, 5u, "the origin with negative zeros"},
        {1.0f, -0.0f, 5.0f, BIN_OK, 0, 0, 5u, "+x axis with y = -0.0"},
        {-1.0f, 0.0f, 5.0f, BIN_OK, 0, 30, 5u, "-x axis"},
        {-1.0f, -0.0f, 5.0f, BIN_OK, 0, 30, 5u, "-x axis with y = -0.0"},
        {0.0f, 1.0f, 5.0f, BIN_OK, 0, 15, 5u, "+y axis"},
        {0.0f, -1.0f, 5.0f, BIN_OK, 0, 45, 5u, "-y axis"},
        {4.0f, 0.0f, 5.0f, BIN_OK, 1, 0, 5u, "on the first ring edge"},
        {80.0f, 0.0f, 5.0f, BIN_OUT_OF_RANGE, 0, 0, 0u, "exactly on max_range"},
        {79.99f, -1e-3f, 5.0f, BIN_OK, 19, 59, 5u, "the last ring, the last sector"},
        {nan, 1.0f, 5.0f, BIN_DROPPED, 0, 0, 0u, "x NaN"},
        {1.0f, inf, 5.0f, BIN_DROPPED, 0, 0, 0u, "y inf"},
        {1.0f, 1.0f, nan, BIN_DROPPED, 0, 0, 0u, "intensity NaN"},
        {1.0f, 1.0f, -inf, BIN_DROPPED, 0, 0, 0u, "intensity -inf"},
        {1.0f, 0.5f, -3.5f, BIN_OK, 0, 4, 0u, "intensity below 0"},
        {1.0f, 0.5f, 255.9f, BIN_OK, 0, 4, 255u, "intensity 255.9"},
        {1.0f, 0.5f, 1e9f, BIN_OK, 0, 4, 255u, "intensity 1e9"},
        {1.0f, 0.5f, -0.9f, BIN_OK, 0, 4, 0u, "intensity -0.9"},
        {1.0f, 0.5f, 17.99f, BIN_OK, 0, 4, 17u, "intensity 17.99"},
    };
    for (const Case& c : cases) {
      int ring = 0, sector = 0;
      unsigned v = 0;
      const int rc = bin_of_point(c.x, c.y, c.w, nr, ns, edge.data(), dir.data(), &ring, &sector, &v);
      const bool ok = rc == c.rc && (rc != BIN_OK || (ring == c.ring && sector == c.sector && v == c.v));
      char what[96];
      snprintf(what, sizeof(what), "special point: %s", c.what);
      check(what, ok ? 0.0 : 1.0, 0.0);
    }
  }

  // ---- the key distance ----
  {
    const uint32_t a[4] = {0u, 16711680u, 5u, 7u}, b[4] = {16711680u, 0u, 9u, 7u};
    const unsigned long long want = 2ull * 16711680ull * 16711680ull + 16ull;
    check("key distance of ring sums near 2^24", key_distance(a, b, 4) == want && key_distance(b, a, 4) == want ? 0.0 : 1.0, 0.0);
    check("key order: ties go to the smaller index", (key_less(3, 5, 3, 6) && !key_less(3, 6, 3, 5) && key_less(2, 9, 3, 0)) ? 0.0 : 1.0, 0.0);
  }

  // ---- the pair distance ----
  for (const auto& sh : shapes) {
    const int nr = sh[0], ns = sh[1];
    const double B = (nr + ns + 8) * ldexp(1.0, -24);
    uint32_t seed = 777u + (uint32_t)(nr * 131 + ns);
    std::vector<uint32_t> a((size_t)nr * ns), b(a.size()), rot(a.size());
    for (size_t i = 0; i < a.size(); i++) {
      a[i] = lcg(seed) % 10 < 3 ? lcg(seed) % 256 : 0u;
      b[i] = lcg(seed) % 10 < 3 ? lcg(seed) % 65536 * 255u : 0u;  // (sums up to 2^24)
    }
    std::vector<float> work(2 * (size_t)ns * (nr + 1));
    char what[96];
    int s32 = -1, s64 = -1;
    const float d32 = pair_distance_f32(a.data(), b.data(), nr, ns, work.data(), &s32);
    const double d64 = distance_f64(a, b, nr, ns, &s64);
    snprintf(what, sizeof(what), "distance %d x %d: float32 against float64, in bounds B", nr, ns);
    check(what, fabs((double)d32 - d64) / B, 1.0);
    const int m = ns > 1 ? ns - 1 : 0;  // a_j = b_(j + m): the shift is m
    for (int j = 0; j < ns; j++)
      for (int r = 0; r < nr; r++) rot[(size_t)j * nr + r] = b[(size_t)((j + m) % ns) * nr + r];
    bool any = false;
    for (uint32_t v : b) any = any || v != 0u;
    const float dr = pair_distance_f32(rot.data(), b.data(), nr, ns, work.data(), &s32);
    snprintf(what, sizeof(what), "distance %d x %d: a copy rotated by %d columns", nr, ns, m);
    check(what, any ? (s32 == m ? fabs((double)dr) / B : 1e9) : (dr == 1.0f ? 0.0 : 1e9), 1.0);
    std::vector<uint32_t> flat(a.size()), none(a.size(), 0u);
    for (int j = 0; j < ns; j++)
      for (int r = 0; r < nr; r++) flat[(size_t)j * nr + r] = (uint32_t)(r + 1);
    const float df = pair_distance_f32(flat.data(), flat.data(), nr, ns, work.data(), &s32);
    snprintf(what, sizeof(what), "distance %d x %d: all columns equal -> shift 0", nr, ns);
    check(what, s32 == 0 ? fabs((double)df) / B : 1e9, 1.0);
    const float de = pair_distance_f32(none.data(), none.data(), nr, ns, work.data(), &s32);
    snprintf(what, sizeof(what), "distance %d x %d: two empty descriptors -> 1, shift 0", nr, ns);
    check(what, (de == 1.0f && s32 == 0) ? 0.0 : 1.0, 0.0);
  }
  check("yaw of a shift lies in (-pi, pi]", (fabs(shift_yaw(30, 60) - SC_PI) < 1e-15 &&shift_yaw(31, 60) < 0.0 && shift_yaw(0, 60) == 0.0 && shift_yaw(59, 60) < 0.0) ? 0.0 : 1.0, 0.0);

  printf(failed ? "%d checks FAILED\n" : "ok\n", failed);
  return failed;
}
