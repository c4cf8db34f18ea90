// cov_design_check: prints the sample design of the cost-sampling covariance and its least-squares fit (csrc/cov_design.h, what
// cfear_cov_by_sampling and cfear_odometry_set_cov_sampling compute on the host) for every command on the command line, one line each,
// every number as %.17g (a double read back is the double printed). m = steps^3 samples:
//   linspace start end num          -> "linspace <num values>"
//   design xy_range yaw_range steps -> "design m <3 m offsets> <10 m row entries>"  (cov_sample_design, row-major)
//   svd xy_range yaw_range steps    -> "svd threshold <10 singular values>"         (jacobi10 of the design's rows, in column order)
//   lstsq xy_range yaw_range steps b[0] .. b[m - 1] -> "lstsq <10 coefficients>"    (lstsq10_svd)
//   pinv xy_range yaw_range steps   -> "pinv m <10 m entries>"                      (pinv10_svd, row-major 10 x m)
// Needs no GPU and no library: tests/test_cov_design_cpu.py compares the lines with numpy.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../csrc/cov_design.h"

static void print(const char* name, const double* v, size_t n, int m = -1) {
  printf("%s", name);
  if (m >= 0) printf(" %d", m);
  for (size_t i = 0; i < n; i++) printf(" %.17g", v[i]);
  printf("\n");
}

int main(int argc, char** argv) {
  int i = 1;
  auto num = [&](int k) { return strtod(argv[i + k], nullptr); };
  while (i < argc) {
    const char* cmd = argv[i];
    const int left = argc - i - 1;
    if (strcmp(cmd, "linspace") == 0 && left >= 3) {
      std::vector<double> v;
      linspace(num(1), num(2), (int)num(3), v);
      print("linspace", v.data(), v.size());
      i += 4;
      continue;
    }
    const bool fit = strcmp(cmd, "lstsq") == 0;
    if (left < 3 || !(fit || strcmp(cmd, "design") == 0 || strcmp(cmd, "svd") == 0 || strcmp(cmd, "pinv") == 0)) break;
    const int steps = (int)num(3);
    if (steps < 1 || steps > 8) break;
    const int m = steps * steps * steps;
    if (fit && left < 3 + m) break;
    std::vector<double> offs, A;
    cov_sample_design(num(1), num(2), steps, offs, A);
    if (strcmp(cmd, "design") == 0) {
      offs.insert(offs.end(), A.begin(), A.end());
      print("design", offs.data(), offs.size(), m);
    } else if (strcmp(cmd, "svd") == 0) {
      std::vector<double> W;
      double V[100], out[11];
      jacobi10(m, A.data(), W, V, out + 1, out);
      print("svd", out, 11);
    } else if (fit) {
      std::vector<double> b((size_t)m);
      for (int k = 0; k < m; k++) b[(size_t)k] = num(4 + k);
      double c[10];
      lstsq10_svd(m, A.data(), b.data(), c);
      print("lstsq", c, 10);
    } else {
      std::vector<double> P((size_t)10 * m);
      pinv10_svd(m, A.data(), P.data());
      print("pinv", P.data(), P.size(), m);
    }
    i += 4 + (fit ? m : 0);
  }
  if (i < argc || argc < 2) {
    fprintf(stderr, "usage: %s [linspace start end num | design xy_range yaw_range steps | svd xy_range yaw_range steps | "
            "lstsq xy_range yaw_range steps b[0] .. b[steps^3 - 1] | pinv xy_range yaw_range steps] ...   (steps 1 .. 8)\n", argv[0]);
    return 2;
  }
  return 0;
}
