// pose_graph_check -- the pose-graph edge functions of csrc/pose_graph_dev.h (what pose_graph.hip's kernel and cfear_pose_graph_cost_host
// run) on a fixed small graph, with no library and no device: the cost against a sum written out here, the analytic Jacobians against
// central differences, the gradient and the diagonal blocks the kernel assembles from a linearised edge against the Jacobians, the 3x3
// inverse, the loss, and the refusals. Prints one line per check and "ok"; the exit code is the number of failed checks. Built plain and
// under -fsanitize=address,undefined (make pose_graph_check_san): tests/test_pose_graph_cpu.py runs both.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../csrc/pose_graph_dev.h"

using namespace cfear_pg;

static int failed = 0;
static void check(const char* what, double got, double bound) {
  const bool ok = got <= bound;  // (a NaN fails)
  printf("%-52s %.3e (<= %.1e) %s\n", what, got, bound, ok ? "ok" : "FAILED");
  if (!ok) failed++;
}

static cfear_pg_edge edge(int a, int b, int flags, double zx, double zy, double zt, const double L[6]) {
  cfear_pg_edge e;
  memset(&e, 0, sizeof(e));
  e.a = a; e.b = b; e.flags = flags; e.z[0] = zx; e.z[1] = zy; e.z[2] = zt;
  // Omega = U^T U with U upper triangular (L: its six entries): symmetric positive definite, every entry used
  const double U[3][3] = {{L[0], L[1], L[2]}, {0.0, L[3], L[4]}, {0.0, 0.0, L[5]}};
  double O[3][3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) { O[i][j] = 0.0; for (int k = 0; k < 3; k++) O[i][j] += U[k][i] * U[k][j]; }
  e.info[0] = O[0][0]; e.info[1] = O[0][1]; e.info[2] = O[0][2]; e.info[3] = O[1][1]; e.info[4] = O[1][2]; e.info[5] = O[2][2];
  return e;
}

int main() {
  // five nodes with headings on both sides of +-pi, six edges (one not finite), measured rotations near +-pi
  std::vector<double> x = {0.0, 0.0, 3.10, 1.5, 0.2, -3.12, 2.9, -0.4, 3.13, 4.1, 0.3, -3.05, 1.0, 2.0, 0.4};
  const double L1[6] = {20.0, 1.0, -0.5, 25.0, 0.7, 90.0}, L2[6] = {10.0, -2.0, 1.5, 12.0, -0.3, 40.0};
  std::vector<cfear_pg_edge> E = {edge(1, 0, 0, -1.4, 0.3, 0.05, L1), edge(2, 1, 0, -1.3, -0.5, 0.04, L1), edge(3, 2, 0, -1.1, 0.8, 0.1, L1),
                                  edge(4, 0, 1, 0.7, -2.1, 3.14, L2), edge(3, 0, 1, 3.5, 1.0, -3.14, L2), edge(4, 2, 1, 0.0, 0.0, 0.0, L2)};
  E[5].info[2] = std::numeric_limits<double>::quiet_NaN();
  const int n = 5, m = (int)E.size();

  // the cost: the entry's function against the sum written out, under every loss
  for (int loss = 0; loss <= 2; loss++) {
    double cost = -1.0, ref = 0.0;
    int32_t used = -1, skipped = -1;
    const int rc = graph_cost(x.data(), n, E.data(), m, loss, 0.8, &cost, &used, &skipped);
    for (int k = 0; k < 5; k++) {
      double e[3];
      edge_error_jacobians(&x[3 * E[k].a], &x[3 * E[k].b], E[k].z, e, nullptr, nullptr);
      const double s = squared_norm(e, E[k].info);
      double rho = s;
      if ((E[k].flags & 1) && loss == LOSS_HUBER && s > 0.64) rho = 2.0 * 0.8 * sqrt(s) - 0.64;
      if ((E[k].flags & 1) && loss == LOSS_CAUCHY) rho = 0.64 * log(1.0 + s / 0.64);
      ref += rho;
      if (fabs(e[2]) > PG_PI) failed++;
    }
    char what[64];
    snprintf(what, sizeof(what), "cost, loss %d (rc %d, used %d, skipped %d)", loss, rc, used, skipped);
    check(what, (rc == 0 && used == 5 && skipped == 1) ? fabs(cost - 0.5 * ref) / (0.5 * ref) : NAN, 1e-14);
  }

  // Jacobians against central differences; the gradient, blocks and products of a linearised edge against them
  double worst_j = 0.0, worst_g = 0.0, worst_d = 0.0, worst_p = 0.0;
  for (int k = 0; k < 5; k++) {
    const cfear_pg_edge& ed = E[k];
    double e[3], A[9], B[9];
    edge_error_jacobians(&x[3 * ed.a], &x[3 * ed.b], ed.z, e, A, B);
    for (int side = 0; side < 2; side++)
      for (int c = 0; c < 3; c++) {
        const double h = 1e-6;
        std::vector<double> xp = x, xm = x;
        const int node = side ? ed.b : ed.a;
        xp[3 * node + c] += h; xm[3 * node + c] -= h;
        double ep[3], em[3];
        edge_error_jacobians(&xp[3 * ed.a], &xp[3 * ed.b], ed.z, ep, nullptr, nullptr);
        edge_error_jacobians(&xm[3 * ed.a], &xm[3 * ed.b], ed.z, em, nullptr, nullptr);
        for (int r = 0; r < 3; r++) worst_j = fmax(worst_j, fabs(wrap_pi(ep[r] - em[r]) / (2.0 * h) - (side ? B : A)[3 * r + c]));
      }
    double lin[LIN_DOUBLES];
    edge_linearise(&x[3 * ed.a], &x[3 * ed.b], ed.z, ed.info, ed.flags, LOSS_CAUCHY, 0.8, lin);
    double rho, w;
    loss_eval((ed.flags & 1) ? LOSS_CAUCHY : LOSS_NONE, 0.8, squared_norm(e, ed.info), &rho, &w);
    const double O[9] = {ed.info[0], ed.info[1], ed.info[2], ed.info[1], ed.info[3], ed.info[4], ed.info[2], ed.info[4], ed.info[5]};
    for (int side = 0; side < 2; side++) {
      const double* J = side ? B : A;
      double g[3], D[6] = {0, 0, 0, 0, 0, 0};
      edge_jt(lin, side, lin + 10, g);
      edge_block(lin, side, D);
      const double Dfull[9] = {D[0], D[1], D[2], D[1], D[3], D[4], D[2], D[4], D[5]};
      for (int i = 0; i < 3; i++) {
        double gi = 0.0;
        for (int r = 0; r < 3; r++)
          for (int c = 0; c < 3; c++) gi += J[3 * r + i] * w * O[3 * r + c] * e[c];
        worst_g = fmax(worst_g, fabs(g[i] - gi) / (1.0 + fabs(gi)));
        for (int j = 0; j < 3; j++) {
          double dij = 0.0;
          for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) dij += J[3 * r + i] * w * O[3 * r + c] * J[3 * c + j];
          worst_d = fmax(worst_d, fabs(Dfull[3 * i + j] - dij) / (1.0 + fabs(dij)));
        }
      }
    }
    const double da[3] = {0.3, -0.2, 0.05}, db[3] = {-0.1, 0.4, -0.02};
    double v[3];
    edge_wju(lin, da, db, v);
    for (int r = 0; r < 3; r++) {
      double vr = 0.0;
      for (int c = 0; c < 3; c++) {
        double u = 0.0;
        for (int i = 0; i < 3; i++) u += A[3 * c + i] * da[i] + B[3 * c + i] * db[i];
        vr += w * O[3 * r + c] * u;
      }
      worst_p = fmax(worst_p, fabs(v[r] - vr) / (1.0 + fabs(vr)));
    }
  }
  check("Jacobians against central differences", worst_j, 1e-7);
  check("J^T W e of a linearised edge", worst_g, 1e-13);
  check("J^T W J of a linearised edge", worst_d, 1e-13);
  check("W (A da + B db) of a linearised edge", worst_p, 1e-13);

  {  // the 3x3 inverse
    const double M[6] = {400.0, 20.0, -10.0, 630.0, 17.0, 8100.0};
    double inv[6], worst = 0.0;
    inverse3_sym(M, inv);
    const double Mf[9] = {M[0], M[1], M[2], M[1], M[3], M[4], M[2], M[4], M[5]}, If[9] = {inv[0], inv[1], inv[2], inv[1], inv[3], inv[4], inv[2], inv[4], inv[5]};
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        double s = 0.0;
        for (int k = 0; k < 3; k++) s += Mf[3 * i + k] * If[3 * k + j];
        worst = fmax(worst, fabs(s - (i == j ? 1.0 : 0.0)));
      }
    check("inverse of a symmetric 3x3", worst, 1e-14);
  }
  {  // wrap: [-pi, pi)
    double worst = 0.0;
    const double in[6] = {PG_PI, -PG_PI, 3.0 * PG_PI, 0.5, -7.0, 100.0};
    for (int i = 0; i < 6; i++) {
      const double w = wrap_pi(in[i]);
      if (!(w >= -PG_PI && w < PG_PI)) worst = 1.0;
      worst = fmax(worst, fabs(sin(w) - sin(in[i])) + fabs(cos(w) - cos(in[i])));
    }
    check("wrap to [-pi, pi)", worst, 1e-13);
  }
  {  // refusals
    double cost = 7.0;
    cfear_pg_edge bad = E[0];
    bad.a = 5;
    int wrong = 0;
    wrong += graph_cost(x.data(), n, &bad, 1, 0, 0.1, &cost, nullptr, nullptr) != CFEAR_ERR_INVALID;
    bad.a = bad.b;
    wrong += graph_cost(x.data(), n, &bad, 1, 0, 0.1, &cost, nullptr, nullptr) != CFEAR_ERR_INVALID;
    wrong += graph_cost(x.data(), n, E.data(), m, CFEAR_LOSS_TUKEY, 0.1, &cost, nullptr, nullptr) != CFEAR_ERR_UNSUPPORTED;
    wrong += graph_cost(x.data(), n, E.data(), m, 0, 0.1, nullptr, nullptr, nullptr) != CFEAR_ERR_INVALID;
    wrong += graph_cost(nullptr, 0, nullptr, 0, 0, 0.1, &cost, nullptr, nullptr) != CFEAR_OK || cost != 0.0;
    check("refusals and the empty graph", (double)wrong, 0.0);
  }
  if (!failed) printf("ok\n");
  return failed;
}
