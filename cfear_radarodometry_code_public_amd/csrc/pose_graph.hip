// pose_graph.hip -- optimising the keyframe graph on the device: batched planar pose graphs (gfx950 only; include/cfear_hip.h states the
// problem, the step rule and the rules for skipped / refused input). What OdometryKeyframeFuser hands to the SLAM back end - the nodes,
// the odometry chain, the loop constraints (types.h:93-190) - is solved here for all sequences of a batch in one launch:
//   pose_graph_kernel       a workgroup per graph, the whole Levenberg-Marquardt loop inside: per iteration every edge is linearised once
//                           (pose_graph_dev.h: 13 doubles per edge in the graph's scratch slice), every node's gradient, diagonal block and
//                           part of H p come from walking that node's incident edges through the adjacency list built on the host (its
//                           order is the edges' order), the conjugate gradients run under the inverse of the damped diagonal blocks, and
//                           the dot products are reduced in a fixed order (blockops.h's wave sums, then the waves in sequence). No
//                           floating-point atomics; every sum is a node's own, so an edge that is skipped is an edge that is not there.
//                           The vectors live in a slice of global memory that only this workgroup touches (it stays in L2): what a wave
//                           wrote before a barrier the workgroup's other waves read behind it.
//   pose_graph_prep_kernel  the log's route: node poses -> initial poses, every node's t_be / information -> its chain edge, on the device.
// Behind them the two entries and the host-only cost (cfear_pose_graph_cost_host).
#include <algorithm>
#include <cmath>

#include "odometry_obj.h"
#include "blockops.h"
#include "pose_graph_dev.h"

static_assert(sizeof(cfear_pg_edge) == 88 && sizeof(cfear_pg_options) == 56 && sizeof(cfear_pg_summary) == 48, "the public layouts (capi.PG_*_DTYPE)");

namespace cfear_dev {
// one graph as its workgroup reads it: where its nodes, edges and adjacency rows start in the call's arrays
struct PgGraph {
  int n, m, fixed, max_lin;
  long long node0, edge0, adj0, adjoff0;
};
struct PgArgs {
  const PgGraph* graphs;
  const int* order;        // [n_graphs] workgroup -> graph, largest first
  const cfear_pg_edge* edges;
  const int* adj_off;      // per graph n + 1 offsets into its adjacency entries
  const int* adj;          // (edge << 1) | side, side 0: the node is the edge's a
  double* x;               // [nodes][3] in / out
  double* nscr;            // [nodes][PG_NODE_DOUBLES]
  double* lin;             // [edges][LIN_DOUBLES]
  int* skip;               // [edges]
  cfear_pg_summary* sums;  // [n_graphs]
  cfear_pg_options opt;
};
constexpr int PG_NODE_DOUBLES = 30;  // xn 3, D 6, M 6, p 3, r 3, d 3, q 3 (+ 3 unused)
}  // namespace cfear_dev

namespace {
using namespace cfear_dev;
using namespace cfear_pg;

constexpr int BLOCK_PG = 256, NW_PG = BLOCK_PG / 64;

// N sums at once in a fixed order: the wave's butterfly (every lane ends with the same bits), then the waves in sequence. red: N * NW_PG doubles
template <int N>
__device__ __forceinline__ void block_sum_d(double (&v)[N], double* red) {
  auto* sl = CFEAR_LDS_PTR(double, red);
#pragma unroll
  for (int k = 0; k < N; k++) v[k] = wave_sum(v[k]);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if (lane_id() == 0)
    for (int k = 0; k < N; k++) sl[N * w + k] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; k++) {
    double r = sl[k];
    for (int i = 1; i < NW_PG; i++) r += sl[N * i + k];
    v[k] = r;
  }
}
__device__ __forceinline__ double block_max_d(double v, double* red) {
  auto* sl = CFEAR_LDS_PTR(double, red);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if (lane_id() == 0) sl[w] = v;
  __syncthreads();
  double r = sl[0];
  for (int i = 1; i < NW_PG; i++) r = fmax(r, sl[i]);
  return r;
}

__global__ __launch_bounds__(BLOCK_PG) void pose_graph_kernel(PgArgs P) {
  __shared__ double red[2 * NW_PG];
  __shared__ int red_i[32];
  const int gi = P.order[blockIdx.x], tid = threadIdx.x;
  const PgGraph* Gp = P.graphs + gi;
  const int n = Gp->n, m = Gp->m, fixed = Gp->fixed, max_lin = Gp->max_lin;
  const cfear_pg_edge* E = P.edges + Gp->edge0;
  int* skip = P.skip + Gp->edge0;
  double* lin = P.lin + LIN_DOUBLES * Gp->edge0;
  const int* aoff = P.adj_off + Gp->adjoff0;
  const int* adj = P.adj + Gp->adj0;
  double* x = P.x + 3 * Gp->node0;
  double* base = P.nscr + PG_NODE_DOUBLES * Gp->node0;
  double* xn = base;
  double* Dm = base + 3 * (size_t)n;
  double* Mm = base + 9 * (size_t)n;
  double* pv = base + 15 * (size_t)n;
  double* rv = base + 18 * (size_t)n;
  double* dv = base + 21 * (size_t)n;
  double* qv = base + 24 * (size_t)n;
  const int loss = P.opt.loss;
  const double limit = P.opt.loss_limit;
  cfear_pg_summary* S = P.sums + gi;

  int used = 0;
  for (int e = tid; e < m; e += BLOCK_PG) {
    const bool ok = edge_finite(E[e].z, E[e].info);
    skip[e] = ok ? 0 : 1;
    used += ok ? 1 : 0;
  }
  used = block_sum(used, red_i);  // (its barriers: the flags are the workgroup's to read)
  if (n == 0 || used == 0) {      // (block-uniform) nothing to do: every pose keeps its bits
    if (tid == 0) {
      S->initial_cost = 0.0; S->final_cost = 0.0; S->iterations = 0; S->accepted = 0; S->linear_iterations = 0;
      S->edges_used = 0; S->edges_skipped = m; S->termination = CFEAR_PG_NOTHING_TO_DO; S->status = 0; S->pad_ = 0;
    }
    return;
  }

  // F at the poses px: every node sums the edges it is the `a` of, in its row's order; the nodes in a fixed order
  const auto cost_at = [&](const double* px) {
    double acc[1] = {0.0};
    for (int i = tid; i < n; i += BLOCK_PG) {
      double ci = 0.0;
      for (int k = aoff[i]; k < aoff[i + 1]; k++) {
        const int w = adj[k];
        if (w & 1) continue;
        const int e = w >> 1;
        if (skip[e]) continue;
        const cfear_pg_edge* ed = E + e;
        ci += edge_cost(px + 3 * (size_t)i, px + 3 * (size_t)ed->b, ed->z, ed->info, ed->flags, loss, limit);
      }
      acc[0] += ci;
    }
    block_sum_d<1>(acc, red);
    return 0.5 * acc[0];
  };

  double F = cost_at(x);
  const double F0 = F;
  double lambda = P.opt.initial_damping;
  int it = 0, accepted = 0, lin_total = 0, term = CFEAR_PG_ITERATION_LIMIT;
  while (it < P.opt.max_iterations) {
    it++;
    // ---- linearise every edge at x ----
    for (int e = tid; e < m; e += BLOCK_PG) {
      if (skip[e]) continue;
      const cfear_pg_edge* ed = E + e;
      edge_linearise(x + 3 * (size_t)ed->a, x + 3 * (size_t)ed->b, ed->z, ed->info, ed->flags, loss, limit, lin + LIN_DOUBLES * (size_t)e);
    }
    __syncthreads();
    // ---- every node: gradient, diagonal block, the preconditioner; CG starts at p = 0 ----
    double s2[2] = {0.0, 0.0};  // r . z, r . r
    for (int i = tid; i < n; i += BLOCK_PG) {
      double g[3] = {0.0, 0.0, 0.0}, D[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      for (int k = aoff[i]; k < aoff[i + 1]; k++) {
        const int w = adj[k], e = w >> 1;
        if (skip[e]) continue;
        const double* L = lin + LIN_DOUBLES * (size_t)e;
        double t[3];
        edge_jt(L, w & 1, L + 10, t);
        g[0] += t[0]; g[1] += t[1]; g[2] += t[2];
        edge_block(L, w & 1, D);
      }
      double r[3] = {0.0, 0.0, 0.0}, z[3] = {0.0, 0.0, 0.0};
      if (i != fixed) {
        double Md[6] = {D[0], D[1], D[2], D[3], D[4], D[5]}, M[6];
        Md[0] += lambda * fmax(D[0], DIAG_MIN); Md[3] += lambda * fmax(D[3], DIAG_MIN); Md[5] += lambda * fmax(D[5], DIAG_MIN);
        inverse3_sym(Md, M);
        for (int c = 0; c < 6; c++) { Dm[6 * (size_t)i + c] = D[c]; Mm[6 * (size_t)i + c] = M[c]; }
        r[0] = -g[0]; r[1] = -g[1]; r[2] = -g[2];
        sym3_mul(M, r, z);
        s2[0] += r[0] * z[0] + r[1] * z[1] + r[2] * z[2];
        s2[1] += r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
      }
      for (int c = 0; c < 3; c++) { rv[3 * (size_t)i + c] = r[c]; dv[3 * (size_t)i + c] = z[c]; pv[3 * (size_t)i + c] = 0.0; }
    }
    block_sum_d<2>(s2, red);
    double rz = s2[0], rr = s2[1];
    const double gnorm = sqrt(rr);
    int k_lin = 0;
    // ---- conjugate gradients on (H + lambda diag(H)) p = -g ----
    while (k_lin < max_lin && !(sqrt(rr) <= P.opt.linear_tolerance * gnorm)) {
      __syncthreads();  // the directions are written
      double dq[1] = {0.0};
      for (int i = tid; i < n; i += BLOCK_PG) {
        double q[3] = {0.0, 0.0, 0.0};
        if (i != fixed) {
          const double di[3] = {dv[3 * (size_t)i], dv[3 * (size_t)i + 1], dv[3 * (size_t)i + 2]};
          for (int k = aoff[i]; k < aoff[i + 1]; k++) {
            const int w = adj[k], e = w >> 1;
            if (skip[e]) continue;
            const cfear_pg_edge* ed = E + e;
            const int other = (w & 1) ? ed->a : ed->b;
            const double dj[3] = {dv[3 * (size_t)other], dv[3 * (size_t)other + 1], dv[3 * (size_t)other + 2]};
            const double* L = lin + LIN_DOUBLES * (size_t)e;
            double v[3], t[3];
            if (w & 1) edge_wju(L, dj, di, v); else edge_wju(L, di, dj, v);
            edge_jt(L, w & 1, v, t);
            q[0] += t[0]; q[1] += t[1]; q[2] += t[2];
          }
          const double* D = Dm + 6 * (size_t)i;
          q[0] += lambda * fmax(D[0], DIAG_MIN) * di[0]; q[1] += lambda * fmax(D[3], DIAG_MIN) * di[1]; q[2] += lambda * fmax(D[5], DIAG_MIN) * di[2];
          dq[0] += di[0] * q[0] + di[1] * q[1] + di[2] * q[2];
        }
        for (int c = 0; c < 3; c++) qv[3 * (size_t)i + c] = q[c];
      }
      block_sum_d<1>(dq, red);
      if (!(dq[0] > 0.0)) break;  // (block-uniform) no curvature left along d: the solve ends with what it has
      const double alpha = rz / dq[0];
      s2[0] = 0.0; s2[1] = 0.0;
      for (int i = tid; i < n; i += BLOCK_PG) {
        if (i == fixed) continue;
        double r[3], z[3];
        for (int c = 0; c < 3; c++) {
          pv[3 * (size_t)i + c] = pv[3 * (size_t)i + c] + alpha * dv[3 * (size_t)i + c];
          r[c] = rv[3 * (size_t)i + c] - alpha * qv[3 * (size_t)i + c];
          rv[3 * (size_t)i + c] = r[c];
        }
        sym3_mul(Mm + 6 * (size_t)i, r, z);
        s2[0] += r[0] * z[0] + r[1] * z[1] + r[2] * z[2];
        s2[1] += r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
      }
      block_sum_d<2>(s2, red);  // (its barriers: every node's H d has read the old directions)
      const double beta = s2[0] / rz;
      rz = s2[0]; rr = s2[1];
      for (int i = tid; i < n; i += BLOCK_PG) {
        if (i == fixed) continue;
        const double r[3] = {rv[3 * (size_t)i], rv[3 * (size_t)i + 1], rv[3 * (size_t)i + 2]};
        double z[3];
        sym3_mul(Mm + 6 * (size_t)i, r, z);
        for (int c = 0; c < 3; c++) dv[3 * (size_t)i + c] = z[c] + beta * dv[3 * (size_t)i + c];
      }
      k_lin++;
    }
    lin_total += k_lin;
    // ---- the step ----
    double pmax = 0.0;
    for (int i = tid; i < n; i += BLOCK_PG)
      for (int c = 0; c < 3; c++) {
        const double p = pv[3 * (size_t)i + c];
        pmax = fmax(pmax, fabs(p));
        xn[3 * (size_t)i + c] = x[3 * (size_t)i + c] + p;
      }
    pmax = block_max_d(pmax, red);  // (its barriers: the candidate is written)
    if (pmax < P.opt.parameter_tolerance) { term = CFEAR_PG_CONVERGED_STEP; break; }
    const double Fn = cost_at(xn);
    if (Fn < F) {
      for (int i = tid; i < n; i += BLOCK_PG) {
        if (i == fixed) continue;
        for (int c = 0; c < 3; c++) x[3 * (size_t)i + c] = xn[3 * (size_t)i + c];
      }
      __syncthreads();
      accepted++;
      const double drop = F - Fn, Fold = F;
      F = Fn;
      lambda = fmax(lambda / 3.0, LAMBDA_MIN);
      if (drop <= P.opt.function_tolerance * Fold) { term = CFEAR_PG_CONVERGED_COST; break; }
    } else {
      if (lambda >= LAMBDA_MAX) { term = CFEAR_PG_DAMPING_LIMIT; break; }
      lambda = fmin(4.0 * lambda, LAMBDA_MAX);
    }
  }
  if (tid == 0) {
    S->initial_cost = F0; S->final_cost = F; S->iterations = it; S->accepted = accepted; S->linear_iterations = lin_total;
    S->edges_used = used; S->edges_skipped = m - used; S->termination = term; S->status = 0; S->pad_ = 0;
  }
}

// the log's route: sequence g's recorded nodes -> graph g's initial poses and the measurement / information of its chain edges (edge i - 1
// is node i's own: a = i, b = i - 1 are the host's)
__global__ __launch_bounds__(BLOCK_PG) void pose_graph_prep_kernel(const PgGraph* graphs, KfLog L, cfear_pg_edge* edges, double* x) {
  const PgGraph* G = graphs + blockIdx.x;
  const cfear_keyframe_node* nodes = L.nodes + (size_t)blockIdx.x * L.max_kf;
  for (int i = threadIdx.x; i < G->n; i += BLOCK_PG) {
    const cfear_keyframe_node* nd = nodes + i;
    double* xi = x + 3 * (G->node0 + i);
    xi[0] = nd->pose[0]; xi[1] = nd->pose[1]; xi[2] = nd->pose[2];
    if (i == 0) continue;
    cfear_pg_edge* e = edges + G->edge0 + (i - 1);
    e->z[0] = nd->t_be[0]; e->z[1] = nd->t_be[1]; e->z[2] = nd->t_be[2];
    const double* I = nd->information;  // the (x, y, yaw) block's upper triangle, as replay._g2o_edge writes it
    e->info[0] = I[0]; e->info[1] = I[1]; e->info[2] = I[5]; e->info[3] = I[7]; e->info[4] = I[11]; e->info[5] = I[35];
  }
}

void pg_defaults(cfear_pg_options* o) {
  memset(o, 0, sizeof(*o));
  o->max_iterations = 50; o->max_linear_iterations = 0; o->loss = CFEAR_LOSS_NONE;
  o->linear_tolerance = 1e-8; o->function_tolerance = 1e-12; o->parameter_tolerance = 1e-10; o->initial_damping = 1e-4; o->loss_limit = 0.1;
}

int pg_check_options(cfear_ctx* ctx, const char* what, const cfear_pg_options& o) {
  char msg[200];
  if (o.loss != CFEAR_LOSS_NONE && o.loss != CFEAR_LOSS_HUBER && o.loss != CFEAR_LOSS_CAUCHY) {
    snprintf(msg, sizeof(msg), "%s: options.loss = %d: CFEAR_LOSS_NONE, CFEAR_LOSS_HUBER or CFEAR_LOSS_CAUCHY", what, o.loss);
    return cfear_fail(ctx, CFEAR_ERR_UNSUPPORTED, msg);
  }
  const double v[5] = {o.linear_tolerance, o.function_tolerance, o.parameter_tolerance, o.initial_damping, o.loss_limit};
  const char* names[5] = {"linear_tolerance", "function_tolerance", "parameter_tolerance", "initial_damping", "loss_limit"};
  for (int i = 0; i < 5; i++)
    if (!std::isfinite(v[i]) || v[i] < 0.0 || (i >= 3 && !(v[i] > 0.0))) {
      snprintf(msg, sizeof(msg), "%s: options.%s = %g", what, names[i], v[i]);
      return cfear_fail(ctx, CFEAR_ERR_INVALID, msg);
    }
  if (o.max_iterations < 0 || o.max_linear_iterations < 0) {
    snprintf(msg, sizeof(msg), "%s: options.max_iterations = %d, max_linear_iterations = %d", what, o.max_iterations, o.max_linear_iterations);
    return cfear_fail(ctx, CFEAR_ERR_INVALID, msg);
  }
  return CFEAR_OK;
}

// every edge of every graph: a, b inside the graph and different (before anything is launched or written)
int pg_check_edges(cfear_ctx* ctx, const char* what, int n_graphs, const int32_t* node_off, const int32_t* edge_off, const cfear_pg_edge* edges) {
  char msg[200];
  for (int g = 0; g < n_graphs; g++) {
    const int n = node_off[g + 1] - node_off[g];
    for (int k = edge_off[g]; k < edge_off[g + 1]; k++) {
      const cfear_pg_edge& e = edges[k];
      const int local = k - edge_off[g];
      if (e.a < 0 || e.a >= n) { snprintf(msg, sizeof(msg), "%s: graph %d edge %d: a = %d, the graph has %d nodes", what, g, local, e.a, n); return cfear_fail(ctx, CFEAR_ERR_INVALID, msg); }
      if (e.b < 0 || e.b >= n) { snprintf(msg, sizeof(msg), "%s: graph %d edge %d: b = %d, the graph has %d nodes", what, g, local, e.b, n); return cfear_fail(ctx, CFEAR_ERR_INVALID, msg); }
      if (e.a == e.b) { snprintf(msg, sizeof(msg), "%s: graph %d edge %d: a = b = %d", what, g, local, e.a); return cfear_fail(ctx, CFEAR_ERR_INVALID, msg); }
    }
  }
  return CFEAR_OK;
}

// The call behind both entries: checked offsets and edges -> the tables (graphs largest first, an adjacency row per node in the edges'
// order), one block of the pool, one launch (with a log: the preparation in front of it), the poses and summaries back.
int pg_solve(cfear_ctx* ctx, const char* what, int n_graphs, const int32_t* node_off, const int32_t* edge_off, const cfear_pg_edge* edges, const int32_t* fixed,
             const cfear_pg_options& opt, const KfLog* log, double* poses, cfear_pg_summary* summaries) {
  const size_t N = (size_t)node_off[n_graphs], M = (size_t)edge_off[n_graphs];
  std::vector<PgGraph> graphs((size_t)n_graphs);
  std::vector<int> order((size_t)n_graphs), adj_off(N + (size_t)n_graphs), adj(2 * M);
  for (int g = 0; g < n_graphs; g++) {
    PgGraph& G = graphs[(size_t)g];
    G.n = node_off[g + 1] - node_off[g]; G.m = edge_off[g + 1] - edge_off[g];
    G.fixed = fixed ? fixed[g] : 0;
    G.max_lin = opt.max_linear_iterations > 0 ? opt.max_linear_iterations : (int)std::min<long long>(30LL * G.n, 2147483647LL);
    G.node0 = node_off[g]; G.edge0 = edge_off[g]; G.adj0 = 2LL * edge_off[g]; G.adjoff0 = (long long)node_off[g] + g;
    order[(size_t)g] = g;
    int* off = adj_off.data() + G.adjoff0;  // counting sort of the (edge, side) entries by node: rows in the edges' order
    for (int i = 0; i <= G.n; i++) off[i] = 0;
    const cfear_pg_edge* E = edges + G.edge0;
    for (int k = 0; k < G.m; k++) { off[E[k].a + 1]++; off[E[k].b + 1]++; }
    for (int i = 0; i < G.n; i++) off[i + 1] += off[i];
    std::vector<int> cur(off, off + G.n);
    int* row = adj.data() + G.adj0;
    for (int k = 0; k < G.m; k++) { row[cur[(size_t)E[k].a]++] = 2 * k; row[cur[(size_t)E[k].b]++] = 2 * k + 1; }
  }
  std::stable_sort(order.begin(), order.end(), [&](int p, int q) {
    return (long long)graphs[(size_t)p].n + graphs[(size_t)p].m > (long long)graphs[(size_t)q].n + graphs[(size_t)q].m;
  });
  // one block of the pool: graphs | order | edges | adjacency offsets | adjacency | poses | node scratch | linearised edges | skip flags | summaries
  size_t o = 0;
  const auto take = [&](size_t bytes) { const size_t at = o; o = align_up(o + bytes, 256); return at; };
  const size_t graphs_o = take(sizeof(PgGraph) * (size_t)n_graphs), order_o = take(sizeof(int) * (size_t)n_graphs), edges_o = take(sizeof(cfear_pg_edge) * M);
  const size_t aoff_o = take(sizeof(int) * adj_off.size()), adj_o = take(sizeof(int) * adj.size()), x_o = take(sizeof(double) * 3 * N);
  const size_t nscr_o = take(sizeof(double) * PG_NODE_DOUBLES * N), lin_o = take(sizeof(double) * LIN_DOUBLES * M), skip_o = take(sizeof(int) * M);
  const size_t sums_o = take(sizeof(cfear_pg_summary) * (size_t)n_graphs);
  void* work = nullptr;
  size_t work_bytes = 0;
  CFEAR_TRY(cfear_pool_alloc(ctx, o, &work, &work_bytes));
  unsigned char* wb = static_cast<unsigned char*>(work);
  PgArgs A;
  A.graphs = reinterpret_cast<const PgGraph*>(wb + graphs_o); A.order = reinterpret_cast<const int*>(wb + order_o);
  A.edges = reinterpret_cast<const cfear_pg_edge*>(wb + edges_o); A.adj_off = reinterpret_cast<const int*>(wb + aoff_o);
  A.adj = reinterpret_cast<const int*>(wb + adj_o); A.x = reinterpret_cast<double*>(wb + x_o); A.nscr = reinterpret_cast<double*>(wb + nscr_o);
  A.lin = reinterpret_cast<double*>(wb + lin_o); A.skip = reinterpret_cast<int*>(wb + skip_o); A.sums = reinterpret_cast<cfear_pg_summary*>(wb + sums_o);
  A.opt = opt;
  std::vector<double> hx(3 * N);  // (the caller's arrays stay untouched unless the whole call succeeds)
  std::vector<cfear_pg_summary> hs((size_t)n_graphs);
  hipStream_t st = ctx->stream;
  const auto up = [&](size_t at, const void* src, size_t bytes) { return bytes ? hipMemcpyAsync(wb + at, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess; };
  hipError_t e = up(graphs_o, graphs.data(), sizeof(PgGraph) * (size_t)n_graphs);
  if (e == hipSuccess) e = up(order_o, order.data(), sizeof(int) * (size_t)n_graphs);
  if (e == hipSuccess) e = up(edges_o, edges, sizeof(cfear_pg_edge) * M);
  if (e == hipSuccess) e = up(aoff_o, adj_off.data(), sizeof(int) * adj_off.size());
  if (e == hipSuccess) e = up(adj_o, adj.data(), sizeof(int) * adj.size());
  if (e == hipSuccess && !log) e = up(x_o, poses, sizeof(double) * 3 * N);
  if (e == hipSuccess && log) {
    hipLaunchKernelGGL(pose_graph_prep_kernel, dim3(n_graphs), dim3(BLOCK_PG), 0, st, A.graphs, *log, reinterpret_cast<cfear_pg_edge*>(wb + edges_o), A.x);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(pose_graph_kernel, dim3(n_graphs), dim3(BLOCK_PG), 0, st, A);
    e = hipGetLastError();
  }
  if (e == hipSuccess && N) e = hipMemcpyAsync(hx.data(), A.x, sizeof(double) * 3 * N, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(hs.data(), A.sums, sizeof(cfear_pg_summary) * (size_t)n_graphs, hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);  // (the host tables are read, and the block is in use, until here)
  if (e == hipSuccess) e = es;
  cfear_pool_free(ctx, work, work_bytes);
  if (e != hipSuccess) return cfear_fail(ctx, CFEAR_ERR_HIP, what, e);
  if (N) memcpy(poses, hx.data(), sizeof(double) * 3 * N);
  memcpy(summaries, hs.data(), sizeof(cfear_pg_summary) * (size_t)n_graphs);
  return CFEAR_OK;
}

}  // namespace

extern "C" {

void cfear_pg_default_options(cfear_pg_options* options) {
  if (options) pg_defaults(options);
}

int cfear_pose_graph_optimize(cfear_ctx* ctx, int n_graphs, const int32_t* node_offsets, const int32_t* edge_offsets, const cfear_pg_edge* edges,
                              const int32_t* fixed, const cfear_pg_options* options, double* poses_xyt, cfear_pg_summary* summaries) {
  const char* what = "pose_graph_optimize";
  if (!ctx || n_graphs < 1 || !node_offsets || !edge_offsets || !summaries) return cfear_fail(ctx, CFEAR_ERR_INVALID, "pose_graph_optimize: bad argument");
  char msg[200];
  if (node_offsets[0] != 0 || edge_offsets[0] != 0) return cfear_fail(ctx, CFEAR_ERR_INVALID, "pose_graph_optimize: node_offsets[0] and edge_offsets[0] must be 0");
  for (int g = 0; g < n_graphs; g++) {
    if (node_offsets[g + 1] < node_offsets[g] || edge_offsets[g + 1] < edge_offsets[g]) {
      snprintf(msg, sizeof(msg), "%s: graph %d: the offsets do not ascend (nodes %d .. %d, edges %d .. %d)", what, g, node_offsets[g], node_offsets[g + 1],
               edge_offsets[g], edge_offsets[g + 1]);
      return cfear_fail(ctx, CFEAR_ERR_INVALID, msg);
    }
    const int n = node_offsets[g + 1] - node_offsets[g];
    if (fixed && n > 0 && (fixed[g] < 0 || fixed[g] >= n)) {
      snprintf(msg, sizeof(msg), "%s: graph %d: fixed = %d, the graph has %d nodes", what, g, fixed[g], n);
      return cfear_fail(ctx, CFEAR_ERR_INVALID, msg);
    }
  }
  if ((node_offsets[n_graphs] > 0 && !poses_xyt) || (edge_offsets[n_graphs] > 0 && !edges)) return cfear_fail(ctx, CFEAR_ERR_INVALID, "pose_graph_optimize: bad argument");
  cfear_pg_options opt;
  if (options) opt = *options; else pg_defaults(&opt);
  CFEAR_TRY(pg_check_options(ctx, what, opt));
  CFEAR_TRY(pg_check_edges(ctx, what, n_graphs, node_offsets, edge_offsets, edges));
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return pg_solve(ctx, what, n_graphs, node_offsets, edge_offsets, edges, fixed, opt, nullptr, poses_xyt, summaries);
}

int cfear_odometry_keyframe_optimize(cfear_ctx* ctx, cfear_odometry* o, const cfear_keyframe_edge* edges, int m, const cfear_pg_options* options,
                                     double* poses_out, int capacity, int32_t* pose_offsets, cfear_pg_summary* summaries) {
  const char* what = "odometry_keyframe_optimize";
  if (!ctx || !o || m < 0 || (m > 0 && !edges) || !pose_offsets || capacity < 0)
    return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_keyframe_optimize: bad argument");
  if (!o->kf.what) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_keyframe_optimize: keyframe recording is off (cfear_odometry_set_keyframe_recording)");
  cfear_pg_options opt;
  if (options) opt = *options; else pg_defaults(&opt);
  CFEAR_TRY(pg_check_options(ctx, what, opt));
  CFEAR_TRY(odo_drain(ctx, o));
  const KfLog L = o->kf.view();
  const int B = o->B;
  std::vector<int> counts(4 * (size_t)B);
  CFEAR_HIP_CHECK(ctx, hipMemcpy(counts.data(), L.counts, sizeof(int) * counts.size(), hipMemcpyDeviceToHost));
  // ---- the checks: nothing is launched, and nothing written, before every edge has passed ----
  char msg[200];
  std::vector<int> extra((size_t)B, 0);
  for (int k = 0; k < m; k++) {
    const cfear_keyframe_edge& e = edges[k];
    if (e.success == 0 || e.status != 0) continue;  // left out
    if (e.sequence < 0 || e.sequence >= B) { snprintf(msg, sizeof(msg), "%s: edges[%d].sequence = %d: no such sequence", what, k, e.sequence); return cfear_fail(ctx, CFEAR_ERR_INVALID, msg); }
    const int n = counts[4 * (size_t)e.sequence];
    if (e.to < 0 || e.to >= n) { snprintf(msg, sizeof(msg), "%s: edges[%d].to = %d: sequence %d has recorded %d keyframes", what, k, e.to, e.sequence, n); return cfear_fail(ctx, CFEAR_ERR_INVALID, msg); }
    if (e.from < 0 || e.from >= n) { snprintf(msg, sizeof(msg), "%s: edges[%d].from = %d: sequence %d has recorded %d keyframes", what, k, e.from, e.sequence, n); return cfear_fail(ctx, CFEAR_ERR_INVALID, msg); }
    if (e.to == e.from) { snprintf(msg, sizeof(msg), "%s: edges[%d].to = from = %d", what, k, e.to); return cfear_fail(ctx, CFEAR_ERR_INVALID, msg); }
    extra[(size_t)e.sequence]++;
  }
  std::vector<int32_t> node_off((size_t)B + 1, 0), edge_off((size_t)B + 1, 0);
  for (int q = 0; q < B; q++) {
    const int n = counts[4 * (size_t)q];
    node_off[(size_t)q + 1] = node_off[(size_t)q] + n;
    edge_off[(size_t)q + 1] = edge_off[(size_t)q] + std::max(n - 1, 0) + extra[(size_t)q];
  }
  for (int q = 0; q <= B; q++) pose_offsets[q] = node_off[(size_t)q];
  if (!poses_out && capacity == 0 && !summaries) return CFEAR_OK;  // the offsets alone
  if (!poses_out || !summaries || capacity < node_off[(size_t)B]) {
    snprintf(msg, sizeof(msg), "%s: %d poses, capacity %d", what, node_off[(size_t)B], capacity);
    return cfear_fail(ctx, (poses_out && summaries) ? CFEAR_ERR_CAPACITY : CFEAR_ERR_INVALID, msg);
  }
  // ---- the edge list: per sequence its chain (measurement and information follow on the device), then the caller's in their order ----
  std::vector<cfear_pg_edge> pe((size_t)edge_off[(size_t)B]);
  if (!pe.empty()) memset(pe.data(), 0, sizeof(cfear_pg_edge) * pe.size());
  std::vector<int> cur((size_t)B);
  for (int q = 0; q < B; q++) {
    const int n = counts[4 * (size_t)q];
    for (int i = 1; i < n; i++) { cfear_pg_edge& e = pe[(size_t)edge_off[(size_t)q] + i - 1]; e.a = i; e.b = i - 1; }
    cur[(size_t)q] = edge_off[(size_t)q] + std::max(n - 1, 0);
  }
  for (int k = 0; k < m; k++) {
    const cfear_keyframe_edge& e = edges[k];
    if (e.success == 0 || e.status != 0) continue;
    cfear_pg_edge& d = pe[(size_t)cur[(size_t)e.sequence]++];
    d.a = e.to; d.b = e.from; d.flags = 1;
    for (int i = 0; i < 3; i++) d.z[i] = e.t_be[i];
    const double* I = e.information;
    d.info[0] = I[0]; d.info[1] = I[1]; d.info[2] = I[5]; d.info[3] = I[7]; d.info[4] = I[11]; d.info[5] = I[35];
  }
  return pg_solve(ctx, what, B, node_off.data(), edge_off.data(), pe.data(), nullptr, opt, &L, poses_out, summaries);
}

int cfear_pose_graph_cost_host(const double* poses_xyt, int n_nodes, const cfear_pg_edge* edges, int n_edges, int loss, double loss_limit, double* cost,
                               int32_t* used, int32_t* skipped) {
  return cfear_pg::graph_cost(poses_xyt, n_nodes, edges, n_edges, loss, loss_limit, cost, used, skipped);
}

}  // extern "C"
