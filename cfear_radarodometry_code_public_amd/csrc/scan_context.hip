// scan_context.hip -- loop candidates by appearance (gfx950 only): Scan-Context descriptors (Kim & Kim, IROS 2018) of clouds and their
// two-stage matching, as include/cfear_hip.h defines them (cfear_sc_params; the rules are scan_context_dev.h's, one copy for the kernels,
// the host and host/scan_context_check.cpp).
//   sc_describe_kernel   a workgroup per cloud: the bins live in LDS (<= 120 x 40 words), every point adds itself with an integer LDS
//                        atomic (max / add: exact and free of any order), then the ring sums. The layout table comes from the host.
//   sc_ring_sums_kernel  the ring keys of caller descriptors (cfear_scan_context_match takes bins alone).
//   sc_match_kernel      a workgroup per `to`. Stage 1: the n_keys smallest ring-key distances among the eligible `from`, one per round -
//                        the smallest (K, index) above the last one chosen, a block-wide minimum in a fixed tree: deterministic, no list
//                        to exclude from. Stage 2: a wave per (to, from) pair, `to` as floats in LDS for all waves, `from` in the wave's
//                        own LDS rows (column stride odd: the lanes of a wave read different columns), a lane per shift (two for more
//                        than 64 sectors) through shift_distance_f32, the minimum over the lanes with ties to the smaller shift. Every
//                        wave keeps its max_per_node best in LDS ordered by (distance, from); thread 0 merges them into the fixed slots
//                        of `to`. Plain FP32 vector arithmetic: the bins are 24-bit integers, which bf16 would round.
// No floating-point atomics. The slots are compacted on the host in (set, to, distance) order. Working memory: one block of the
// context's pool per call.
#include <algorithm>
#include <cmath>

#include "odometry_obj.h"
#include "scan_context_dev.h"

static_assert(sizeof(cfear_sc_params) == 48 && sizeof(cfear_sc_candidate) == 40, "the public layouts (capi.ScParams / SC_CANDIDATE_DTYPE)");

namespace cfear_dev {
// One cloud to describe: n points from `first` on in the call's points
struct ScJob {
  unsigned long long first;
  int n, pad_;
};
// One entry of a wave's best list, and of the fixed slots of a `to`
struct ScTop {
  unsigned long long K;
  float d;
  int from, shift, pad_;
};
struct ScMatchArgs {
  const uint32_t* bins;       // [N][n_sectors][n_rings]
  const uint32_t* ring_sums;  // [N][n_rings]
  const int* set_off;         // [n_sets + 1]
  ScTop* slots;               // [N][mp]
  int* counts;                // [N]
  int n_sets, nr, ns, stride;
  int gap, n_keys, mp, waves;
  double max_distance;
};
}  // namespace cfear_dev

namespace {

using namespace cfear_sc;
using cfear_dev::ScJob;
using cfear_dev::ScMatchArgs;
using cfear_dev::ScTop;

constexpr int BLOCK_SC = 256;

__global__ __launch_bounds__(BLOCK_SC) void sc_describe_kernel(const float* points, const ScJob* jobs, const double* table /*[nr + 1] edges, [ns][2] directions*/,
                                                               int nr, int ns, int value, uint32_t* bins, uint32_t* ring_sums, int* dropped) {
  __shared__ uint32_t sb[MAX_SECTORS * MAX_RINGS];
  __shared__ double s_edge[MAX_RINGS + 1];
  __shared__ double s_dir[2 * MAX_SECTORS];
  __shared__ int s_drop;
  const int b = blockIdx.x, tid = threadIdx.x, nb = nr * ns;
  for (int i = tid; i < nb; i += BLOCK_SC) sb[i] = 0u;
  for (int i = tid; i <= nr; i += BLOCK_SC) s_edge[i] = table[i];
  for (int i = tid; i < 2 * ns; i += BLOCK_SC) s_dir[i] = table[nr + 1 + i];
  if (tid == 0) s_drop = 0;
  __syncthreads();
  const ScJob J = jobs[b];
  const float* p = points + 3 * (size_t)J.first;
  int drop = 0;
  for (int i = tid; i < J.n; i += BLOCK_SC) {
    const float x = p[3 * (size_t)i], y = p[3 * (size_t)i + 1], w = p[3 * (size_t)i + 2];
    int ring, sector;
    unsigned v;
    const int rc = bin_of_point(x, y, w, nr, ns, s_edge, s_dir, &ring, &sector, &v);
    if (rc == BIN_DROPPED) drop++;
    if (rc != BIN_OK) continue;
    uint32_t* cell = &sb[sector * nr + ring];  // (ring < nr and sector < ns: both are counts over fewer entries than that)
    if (value == CFEAR_SC_MAX) atomicMax(cell, v);
    else atomicAdd(cell, value == CFEAR_SC_SUM ? v : 1u);
  }
  if (drop) atomicAdd(&s_drop, drop);
  __syncthreads();
  uint32_t* out = bins + (size_t)b * nb;
  for (int i = tid; i < nb; i += BLOCK_SC) out[i] = sb[i];
  if (tid < nr) {
    uint32_t s = 0;
    for (int j = 0; j < ns; j++) s += sb[j * nr + tid];
    ring_sums[(size_t)b * nr + tid] = s;
  }
  if (tid == 0 && dropped) dropped[b] = s_drop;
}

__global__ __launch_bounds__(BLOCK_SC) void sc_ring_sums_kernel(const uint32_t* bins, long long total /* descriptors x rings */, int nr, int ns, uint32_t* ring_sums) {
  const long long i = (long long)blockIdx.x * BLOCK_SC + threadIdx.x;
  if (i >= total) return;
  const long long d = i / nr;
  const int r = (int)(i - d * nr);
  const uint32_t* b = bins + (size_t)d * nr * ns;
  uint32_t s = 0;
  for (int j = 0; j < ns; j++) s += b[j * nr + r];
  ring_sums[i] = s;
}

// the LDS of sc_match_kernel, in bytes from the start: what the host sizes and the kernel walks
struct ScLds {
  size_t redK, top, redI, cand, topn, ars, fa, na, wave0, wave_bytes, total;
};
__host__ __device__ inline ScLds sc_lds(int nr, int ns, int stride, int mp, int waves) {
  ScLds L;
  const size_t T = 64 * (size_t)waves;
  size_t o = 0;
  L.redK = o; o += 8 * T;
  L.top = o; o += sizeof(ScTop) * (size_t)mp * waves;
  L.redI = o; o += 4 * T;
  L.cand = o; o += 4 * (size_t)MAX_KEYS;
  L.topn = o; o += 4 * 4;
  L.ars = o; o += 4 * (size_t)MAX_RINGS;
  L.fa = o; o += 4 * (size_t)ns * stride;
  L.na = o; o += 4 * (size_t)ns;
  L.wave0 = o;
  L.wave_bytes = 4 * ((size_t)ns * stride + ns);
  L.total = o + L.wave_bytes * waves;
  return L;
}

__global__ __launch_bounds__(BLOCK_SC) void sc_match_kernel(ScMatchArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int T = 64 * A.waves, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int nr = A.nr, ns = A.ns, st = A.stride, mp = A.mp, nb = nr * ns;
  const ScLds L = sc_lds(nr, ns, st, mp, A.waves);
  unsigned long long* redK = reinterpret_cast<unsigned long long*>(lds + L.redK);
  ScTop* top = reinterpret_cast<ScTop*>(lds + L.top);
  int* redI = reinterpret_cast<int*>(lds + L.redI);
  int* cand = reinterpret_cast<int*>(lds + L.cand);
  int* topn = reinterpret_cast<int*>(lds + L.topn);
  uint32_t* ars = reinterpret_cast<uint32_t*>(lds + L.ars);
  float* fa = reinterpret_cast<float*>(lds + L.fa);
  float* na = reinterpret_cast<float*>(lds + L.na);
  float* fb = reinterpret_cast<float*>(lds + L.wave0 + L.wave_bytes * wave);
  float* nbm = fb + (size_t)ns * st;

  const int g = blockIdx.x;  // the descriptor across all sets; its set: the last one that starts at or before g (an empty set never is)
  int lo = 0, hi = A.n_sets;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (A.set_off[mid] <= g) lo = mid; else hi = mid;
  }
  const int base = A.set_off[lo], to = g - base;
  const int elig = to - A.gap + 1;  // `from` in 0 .. to - gap
  if (elig <= 0) {                  // (block-uniform)
    if (tid == 0) A.counts[g] = 0;
    return;
  }
  {
    const uint32_t* src = A.bins + (size_t)g * nb;
    for (int i = tid; i < nb; i += T) {
      const int j = i / nr;
      fa[j * st + (i - j * nr)] = (float)src[i];
    }
    if (tid < nr) ars[tid] = A.ring_sums[(size_t)g * nr + tid];
    if (tid < 4) topn[tid] = 0;
  }
  __syncthreads();
  for (int j = tid; j < ns; j += T) na[j] = column_norm_f32(fa + (size_t)j * st, nr);
  const uint32_t* rs0 = A.ring_sums + (size_t)base * nr;

  // ---- stage 1: the n_keys smallest (K, from), ascending; with no more eligible than that every one of them, in index order ----
  const bool keyed = A.n_keys > 0 && elig > A.n_keys;
  const int ncand = keyed ? A.n_keys : elig;
  if (keyed) {
    unsigned long long lastK = 0;
    int lastI = -1;
    for (int round = 0; round < ncand; round++) {
      unsigned long long bestK = ~0ull;
      int bestI = 0x7fffffff;
      for (int f = tid; f < elig; f += T) {
        const unsigned long long K = key_distance(ars, rs0 + (size_t)f * nr, nr);
        if (key_less(lastK, lastI, K, f) && key_less(K, f, bestK, bestI)) { bestK = K; bestI = f; }
      }
      redK[tid] = bestK; redI[tid] = bestI;
      __syncthreads();
      for (int s = T >> 1; s > 0; s >>= 1) {
        if (tid < s && key_less(redK[tid + s], redI[tid + s], redK[tid], redI[tid])) { redK[tid] = redK[tid + s]; redI[tid] = redI[tid + s]; }
        __syncthreads();
      }
      lastK = redK[0]; lastI = redI[0];
      if (tid == 0) cand[round] = lastI;
      __syncthreads();  // (redK / redI are written again in the next round)
    }
  }

  // ---- stage 2: a wave per pair, a lane per shift ----
  ScTop* mine = top + (size_t)wave * mp;
  for (int c0 = 0; c0 < ncand; c0 += A.waves) {
    const int c = c0 + wave;
    const bool active = c < ncand;  // (wave-uniform)
    const int f = active ? (keyed ? cand[c] : c) : 0;
    __syncthreads();  // the pair before has been read (and, the first time round, the norms of `to` and the candidates are written)
    if (active) {
      const uint32_t* src = A.bins + (size_t)(base + f) * nb;
      for (int i = lane; i < nb; i += 64) {
        const int j = i / nr;
        fb[j * st + (i - j * nr)] = (float)src[i];
      }
    }
    __syncthreads();
    if (active)
      for (int j = lane; j < ns; j += 64) nbm[j] = column_norm_f32(fb + (size_t)j * st, nr);
    __syncthreads();
    if (!active) continue;
    float bd = 2.0f;  // (a distance lies in [0, 1]: a lane without a shift never wins)
    int bs = 0x7fffffff;
    for (int s = lane; s < ns; s += 64) {
      const float d = shift_distance_f32(fa, na, fb, nbm, nr, ns, st, s);
      if (shift_less(d, s, bd, bs)) { bd = d; bs = s; }
    }
    for (int m = 32; m > 0; m >>= 1) {
      const float od = __shfl_xor(bd, m, 64);
      const int os = __shfl_xor(bs, m, 64);
      if (shift_less(od, os, bd, bs)) { bd = od; bs = os; }
    }
    if (lane == 0 && (double)bd <= A.max_distance) {  // into the wave's best, ordered by (distance, from)
      int n = topn[wave];
      int pos = n;
      while (pos > 0 && (bd < mine[pos - 1].d || (bd == mine[pos - 1].d && f < mine[pos - 1].from))) pos--;
      if (pos < mp) {
        const int last = n < mp ? n : mp - 1;
        for (int k = last; k > pos; k--) mine[k] = mine[k - 1];
        ScTop e;
        e.K = key_distance(ars, rs0 + (size_t)f * nr, nr); e.d = bd; e.from = f; e.shift = bs; e.pad_ = 0;
        mine[pos] = e;
        if (n < mp) topn[wave] = n + 1;
      }
    }
  }
  __syncthreads();
  if (tid != 0) return;
  int head[4] = {0, 0, 0, 0};
  ScTop* out = A.slots + (size_t)g * mp;
  int n = 0;
  for (; n < mp; n++) {
    int bw = -1;
    for (int w = 0; w < A.waves; w++) {
      if (head[w] >= topn[w]) continue;
      const ScTop& e = top[(size_t)w * mp + head[w]];
      if (bw < 0) { bw = w; continue; }
      const ScTop& q = top[(size_t)bw * mp + head[bw]];
      if (e.d < q.d || (e.d == q.d && e.from < q.from)) bw = w;
    }
    if (bw < 0) break;
    out[n] = top[(size_t)bw * mp + head[bw]];
    head[bw]++;
  }
  A.counts[g] = n;
}

// ---- the host side ----------------------------------------------------------------------------------------------------------------------

void sc_defaults(cfear_sc_params* p) {
  memset(p, 0, sizeof(*p));
  p->n_rings = 20; p->n_sectors = 60; p->value = CFEAR_SC_MAX; p->source = 0; p->min_index_gap = 6; p->n_keys = 10; p->max_per_node = 1;
  p->max_range = 80.0; p->max_distance = 0.4;
}

// the refusal of a field, or nullptr; msg: where the text goes
const char* sc_param_fault(const cfear_sc_params& p, char* msg, size_t len) {
  if (p.n_rings < 1 || p.n_rings > MAX_RINGS) { snprintf(msg, len, "params.n_rings = %d: 1 .. %d", p.n_rings, MAX_RINGS); return msg; }
  if (p.n_sectors < 1 || p.n_sectors > MAX_SECTORS) { snprintf(msg, len, "params.n_sectors = %d: 1 .. %d", p.n_sectors, MAX_SECTORS); return msg; }
  if (!std::isfinite(p.max_range) || !(p.max_range > 0.0)) { snprintf(msg, len, "params.max_range = %g: finite and above 0", p.max_range); return msg; }
  if (p.value != CFEAR_SC_MAX && p.value != CFEAR_SC_SUM && p.value != CFEAR_SC_COUNT) { snprintf(msg, len, "params.value = %d: CFEAR_SC_MAX, CFEAR_SC_SUM or CFEAR_SC_COUNT", p.value); return msg; }
  if (p.source != 0 && p.source != 1) { snprintf(msg, len, "params.source = %d: 0 (the filtered cloud) or 1 (the peaks cloud)", p.source); return msg; }
  if (p.min_index_gap < 1) { snprintf(msg, len, "params.min_index_gap = %d: at least 1", p.min_index_gap); return msg; }
  if (p.n_keys < 0 || p.n_keys > MAX_KEYS) { snprintf(msg, len, "params.n_keys = %d: 0 (exhaustive) or 1 .. %d", p.n_keys, MAX_KEYS); return msg; }
  if (p.max_per_node < 1 || p.max_per_node > MAX_PER_NODE) { snprintf(msg, len, "params.max_per_node = %d: 1 .. %d", p.max_per_node, MAX_PER_NODE); return msg; }
  if (!(p.max_distance > 0.0 && p.max_distance <= 1.0)) { snprintf(msg, len, "params.max_distance = %g: in (0, 1]", p.max_distance); return msg; }
  return nullptr;
}

int sc_params(cfear_ctx* ctx, const char* what, const cfear_sc_params* in, cfear_sc_params* out) {
  if (in) *out = *in; else sc_defaults(out);
  char text[160], msg[256];
  if (sc_param_fault(*out, text, sizeof(text))) {
    snprintf(msg, sizeof(msg), "%s: %s", what, text);
    return cfear_fail(ctx, CFEAR_ERR_INVALID, msg);
  }
  return CFEAR_OK;
}

// offsets[0 .. n] ascend from 0
int sc_check_offsets(cfear_ctx* ctx, const char* what, const char* name, const int32_t* off, int n) {
  char msg[200];
  if (off[0] != 0) { snprintf(msg, sizeof(msg), "%s: %s[0] = %d, must be 0", what, name, off[0]); return cfear_fail(ctx, CFEAR_ERR_INVALID, msg); }
  for (int i = 0; i < n; i++)
    if (off[i + 1] < off[i]) { snprintf(msg, sizeof(msg), "%s: %s[%d] = %d is below %s[%d] = %d", what, name, i + 1, off[i + 1], name, i, off[i]); return cfear_fail(ctx, CFEAR_ERR_INVALID, msg); }
  return CFEAR_OK;
}

std::vector<double> sc_table(const cfear_sc_params& P) {
  std::vector<double> t((size_t)P.n_rings + 1 + 2 * (size_t)P.n_sectors);
  make_layout(P.n_rings, P.n_sectors, P.max_range, t.data(), t.data() + P.n_rings + 1);
  return t;
}

// the describe launch of n clouds on the context stream (jobs and table already on their way on that stream)
hipError_t sc_launch_describe(cfear_ctx* ctx, const cfear_sc_params& P, const float* d_points, const ScJob* d_jobs, const double* d_table, int n, uint32_t* d_bins,
                              uint32_t* d_ring, int* d_dropped) {
  if (n < 1) return hipSuccess;
  hipLaunchKernelGGL(sc_describe_kernel, dim3(n), dim3(BLOCK_SC), 0, ctx->stream, d_points, d_jobs, d_table, P.n_rings, P.n_sectors, P.value, d_bins, d_ring, d_dropped);
  return hipGetLastError();
}

// the waves of a match workgroup: as many of 4, 2, 1 as 64 KB of LDS hold
int sc_match_waves(const cfear_sc_params& P, int stride) {
  for (int w = 4; w > 1; w >>= 1)
    if (sc_lds(P.n_rings, P.n_sectors, stride, P.max_per_node, w).total <= 65536) return w;
  return 1;
}

// the match launch over N descriptors in n_sets sets (offsets on the device) into slots / counts
hipError_t sc_launch_match(cfear_ctx* ctx, const cfear_sc_params& P, int n_sets, const int* d_set_off, int N, const uint32_t* d_bins, const uint32_t* d_ring, ScTop* d_slots,
                           int* d_counts) {
  if (N < 1) return hipSuccess;
  ScMatchArgs A;
  A.bins = d_bins; A.ring_sums = d_ring; A.set_off = d_set_off; A.slots = d_slots; A.counts = d_counts;
  A.n_sets = n_sets; A.nr = P.n_rings; A.ns = P.n_sectors; A.stride = P.n_rings | 1;
  A.gap = P.min_index_gap; A.n_keys = P.n_keys; A.mp = P.max_per_node; A.waves = sc_match_waves(P, A.stride);
  A.max_distance = P.max_distance;
  const size_t lds = sc_lds(A.nr, A.ns, A.stride, A.mp, A.waves).total;
  hipLaunchKernelGGL(sc_match_kernel, dim3(N), dim3(64 * A.waves), lds, ctx->stream, A);
  return hipGetLastError();
}

// slots and counts of N descriptors -> the records, (set, to, distance) ascending. *n: how many; more than capacity: CFEAR_ERR_CAPACITY, nothing written
int sc_compact(cfear_ctx* ctx, const char* what, const cfear_sc_params& P, int n_sets, const int32_t* set_off, const ScTop* slots, const int* counts,
               cfear_sc_candidate* candidates, int capacity, int* n) {
  const int N = set_off[n_sets];
  long long total = 0;
  for (int g = 0; g < N; g++) total += counts[g];
  if (n) *n = (int)std::min<long long>(total, 2147483647LL);
  if (total > capacity) {
    char msg[200];
    snprintf(msg, sizeof(msg), "%s: %lld candidates, capacity %d", what, total, capacity);
    return cfear_fail(ctx, CFEAR_ERR_CAPACITY, msg);
  }
  size_t k = 0;
  for (int q = 0; q < n_sets; q++)
    for (int g = set_off[q]; g < set_off[q + 1]; g++)
      for (int i = 0; i < counts[g]; i++) {
        const ScTop& e = slots[(size_t)g * P.max_per_node + i];
        cfear_sc_candidate& c = candidates[k++];
        c.sequence = q; c.to = g - set_off[q]; c.from = e.from; c.shift = e.shift;
        c.distance = (double)e.d; c.yaw = shift_yaw(e.shift, P.n_sectors); c.key_distance = e.K;
      }
  return CFEAR_OK;
}

// The start of the two log routes: the log has the clouds asked for, the streams are drained; the recorded counts per sequence and the
// describe jobs of every recorded keyframe (sequence-major) come back. A cloud above the limit is refused by name.
int sc_log_jobs(cfear_ctx* ctx, cfear_odometry* o, const char* what, const cfear_sc_params& P, std::vector<int32_t>& seq_off, std::vector<ScJob>& jobs) {
  char msg[256];
  if (!o->kf.what) { snprintf(msg, sizeof(msg), "%s: keyframe recording is off (cfear_odometry_set_keyframe_recording)", what); return cfear_fail(ctx, CFEAR_ERR_INVALID, msg); }
  if (!o->kf.records_clouds()) {
    snprintf(msg, sizeof(msg), "%s: the log was switched on without CFEAR_KF_CLOUD (cfear_odometry_set_keyframe_clouds)", what);
    return cfear_fail(ctx, CFEAR_ERR_INVALID, msg);
  }
  if (P.source == 1 && !o->kf.records_peaks()) {
    snprintf(msg, sizeof(msg), "%s: params.source = 1 (the peaks cloud) and the log was switched on without CFEAR_KF_PEAKS", what);
    return cfear_fail(ctx, CFEAR_ERR_INVALID, msg);
  }
  CFEAR_TRY(odo_drain(ctx, o));
  const KfLog L = o->kf.view();
  const int B = o->B;
  std::vector<int> counts(4 * (size_t)B);
  CFEAR_HIP_CHECK(ctx, hipMemcpy(counts.data(), L.counts, sizeof(int) * counts.size(), hipMemcpyDeviceToHost));
  seq_off.assign((size_t)B + 1, 0);
  for (int q = 0; q < B; q++) seq_off[(size_t)q + 1] = seq_off[(size_t)q] + counts[4 * (size_t)q];
  jobs.resize((size_t)seq_off[(size_t)B]);
  std::vector<int> po;
  for (int q = 0; q < B; q++) {
    const int m = counts[4 * (size_t)q];
    if (m < 1) continue;
    po.resize(3 * (size_t)m);
    CFEAR_HIP_CHECK(ctx, hipMemcpy(po.data(), L.point_off + 3 * (size_t)q * L.max_kf, sizeof(int) * 3 * (size_t)m, hipMemcpyDeviceToHost));
    for (int i = 0; i < m; i++) {
      ScJob& J = jobs[(size_t)seq_off[(size_t)q] + i];
      const int* p3 = po.data() + 3 * (size_t)i;
      J.first = (unsigned long long)q * L.max_points + p3[0] + (P.source ? p3[1] : 0);
      J.n = P.source ? p3[2] : p3[1];
      J.pad_ = 0;
      if (J.n > MAX_POINTS) {
        snprintf(msg, sizeof(msg), "%s: keyframe %d of sequence %d has a cloud of %d points, at most %d are described", what, i, q, J.n, MAX_POINTS);
        return cfear_fail(ctx, CFEAR_ERR_INVALID, msg);
      }
    }
  }
  return CFEAR_OK;
}

}  // namespace

extern "C" {

void cfear_sc_default_params(cfear_sc_params* params) {
  if (params) sc_defaults(params);
}

int cfear_scan_context_layout(const cfear_sc_params* params, double* ring_edge2, double* sector_dir) {
  if (!params || !ring_edge2 || !sector_dir) return CFEAR_ERR_INVALID;
  char text[160];
  if (sc_param_fault(*params, text, sizeof(text))) return CFEAR_ERR_INVALID;
  make_layout(params->n_rings, params->n_sectors, params->max_range, ring_edge2, sector_dir);
  return CFEAR_OK;
}

int cfear_scan_context_describe(cfear_ctx* ctx, const cfear_sc_params* params, const float* xyi, const int32_t* point_offsets, int n_clouds, uint32_t* bins,
                                uint32_t* ring_sums, int32_t* dropped) {
  const char* what = "scan_context_describe";
  if (!ctx || n_clouds < 0 || !point_offsets || (n_clouds > 0 && !bins)) return cfear_fail(ctx, CFEAR_ERR_INVALID, "scan_context_describe: bad argument");
  cfear_sc_params P;
  CFEAR_TRY(sc_params(ctx, what, params, &P));
  CFEAR_TRY(sc_check_offsets(ctx, what, "point_offsets", point_offsets, n_clouds));
  const size_t total = (size_t)point_offsets[n_clouds];
  if (total > 0 && !xyi) return cfear_fail(ctx, CFEAR_ERR_INVALID, "scan_context_describe: bad argument");
  std::vector<ScJob> jobs((size_t)n_clouds);
  for (int c = 0; c < n_clouds; c++) {
    const int np = point_offsets[c + 1] - point_offsets[c];
    if (np > MAX_POINTS) {
      char msg[200];
      snprintf(msg, sizeof(msg), "%s: cloud %d has %d points, at most %d are described", what, c, np, MAX_POINTS);
      return cfear_fail(ctx, CFEAR_ERR_INVALID, msg);
    }
    jobs[(size_t)c].first = (unsigned long long)point_offsets[c]; jobs[(size_t)c].n = np; jobs[(size_t)c].pad_ = 0;
  }
  if (n_clouds == 0) return CFEAR_OK;
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const std::vector<double> table = sc_table(P);
  const size_t nb = (size_t)P.n_rings * P.n_sectors, N = (size_t)n_clouds;
  // one block of the pool: points | jobs | table | bins | ring sums | dropped
  size_t o = 0;
  const auto take = [&](size_t bytes) { const size_t at = o; o = align_up(o + bytes, 256); return at; };
  const size_t pts_o = take(sizeof(float) * 3 * total), jobs_o = take(sizeof(ScJob) * N), tab_o = take(sizeof(double) * table.size());
  const size_t bins_o = take(sizeof(uint32_t) * nb * N), ring_o = take(sizeof(uint32_t) * P.n_rings * N), drop_o = take(sizeof(int) * N);
  void* work = nullptr;
  size_t work_bytes = 0;
  CFEAR_TRY(cfear_pool_alloc(ctx, o, &work, &work_bytes));
  unsigned char* wb = static_cast<unsigned char*>(work);
  std::vector<uint32_t> hb(nb * N), hr((size_t)P.n_rings * N);  // (the caller's arrays stay untouched unless the whole call succeeds)
  std::vector<int> hd(N);
  hipStream_t st = ctx->stream;
  hipError_t e = total ? hipMemcpyAsync(wb + pts_o, xyi, sizeof(float) * 3 * total, hipMemcpyHostToDevice, st) : hipSuccess;
  if (e == hipSuccess) e = hipMemcpyAsync(wb + jobs_o, jobs.data(), sizeof(ScJob) * N, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(wb + tab_o, table.data(), sizeof(double) * table.size(), hipMemcpyHostToDevice, st);
  if (e == hipSuccess)
    e = sc_launch_describe(ctx, P, reinterpret_cast<const float*>(wb + pts_o), reinterpret_cast<const ScJob*>(wb + jobs_o), reinterpret_cast<const double*>(wb + tab_o),
                           n_clouds, reinterpret_cast<uint32_t*>(wb + bins_o), reinterpret_cast<uint32_t*>(wb + ring_o), reinterpret_cast<int*>(wb + drop_o));
  if (e == hipSuccess) e = hipMemcpyAsync(hb.data(), wb + bins_o, sizeof(uint32_t) * hb.size(), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(hr.data(), wb + ring_o, sizeof(uint32_t) * hr.size(), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(hd.data(), wb + drop_o, sizeof(int) * N, hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);  // (the host tables are read, and the block is in use, until here)
  if (e == hipSuccess) e = es;
  cfear_pool_free(ctx, work, work_bytes);
  if (e != hipSuccess) return cfear_fail(ctx, CFEAR_ERR_HIP, what, e);
  memcpy(bins, hb.data(), sizeof(uint32_t) * hb.size());
  if (ring_sums) memcpy(ring_sums, hr.data(), sizeof(uint32_t) * hr.size());
  if (dropped) memcpy(dropped, hd.data(), sizeof(int) * N);
  return CFEAR_OK;
}

int cfear_scan_context_match(cfear_ctx* ctx, const cfear_sc_params* params, int n_sets, const int32_t* set_offsets, const uint32_t* bins, cfear_sc_candidate* candidates,
                             int capacity, int* n) {
  const char* what = "scan_context_match";
  if (!ctx || n_sets < 0 || !set_offsets || capacity < 0 || (capacity > 0 && !candidates)) return cfear_fail(ctx, CFEAR_ERR_INVALID, "scan_context_match: bad argument");
  cfear_sc_params P;
  CFEAR_TRY(sc_params(ctx, what, params, &P));
  CFEAR_TRY(sc_check_offsets(ctx, what, "set_offsets", set_offsets, n_sets));
  const size_t N = (size_t)set_offsets[n_sets];
  if (N > 0 && !bins) return cfear_fail(ctx, CFEAR_ERR_INVALID, "scan_context_match: bad argument");
  if (N == 0) {
    if (n) *n = 0;
    return CFEAR_OK;
  }
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const size_t nb = (size_t)P.n_rings * P.n_sectors;
  // one block of the pool: set offsets | bins | ring sums | slots | counts
  size_t o = 0;
  const auto take = [&](size_t bytes) { const size_t at = o; o = align_up(o + bytes, 256); return at; };
  const size_t off_o = take(sizeof(int) * ((size_t)n_sets + 1)), bins_o = take(sizeof(uint32_t) * nb * N), ring_o = take(sizeof(uint32_t) * P.n_rings * N);
  const size_t slots_o = take(sizeof(ScTop) * P.max_per_node * N), cnt_o = take(sizeof(int) * N);
  void* work = nullptr;
  size_t work_bytes = 0;
  CFEAR_TRY(cfear_pool_alloc(ctx, o, &work, &work_bytes));
  unsigned char* wb = static_cast<unsigned char*>(work);
  std::vector<ScTop> hs((size_t)P.max_per_node * N);
  std::vector<int> hc(N);
  hipStream_t st = ctx->stream;
  hipError_t e = hipMemcpyAsync(wb + off_o, set_offsets, sizeof(int) * ((size_t)n_sets + 1), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(wb + bins_o, bins, sizeof(uint32_t) * nb * N, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    const long long total = (long long)N * P.n_rings;
    hipLaunchKernelGGL(sc_ring_sums_kernel, dim3((unsigned)((total + BLOCK_SC - 1) / BLOCK_SC)), dim3(BLOCK_SC), 0, st, reinterpret_cast<const uint32_t*>(wb + bins_o), total,
                       P.n_rings, P.n_sectors, reinterpret_cast<uint32_t*>(wb + ring_o));
    e = hipGetLastError();
  }
  if (e == hipSuccess)
    e = sc_launch_match(ctx, P, n_sets, reinterpret_cast<const int*>(wb + off_o), (int)N, reinterpret_cast<const uint32_t*>(wb + bins_o),
                        reinterpret_cast<const uint32_t*>(wb + ring_o), reinterpret_cast<ScTop*>(wb + slots_o), reinterpret_cast<int*>(wb + cnt_o));
  if (e == hipSuccess) e = hipMemcpyAsync(hs.data(), wb + slots_o, sizeof(ScTop) * hs.size(), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(hc.data(), wb + cnt_o, sizeof(int) * N, hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  cfear_pool_free(ctx, work, work_bytes);
  if (e != hipSuccess) return cfear_fail(ctx, CFEAR_ERR_HIP, what, e);
  return sc_compact(ctx, what, P, n_sets, set_offsets, hs.data(), hc.data(), candidates, capacity, n);
}

int cfear_odometry_keyframe_descriptors(cfear_ctx* ctx, cfear_odometry* o, const cfear_sc_params* params, int sequence, int first, uint32_t* bins, uint32_t* ring_sums,
                                        int capacity, int* n) {
  const char* what = "odometry_keyframe_descriptors";
  if (!ctx || !o || first < 0 || capacity < 0) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_keyframe_descriptors: bad argument");
  if (sequence < 0 || sequence >= o->B) {
    char msg[160];
    snprintf(msg, sizeof(msg), "%s: sequence %d of %d", what, sequence, o->B);
    return cfear_fail(ctx, CFEAR_ERR_INVALID, msg);
  }
  cfear_sc_params P;
  CFEAR_TRY(sc_params(ctx, what, params, &P));
  std::vector<int32_t> seq_off;
  std::vector<ScJob> jobs;
  CFEAR_TRY(sc_log_jobs(ctx, o, what, P, seq_off, jobs));
  const int recorded = seq_off[(size_t)sequence + 1] - seq_off[(size_t)sequence];
  if (n) *n = recorded;
  const size_t N = jobs.size();
  const int m = std::min(capacity, recorded - first);
  if (N == 0 || m <= 0) return CFEAR_OK;
  const KfLog L = o->kf.view();
  const std::vector<double> table = sc_table(P);
  const size_t nb = (size_t)P.n_rings * P.n_sectors;
  // one block of the pool: jobs | table | bins | ring sums
  size_t off = 0;
  const auto take = [&](size_t bytes) { const size_t at = off; off = align_up(off + bytes, 256); return at; };
  const size_t jobs_o = take(sizeof(ScJob) * N), tab_o = take(sizeof(double) * table.size()), bins_o = take(sizeof(uint32_t) * nb * N);
  const size_t ring_o = take(sizeof(uint32_t) * P.n_rings * N);
  void* work = nullptr;
  size_t work_bytes = 0;
  CFEAR_TRY(cfear_pool_alloc(ctx, off, &work, &work_bytes));
  unsigned char* wb = static_cast<unsigned char*>(work);
  std::vector<uint32_t> hb(bins ? nb * (size_t)m : 0), hr(ring_sums ? (size_t)P.n_rings * m : 0);
  const size_t d0 = (size_t)seq_off[(size_t)sequence] + first;
  hipStream_t st = ctx->stream;
  hipError_t e = hipMemcpyAsync(wb + jobs_o, jobs.data(), sizeof(ScJob) * N, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(wb + tab_o, table.data(), sizeof(double) * table.size(), hipMemcpyHostToDevice, st);
  if (e == hipSuccess)
    e = sc_launch_describe(ctx, P, L.points, reinterpret_cast<const ScJob*>(wb + jobs_o), reinterpret_cast<const double*>(wb + tab_o), (int)N,
                           reinterpret_cast<uint32_t*>(wb + bins_o), reinterpret_cast<uint32_t*>(wb + ring_o), nullptr);
  if (e == hipSuccess && !hb.empty()) e = hipMemcpyAsync(hb.data(), wb + bins_o + sizeof(uint32_t) * nb * d0, sizeof(uint32_t) * hb.size(), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && !hr.empty()) e = hipMemcpyAsync(hr.data(), wb + ring_o + sizeof(uint32_t) * P.n_rings * d0, sizeof(uint32_t) * hr.size(), hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  cfear_pool_free(ctx, work, work_bytes);
  if (e != hipSuccess) return cfear_fail(ctx, CFEAR_ERR_HIP, what, e);
  if (!hb.empty()) memcpy(bins, hb.data(), sizeof(uint32_t) * hb.size());
  if (!hr.empty()) memcpy(ring_sums, hr.data(), sizeof(uint32_t) * hr.size());
  return CFEAR_OK;
}

int cfear_odometry_keyframe_candidates(cfear_ctx* ctx, cfear_odometry* o, const cfear_sc_params* params, cfear_sc_candidate* candidates, int capacity, int* n) {
  const char* what = "odometry_keyframe_candidates";
  if (!ctx || !o || capacity < 0 || (capacity > 0 && !candidates)) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_keyframe_candidates: bad argument");
  cfear_sc_params P;
  CFEAR_TRY(sc_params(ctx, what, params, &P));
  std::vector<int32_t> seq_off;
  std::vector<ScJob> jobs;
  CFEAR_TRY(sc_log_jobs(ctx, o, what, P, seq_off, jobs));
  const size_t N = jobs.size();
  if (N == 0) {
    if (n) *n = 0;
    return CFEAR_OK;
  }
  const KfLog L = o->kf.view();
  const int B = o->B;
  const std::vector<double> table = sc_table(P);
  const size_t nb = (size_t)P.n_rings * P.n_sectors;
  // one block of the pool: jobs | table | sequence offsets | bins | ring sums | slots | counts
  size_t off = 0;
  const auto take = [&](size_t bytes) { const size_t at = off; off = align_up(off + bytes, 256); return at; };
  const size_t jobs_o = take(sizeof(ScJob) * N), tab_o = take(sizeof(double) * table.size()), off_o = take(sizeof(int) * ((size_t)B + 1));
  const size_t bins_o = take(sizeof(uint32_t) * nb * N), ring_o = take(sizeof(uint32_t) * P.n_rings * N);
  const size_t slots_o = take(sizeof(ScTop) * P.max_per_node * N), cnt_o = take(sizeof(int) * N);
  void* work = nullptr;
  size_t work_bytes = 0;
  CFEAR_TRY(cfear_pool_alloc(ctx, off, &work, &work_bytes));
  unsigned char* wb = static_cast<unsigned char*>(work);
  std::vector<ScTop> hs((size_t)P.max_per_node * N);
  std::vector<int> hc(N);
  hipStream_t st = ctx->stream;
  hipError_t e = hipMemcpyAsync(wb + jobs_o, jobs.data(), sizeof(ScJob) * N, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(wb + tab_o, table.data(), sizeof(double) * table.size(), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(wb + off_o, seq_off.data(), sizeof(int) * ((size_t)B + 1), hipMemcpyHostToDevice, st);
  if (e == hipSuccess)
    e = sc_launch_describe(ctx, P, L.points, reinterpret_cast<const ScJob*>(wb + jobs_o), reinterpret_cast<const double*>(wb + tab_o), (int)N,
                           reinterpret_cast<uint32_t*>(wb + bins_o), reinterpret_cast<uint32_t*>(wb + ring_o), nullptr);
  if (e == hipSuccess)
    e = sc_launch_match(ctx, P, B, reinterpret_cast<const int*>(wb + off_o), (int)N, reinterpret_cast<const uint32_t*>(wb + bins_o),
                        reinterpret_cast<const uint32_t*>(wb + ring_o), reinterpret_cast<ScTop*>(wb + slots_o), reinterpret_cast<int*>(wb + cnt_o));
  if (e == hipSuccess) e = hipMemcpyAsync(hs.data(), wb + slots_o, sizeof(ScTop) * hs.size(), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(hc.data(), wb + cnt_o, sizeof(int) * N, hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  cfear_pool_free(ctx, work, work_bytes);
  if (e != hipSuccess) return cfear_fail(ctx, CFEAR_ERR_HIP, what, e);
  return sc_compact(ctx, what, P, B, seq_off.data(), hs.data(), hc.data(), candidates, capacity, n);
}

}  // extern "C"
