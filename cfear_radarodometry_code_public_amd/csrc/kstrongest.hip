// kstrongest.hip -- K1/K2: batched k-strongest filter + axial non-max suppression for gfx950.
//
// Replaces StructuredKStrongest::FilterKstrongest (radar_filters.cpp:209-237) and
// AxialNonMaxSupress (radar_filters.cpp:238-298) for n_scans x A azimuth rows of R uint8 bins.
//
// Mapping: one 64-lane wavefront owns one azimuth row (persistent wave loop over rows). The row is
// streamed from HBM as aligned 16-byte chunks, chunk c = j*64 + lane, i.e. every load instruction of
// the wave covers 1 KiB contiguous. The chunks stay in VGPRs for the selection and are also staged
// in a wave-private LDS window (row + 6-byte halo either side) for the byte lookups of the
// compaction and of the 13-tap non-max-suppression window.
//
// Selection (bit-exact with the reference's bounded sorted insert): the result is the k largest
// keys (intensity, range) among bytes >= z_min. Instead of sorting, the wave
//   1. probes the previous azimuth's threshold T (a wave walks consecutive rows); if that yields fewer than k
//      candidates it bounds the k-th largest intensity from below by the k-th largest per-lane maximum,
//   2. counts bytes >= T with SWAR compares (4 bytes / 5 VALU ops) and narrows T by bisection
//      until k <= count <= 64 (usually the first probe),
//   3. gives every candidate a lane without a per-candidate loop (prefix sums, owner scatter + DPP max-scan,
//      popcount split + byte table), ranks the keys with LDS broadcast reads (the key includes the range, so
//      ties go to the larger range bin exactly like std::pair<uchar,int> ordering) and
//   4. handles rows with > 64 ties at the threshold intensity by a backwards positional scan.
// No block-level barrier is used: the four waves of a block are independent.
#include "common.h"
#include "kstrongest_shape.h"

// tools/build_k1_stop_variants.sh: profile builds whose row loop ends after phase n (1 load + LDS staging, 2 threshold search and
// candidate masks, 3 candidates to lanes, 4 ranking; 0 = the product kernel); PMC counters of successive variants difference into
// per-phase instruction counts (tools/pmc_k1_phases.sh). What a stopped row stores depends on the phase's results, so nothing of
// the phase is optimised away.
#ifndef CFEAR_K1_STOP
#define CFEAR_K1_STOP 0
#endif
#define K1_STOP_AT(n, val)                                                           \
  if (CFEAR_K1_STOP == (n)) {                                                        \
    if (lane < k) slots[g * (long long)k + lane] = (uint32_t)(val);                  \
    wave_lds_fence();                                                                \
    continue;                                                                        \
  }

namespace {

constexpr uint32_t HI = 0x80808080u;

__device__ __forceinline__ int lane_id() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// wave64 inclusive prefix sum with DPP adds (Hillis-Steele inside the 16-lane rows, then two row broadcasts)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_add_i(int v) {
  return v + __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xF, false);  // lanes without a source add 0
}
__device__ __forceinline__ int wave_inclusive_scan(int v) {
  v = dpp_add_i<0x111, 0xF>(v);  // row_shr:1
  v = dpp_add_i<0x112, 0xF>(v);  // row_shr:2
  v = dpp_add_i<0x114, 0xF>(v);  // row_shr:4
  v = dpp_add_i<0x118, 0xF>(v);  // row_shr:8
  v = dpp_add_i<0x142, 0xA>(v);  // row_bcast15 -> rows 1, 3
  v = dpp_add_i<0x143, 0xC>(v);  // row_bcast31 -> rows 2, 3
  return v;
}

// same shape with max (values >= 0): lane i gets the maximum over lanes 0..i
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_max_i(int v) {
  const int o = __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xF, false);
  return o > v ? o : v;
}
__device__ __forceinline__ int wave_inclusive_max(int v) {
  v = dpp_max_i<0x111, 0xF>(v);
  v = dpp_max_i<0x112, 0xF>(v);
  v = dpp_max_i<0x114, 0xF>(v);
  v = dpp_max_i<0x118, 0xF>(v);
  v = dpp_max_i<0x142, 0xA>(v);
  v = dpp_max_i<0x143, 0xC>(v);
  return v;
}

// ... with OR: lane 63 ends up with the OR over the wave
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_or_i(int v) {
  return v | __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xF, false);
}
__device__ __forceinline__ int wave_inclusive_or(int v) {
  v = dpp_or_i<0x111, 0xF>(v);
  v = dpp_or_i<0x112, 0xF>(v);
  v = dpp_or_i<0x114, 0xF>(v);
  v = dpp_or_i<0x118, 0xF>(v);
  v = dpp_or_i<0x142, 0xA>(v);
  v = dpp_or_i<0x143, 0xC>(v);
  return v;
}

// wave-wide sum of a small non-negative per-lane integer: six DPP adds and a readlane (the ballot bit-slicing
// it replaces cost two VALU instructions per bit)
template <int BITS>
__device__ __forceinline__ int wave_sum_small(int v) {
  return __builtin_amdgcn_readlane(wave_inclusive_scan(v), 63);
}

__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// bytes [lo, hi) of a 16-byte chunk kept, the rest zeroed
__device__ __forceinline__ uint32_t dword_keep(int lo, int hi) {
  lo = lo < 0 ? 0 : (lo > 4 ? 4 : lo);
  hi = hi < 0 ? 0 : (hi > 4 ? 4 : hi);
  if (hi <= lo) return 0u;
  const uint32_t mh = hi == 4 ? 0xFFFFFFFFu : ((1u << (8 * hi)) - 1u);
  const uint32_t ml = lo == 0 ? 0u : ((1u << (8 * lo)) - 1u);
  return mh & ~ml;
}
__device__ __forceinline__ uint4 chunk_keep(uint4 v, int lo, int hi) {
  if (lo <= 0 && hi >= 16) return v;
  v.x &= dword_keep(lo, hi);
  v.y &= dword_keep(lo - 4, hi - 4);
  v.z &= dword_keep(lo - 8, hi - 8);
  v.w &= dword_keep(lo - 12, hi - 12);
  return v;
}

// per-byte (x >= T) in bit 7 of every byte (the other bits are not cleared); brep = (T & 0x7f) replicated, THIGH = (T >= 128)
template <bool THIGH>
__device__ __forceinline__ uint32_t ge_bit7(uint32_t x, uint32_t brep) {
  const uint32_t d = (x | HI) - brep;
  return THIGH ? (x & d) : (x | d);
}
__device__ __forceinline__ uint32_t bfi(uint32_t mask, uint32_t a, uint32_t b) { return (a & mask) | (b & ~mask); }  // v_bfi_b32

// Chunk candidate mask layout: bit (8*b + d) <-> byte b of dword d (byte index 4*d + b in the chunk). The four flag bits of a
// byte position are gathered with bit-field inserts (bit 7 from dword 3, bit 6 from dword 2 >> 1, ...: one v_bfi_b32 per dword
// instead of an AND with 0x80808080 and an OR) and moved down once.
template <int NCH, bool THIGH>
__device__ __forceinline__ void ge_masks_t(const uint4 (&v)[NCH], uint32_t brep, uint32_t (&m)[NCH]) {
#pragma unroll
  for (int j = 0; j < NCH; j++) {
    const uint32_t t0 = ge_bit7<THIGH>(v[j].x, brep), t1 = ge_bit7<THIGH>(v[j].y, brep);
    const uint32_t t2 = ge_bit7<THIGH>(v[j].z, brep), t3 = ge_bit7<THIGH>(v[j].w, brep);
    uint32_t u = bfi(0x80808080u, t3, t2 >> 1);
    u = bfi(0xC0C0C0C0u, u, t1 >> 2);
    u = bfi(0xE0E0E0E0u, u, t0 >> 3);
    m[j] = (u >> 4) & 0x0F0F0F0Fu;
  }
}
// masks of the bytes >= T (1 <= T <= 255; T == 256 -> none), restricted to the row by the validity
// masks of the first chunk group (vhead, j == 0) and of the chunk groups >= jt (vtail); returns the
// per-lane candidate count
template <int NCH>
__device__ __forceinline__ int count_mask(const uint4 (&v)[NCH], int T, uint32_t (&m)[NCH], uint32_t vhead, int jt,
                                          uint32_t vtail, uint32_t vtail2) {
  if (T >= 256) {
#pragma unroll
    for (int j = 0; j < NCH; j++) m[j] = 0;
    return 0;
  }
  const uint32_t brep = (uint32_t)(T & 0x7f) * 0x01010101u;
  if (T >= 128) ge_masks_t<NCH, true>(v, brep, m); else ge_masks_t<NCH, false>(v, brep, m);
  m[0] &= vhead;
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < NCH; j++) {
    if (j == jt) m[j] &= vtail;
    if (j == jt + 1) m[j] &= vtail2;
    if (j > jt + 1) m[j] = 0;
    cnt += __popc(m[j]);
  }
  return cnt;
}

// per-lane maximum row byte, from the registers the row is held in (the cold / cluttered-row paths). Only the first chunk group and
// the group holding the row end can have bytes outside the row; their validity flags (candidate-mask layout: bit 8b + d <-> byte b
// of dword d) are widened to byte masks - t = the flags of dword d in bit 0 of every byte, (t << 8) - t = 0xFF in every flagged
// byte - and the rest is v_pk_max_u16 on the odd bytes and on the even bytes << 8. (Until round 4 the row was read back from LDS
// and every chunk masked by byte ranges: twice the instructions.)
template <int NCH>
__device__ __forceinline__ int lane_max_byte_regs(const uint4 (&v)[NCH], uint32_t vhead, int jt, uint32_t vtail) {
  typedef unsigned short us2 __attribute__((ext_vector_type(2)));
  us2 ao = {0, 0}, ae = {0, 0};
#pragma unroll
  for (int j = 0; j < NCH; j++) {
    uint32_t w[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
    if (j == 0 || j >= jt) {  // (jt is wave-uniform)
      const uint32_t f = j > jt ? 0u : (j == jt ? vtail : vhead);  // (vtail includes vhead when the row ends in the first group)
#pragma unroll
      for (int d = 0; d < 4; d++) {
        const uint32_t t = (f >> d) & 0x01010101u;
        w[d] &= (t << 8) - t;
      }
    }
#pragma unroll
    for (int d = 0; d < 4; d++) {
      ao = __builtin_elementwise_max(ao, __builtin_bit_cast(us2, w[d]));
      ae = __builtin_elementwise_max(ae, __builtin_bit_cast(us2, w[d] << 8));
    }
  }
  const int m0 = ao.x >> 8, m1 = ao.y >> 8, m2 = ae.x >> 8, m3 = ae.y >> 8;
  const int a = m0 > m1 ? m0 : m1, b = m2 > m3 ? m2 : m3;
  return a > b ? a : b;
}

// per-lane candidate mask of all chunks: chunk j occupies the bit set {8b + d + 4*(j&1)} of word j>>1
// (b = byte in dword, d = dword in chunk), i.e. two chunks interleave into one 32-bit word.
template <int NCH>
__device__ __forceinline__ void pack_masks(const uint32_t (&m)[NCH], uint32_t (&w)[NCH / 2]) {
#pragma unroll
  for (int i = 0; i < NCH / 2; i++) w[i] = m[2 * i] | (m[2 * i + 1] << 4);
}

// candidate-mask bits (layout 8*b + d) of the chunk bytes with index in [lo_b, hi_b)
__device__ __forceinline__ uint32_t chunk_range_mask(int lo_b, int hi_b) {
  uint32_t keep = 0;
#pragma unroll
  for (int d = 0; d < 4; d++) {
    int l = lo_b - 4 * d, h = hi_b - 4 * d;
    l = l < 0 ? 0 : (l > 4 ? 4 : l);
    h = h < 0 ? 0 : (h > 4 ? 4 : h);
    const uint32_t nib = h > l ? (((1u << h) - 1u) & ~((1u << l) - 1u)) : 0u;  // bits b in [l, h)
    const uint32_t spread = (nib & 1u) | ((nib & 2u) << 7) | ((nib & 4u) << 14) | ((nib & 8u) << 21);
    keep |= spread << d;
  }
  return keep;
}

// backwards positional scan over the LDS row: position of the need-th largest range bin whose byte == val
__device__ __forceinline__ int tie_position(const uint8_t* win, int head, int R, int val, int need, int lane) {
  int acc = 0;
  for (int tb = R - 64; tb > -64; tb -= 64) {
    const int pos = tb + lane;
    const bool hit = pos >= 0 && win[head + pos] == (uint8_t)val;
    unsigned long long bb = __ballot(hit);
    const int c = __popcll(bb);
    if (acc + c >= need) {
      int want = need - acc, bit = 63;
      while (true) {
        bit = 63 - __clzll(bb);
        if (--want == 0) break;
        bb &= ~(1ull << bit);
      }
      return tb + bit;
    }
    acc += c;
  }
  return 0;
}

// PEAKS = false: the instantiation of the batched odometry routes (step, replay), whose cloud pass reads the valid bit, the range and the
// intensity of a slot and never the peak flag: the row ends at the emit, bit 25 is written 0, and what only the suppression's reads need goes
// with it - the scan masking of an image's first and last row and the 6 bytes past the row end (every other reader of the window, the
// candidate's intensity byte and tie_position, stays inside the row). Bits 0..24 are the same in both instantiations.
template <int NCH, int OCC, bool PEAKS>
__global__ __launch_bounds__(256, OCC) void kstrongest_kernel(const uint8_t* __restrict__ polar,
                                                            uint32_t* __restrict__ slots, int A, int R,
                                                            long long n_rows, int u_zmin, int k,
                                                            long long alloc_bytes, int rows_per_wave) {
  constexpr int WIN = NCH * 1024;  // LDS window bytes per wave
  constexpr int SUMBITS = NCH == 4 ? 7 : (NCH == 8 ? 8 : 9);
  __shared__ uint4 lds_win[4][NCH * 64];
  __shared__ __attribute__((aligned(16))) uint32_t lds_keys[4][64];
  __shared__ uint32_t lds_ge[20];  // lds_ge[n] = candidate-mask bits of the chunk bytes with index >= n (n = 0..16)
  __shared__ uint32_t lds_cmp[4][(1 + NCH / 2) * 64];  // per wave: slot offsets and candidate-mask words of every lane
  __shared__ uint8_t lds_nth[256 * 8];                 // lds_nth[b * 8 + r] = position of the r-th set bit of byte b
  if (threadIdx.x <= 16) lds_ge[threadIdx.x] = chunk_range_mask((int)threadIdx.x, 16);
  {
    const uint32_t b = threadIdx.x;  // 256 threads, one byte value each
    int r = 0;
    for (int p = 0; p < 8; p++)
      if ((b >> p) & 1u) lds_nth[b * 8 + r++] = (uint8_t)p;
    for (; r < 8; r++) lds_nth[b * 8 + r] = 0;
  }
  __syncthreads();  // the only block-level barrier: before the waves go their own way
  const int lane = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // scalar: keeps all per-row bookkeeping on the SALU
  uint8_t* const win = reinterpret_cast<uint8_t*>(&lds_win[wave][0]);
  uint32_t* const keys = &lds_keys[wave][0];
  uint32_t* const cmp_ex = &lds_cmp[wave][0];   // [64] first slot of every lane
  uint32_t* const cmp_w = &lds_cmp[wave][64];   // [NCH/2][64] mask words of every lane
  const long long scan_bytes = (long long)A * (long long)R;
  const int Tfloor = u_zmin > 1 ? u_zmin : 1;

  // each wave owns rows_per_wave consecutive rows: the selection threshold of one azimuth is the
  // first guess for the next one
  const long long g0 = ((long long)blockIdx.x * 4 + wave) * rows_per_wave;
  long long g1 = g0 + rows_per_wave;
  if (g1 > n_rows) g1 = n_rows;
  int Tprev = Tfloor;

  long long scan = g0 / A;
  int bearing = (int)(g0 - scan * A);
  for (long long g = g0; g < g1; g++, bearing++) {
    if (bearing == A) { bearing = 0; scan++; }
    // all addressing relative to the (16-byte aligned) kernel argument so that the loads are
    // global_load_dwordx4 with a scalar base and a 32-bit lane offset
    const long long row_off = g * (long long)R;
    const long long wstart_off = (row_off - 6) & ~15LL;     // may be -16 for the very first row
    const int head = (int)(row_off - wstart_off);           // 6..21: window offset of range bin 0
    // chunks [c_lo, c_hi) are inside the allocation and needed (row + 6-byte halo either side; without the suppression nothing past the row)
    const int c_lo = wstart_off >= 0 ? 0 : (int)((-wstart_off + 15) >> 4);
    int c_hi = (head + R + (PEAKS ? 6 : 0) + 15) >> 4;
    {
      const long long lim = (alloc_bytes - wstart_off + 15) >> 4;
      if (lim < c_hi) c_hi = (int)lim;
    }
    const bool edge_row = PEAKS && (bearing == 0 || bearing == A - 1);  // (the scan masking serves the suppression's halo reads only)
    const uint8_t* const wp = polar + wstart_off;  // wave-uniform

    // ---- load: HBM -> VGPR and LDS (PEAKS: scan-masked on the first/last row, keeps the cross-row halo; without the suppression there is no
    // halo to keep - c_hi ends at the row, edge_row is false and every row whose window starts inside the allocation takes the common path).
    // Branch-free: out-of-range chunks read a clamped (valid) address and are zeroed afterwards, so
    // the NCH loads of 1 KiB each are all in flight together.
    uint4 v[NCH];
    if (!edge_row && c_lo == 0) {
      // common case (398 of 400 azimuths): everything the window needs lies inside this scan's image. Chunks past
      // the halo (PEAKS = false: past the row end) re-read the last needed chunk (no extra HBM traffic); what they hold is never looked
      // at: the selection masks them (vhead / vtail), win[woff] and tie_position stay inside [head, head + R), and the suppression - the
      // only reader outside the row, PEAKS only - reads at most 6 bytes past it.
#pragma unroll
      for (int j = 0; j < NCH; j++) {
        const int cc = min(j * 64 + lane, c_hi - 1);
        {
          typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
          const u32x4 t = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp + (uint32_t)(16 * cc)));
          v[j] = make_uint4(t.x, t.y, t.z, t.w);
        }
      }
#pragma unroll
      for (int j = 0; j < NCH; j++) reinterpret_cast<uint4*>(win)[j * 64 + lane] = v[j];
    } else {
#pragma unroll
    for (int j = 0; j < NCH; j++) {
      const int c = j * 64 + lane;
      const int cc = min(max(c, c_lo), c_hi - 1);
      v[j] = *reinterpret_cast<const uint4*>(wp + (uint32_t)(16 * cc));
    }
#pragma unroll
    for (int j = 0; j < NCH; j++) {
      const int c = j * 64 + lane;
      if (c < c_lo || c >= c_hi) v[j] = make_uint4(0, 0, 0, 0);
      uint4 staged = v[j];
      if (edge_row) {
        // bytes outside this scan's image read as 0 (the reference's unchecked cv::Mat::at would run
        // off the buffer there, radar_filters.cpp:260)
        const long long ca = wstart_off + 16LL * c;
        const long long slo = scan * scan_bytes - ca, shi = (scan + 1) * scan_bytes - ca;
        if (slo > 0 || shi < 16) staged = chunk_keep(staged, (int)(slo > 16 ? 16 : slo), (int)(shi < 0 ? 0 : (shi > 16 ? 16 : shi)));
      }
      reinterpret_cast<uint4*>(win)[c] = staged;
    }
    }
    // validity of the chunk bytes w.r.t. the row [0, R): only the first chunk group and the group(s)
    // holding the row end can be partial
    const int jt = (head + R - 1) >> 10;  // chunk group of the last range bin
    int hb = head - 16 * lane, tb = head + R - 16 * (jt * 64 + lane);
    hb = hb < 0 ? 0 : (hb > 16 ? 16 : hb);
    tb = tb < 0 ? 0 : (tb > 16 ? 16 : tb);
    const uint32_t vhead = lds_ge[hb];
    const uint32_t vtail = (~lds_ge[tb] & 0x0F0F0F0Fu) & (jt == 0 ? vhead : 0x0F0F0F0Fu);
    const uint32_t vtail2 = 0u;  // groups after jt hold no row bytes
    wave_lds_fence();
    K1_STOP_AT(1, v[0].x ^ v[1].y ^ v[2].z ^ v[3].w ^ vhead ^ vtail);

    // ---- threshold search: first probe = previous row's threshold ----
    int lo = Tprev;
    uint32_t m[NCH];
    int cnt = wave_sum_small<SUMBITS>(count_mask<NCH>(v, lo, m, vhead, jt, vtail, vtail2));
    if (cnt < k && lo > Tfloor) {
      // too few: restart from the floor, bounded below by the k-th largest per-lane maximum
      lo = Tfloor;
      int lm = lane_max_byte_regs<NCH>(v, vhead, jt, vtail);
      if (lm < Tfloor) lm = 0;
      int tl = 0, th = 256;
      while (th - tl > 1) {
        const int mid = (tl + th) >> 1;
        if (__popcll(__ballot(lm >= mid)) >= k) tl = mid; else th = mid;
      }
      if (tl > lo) lo = tl;  // count(bytes >= tl) >= k is guaranteed
      cnt = wave_sum_small<SUMBITS>(count_mask<NCH>(v, lo, m, vhead, jt, vtail, vtail2));
    }
    if (cnt > 64 && lo < 255) {
      // far too many (a wave's first row starts from z_min; a cluttered row after a quiet one): jump to the k-th largest per-lane
      // maximum - at least k lanes hold a byte that large, so count(>= it) >= k - instead of bisecting with a full recount per
      // step (eight recounts on uniformly distributed bytes, where ~76 % of the bins pass z_min)
      int lm = lane_max_byte_regs<NCH>(v, vhead, jt, vtail);
      int tl = lo, th = 256;
      while (th - tl > 1) {
        const int mid = (tl + th) >> 1;
        if (__popcll(__ballot(lm >= mid)) >= k) tl = mid; else th = mid;
      }
      if (tl > lo) {
        lo = tl;
        cnt = wave_sum_small<SUMBITS>(count_mask<NCH>(v, lo, m, vhead, jt, vtail, vtail2));
      }
    }
    if (cnt > 64) {
      int hi = 256;
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        uint32_t mm[NCH];
        const int c2 = wave_sum_small<SUMBITS>(count_mask<NCH>(v, mid, mm, vhead, jt, vtail, vtail2));
        if (c2 >= k) {
          lo = mid; cnt = c2;
#pragma unroll
          for (int j = 0; j < NCH; j++) m[j] = mm[j];
          if (c2 <= 64) break;
        } else {
          hi = mid;
        }
      }
    }
    // next row starts from this threshold (one higher when the candidate set is getting large)
    Tprev = (cnt > 40 && lo < 255) ? lo + 1 : lo;

    // ---- ties: > 64 bytes equal to the threshold intensity, or z_min == 0 and zeros are needed ----
    if (cnt > 64) {
      uint32_t mg[NCH];
      const int c_gt = wave_sum_small<SUMBITS>(count_mask<NCH>(v, lo + 1, mg, vhead, jt, vtail, vtail2));
      const int pstar = tie_position(win, head, R, lo, k - c_gt, lane);
#pragma unroll
      for (int j = 0; j < NCH; j++) {
        const int bp = 16 * (j * 64 + lane) - head;  // range bin of byte 0 of this chunk
        const int nb = pstar - bp;                   // chunk bytes with index >= nb have range >= pstar (m is inside the row already)
        const uint32_t keep = lds_ge[nb < 0 ? 0 : (nb > 16 ? 16 : nb)];
        m[j] = mg[j] | (m[j] & ~mg[j] & keep);  // (> lo) | (== lo & range >= pstar)
      }
      cnt = k;
    } else if (u_zmin == 0 && cnt < k && R > cnt && lo == 1) {
      // z_min == 0: zero-valued bins are candidates too; take the largest ranges among them
      int need = k - cnt;
      if (need > R - cnt) need = R - cnt;
      const int pstar = tie_position(win, head, R, 0, need, lane);
#pragma unroll
      for (int j = 0; j < NCH; j++) {
        const int bp = 16 * (j * 64 + lane) - head;
        const uint32_t keep = chunk_range_mask(pstar - bp, R - bp);  // (zeros are not in m: the row end has to be cut here; rare path)
        m[j] |= (~m[j]) & 0x0F0F0F0Fu & keep;
      }
      cnt += need;
    }

    K1_STOP_AT(2, (uint32_t)cnt + (m[0] ^ m[1] ^ m[NCH - 2] ^ m[NCH - 1]));
    // ---- compaction without a per-candidate loop (strong returns cluster: a lane often holds five or more
    // candidates). Lane l's candidates take the slots ex[l] .. ex[l] + count - 1 (DPP prefix sum). The lane that
    // owns slot s finds its producer l (producers scatter their id to their first slot, a DPP max-scan spreads it),
    // fetches l's mask words from LDS and picks set bit number s - ex[l] (popcount split + byte table) ----
    const int C = cnt < 64 ? cnt : 64;
    const int kk = k < C ? k : C;  // number of emitted points
    uint32_t key = 0u;
    {
      uint32_t w[NCH / 2];
      pack_masks<NCH>(m, w);
      int c = 0;
#pragma unroll
      for (int i = 0; i < NCH / 2; i++) c += __popc(w[i]);
      const int ex = wave_inclusive_scan(c) - c;
      keys[lane] = 0u;
      cmp_ex[lane] = (uint32_t)ex;
#pragma unroll
      for (int i = 0; i < NCH / 2; i++) cmp_w[i * 64 + lane] = w[i];
      wave_lds_fence();
      if (c > 0 && ex < 64) keys[ex] = (uint32_t)(lane + 1);
      wave_lds_fence();
      const int owner = wave_inclusive_max((int)keys[lane]) - 1;
      if (lane < C) {
        const int l = owner;
        int r = lane - (int)cmp_ex[l];
        uint32_t sel = 0u;
        int wi = 0;
        bool found = false;
#pragma unroll
        for (int i = 0; i < NCH / 2; i++) {
          const uint32_t wv = cmp_w[i * 64 + l];
          const int ci = __popc(wv);
          if (!found) {
            if (r < ci) { sel = wv; wi = i; found = true; } else r -= ci;
          }
        }
        int t = 0;  // position of set bit number r of sel
        {
          const uint32_t lo16 = sel & 0xFFFFu;
          const int c16 = __popc(lo16);
          if (r >= c16) { r -= c16; t = 16; sel >>= 16; } else sel = lo16;
          const uint32_t lo8 = sel & 0xFFu;
          const int c8 = __popc(lo8);
          if (r >= c8) { r -= c8; t += 8; sel >>= 8; } else sel = lo8;
          t += lds_nth[sel * 8 + r];
        }
        const int j = 2 * wi + ((t >> 2) & 1);
        const int bi = 4 * (t & 3) + (t >> 3);  // byte index inside the chunk
        const uint32_t woff = (uint32_t)(16 * (j * 64 + l) + bi);  // window offset
        key = (woff - (uint32_t)head) | ((uint32_t)win[woff] << 16) | (1u << 24);
      }
    }
    K1_STOP_AT(3, key);
    // ---- ranks. Few candidates (C <= 2k, the usual case behind a threshold that tracks the previous azimuth): every lane counts the
    // larger keys among all C - four keys per LDS instruction (broadcast reads), a compare and an add per key; lanes >= C hold key 0,
    // so reading past C is harmless. Many candidates (a cold threshold, uniformly distributed bytes: C up to 64): two vector
    // instructions per key are the largest item of the row, so first K* = the k-th largest key by bisection on count(key >= mid) - one
    // vector compare per step, the count and the interval on the scalar unit, ending as soon as a step counts exactly k (keys are
    // distinct: the range bin is part of the key, so equal intensities are split by range exactly like std::pair<uchar, int>) -
    // then the k kept keys move to the front of the LDS array (a prefix count of the ballot) and are ranked among themselves.
    bool kept;
    int rank = 0;
    wave_lds_fence();  // every lane has fetched its slot code
    if (C > 2 * k) {  // wave-uniform
      const uint32_t k24 = key & 0xFFFFFFu;  // intensity << 16 | range (lanes >= C hold 0)
      uint32_t klo = (uint32_t)lo << 16, khi = 256u << 16;  // count(>= klo) = C > k, count(>= khi) = 0
      while (khi - klo > 1u) {
        const uint32_t mid = (klo + khi) >> 1;
        const int c = __popcll(__ballot(k24 >= mid));
        if (c >= k) { klo = mid; if (c == k) break; } else khi = mid;
      }
      kept = k24 >= klo;  // exactly k lanes (kk = k)
      const unsigned long long keptb = __ballot(kept);
      const int kpos = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(keptb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)keptb, 0u));
      if (kept) keys[kpos] = key;
      if (lane >= kk && lane < kk + 4) keys[lane] = 0u;  // the rest of the last group of four (key 0 is smaller than any kept key)
      wave_lds_fence();
      for (int j = 0; j < kk; j += 4) {
        const uint4 ka = reinterpret_cast<const uint4*>(keys)[j >> 2];
        rank += (ka.x > key) ? 1 : 0; rank += (ka.y > key) ? 1 : 0; rank += (ka.z > key) ? 1 : 0; rank += (ka.w > key) ? 1 : 0;
      }
    } else {
      keys[lane] = key;
      wave_lds_fence();
      for (int j = 0; j < C; j += 4) {
        const uint4 ka = reinterpret_cast<const uint4*>(keys)[j >> 2];
        rank += (ka.x > key) ? 1 : 0; rank += (ka.y > key) ? 1 : 0; rank += (ka.z > key) ? 1 : 0; rank += (ka.w > key) ? 1 : 0;
      }
      kept = lane < C && rank < kk;
    }
    K1_STOP_AT(4, key + (uint32_t)rank);

    // ---- axial non-max suppression (radar_filters.cpp:238-298) on the kept points ----
    uint32_t peak = 0;
    if constexpr (PEAKS) {
    const int mpos = (int)(key & 0xFFFFu);
    const bool interior = mpos >= 3 && mpos < R - 3;  // :251
    uint32_t covered = 0x7Fu;
    const bool edge_points = __ballot(kept && !interior) != 0;  // wave-uniform: a kept point within 3 bins of a row end (rare)
    if (edge_points) {
      // scores exist only where a valid kept point's +-3 window put them in the map (:253-263); everything else reads as the
      // unordered_map default 0 (:271-276). An interior point's own window covers its seven scores; a point within three bins of a
      // row end only sees what INTERIOR kept points within six bins of that end wrote: positions 3 .. 8 (and R - 9 .. R - 4). Those are
      // marked with one bit each, the marks of the wave OR-ed by six DPP steps, spread over their +-3 windows by three shift-ors
      // (E bit j <-> a score exists at bin j - 3, resp. R - 12 + j), and a lane shifts its seven bits out. (It was a loop over every kept
      // lane with seven compare-ors each, in every wave that holds an edge point: with tied intensities the kept points crowd at the
      // far end of the row - ties go to the larger range - and every row took it.)
      if (R >= 24) {
        const bool ik = kept && interior;
        int marks = (ik && mpos <= 8) ? (1 << (mpos - 3)) : 0;
        marks |= (ik && mpos >= R - 9) ? (1 << (6 + mpos - (R - 9))) : 0;
        marks = __builtin_amdgcn_readlane(wave_inclusive_or(marks), 63);
        uint32_t es = (uint32_t)marks & 0x3Fu, ee = ((uint32_t)marks >> 6) & 0x3Fu;
        es |= es << 1; es |= es << 2; es |= es << 3;  // bit b set -> bits b .. b + 6
        ee |= ee << 1; ee |= ee << 2; ee |= ee << 3;
        const uint32_t c_lo = ((es << 3) >> (mpos < 3 ? mpos : 0)) & 0x7Fu;          // bin r = mpos - 3 + t <-> bit r + 3 of es << 3
        const uint32_t c_hi = (ee >> (mpos >= R - 3 ? mpos - R + 9 : 0)) & 0x7Fu;    // <-> bit r - (R - 12) of ee
        covered = interior ? 0x7Fu : (mpos < 3 ? c_lo : c_hi);
      } else {  // a row too short for the two ends to be apart: the plain loop
        covered = 0;
        unsigned long long kb = __ballot(kept);
        while (kb) {
          const int i = __ffsll((long long)kb) - 1;
          kb &= kb - 1;
          const int mi = (int)(__builtin_amdgcn_readlane((int)key, i) & 0xFFFF);
          if (mi >= 3 && mi < R - 3) {
#pragma unroll
            for (int t = 0; t < 7; t++) {
              const int r = mpos - 3 + t;
              if (r >= mi - 3 && r <= mi + 3) covered |= 1u << t;
            }
          }
        }
      }
    }
    if (kept) {
      const int off0 = head + mpos - 6;
      int bv[13];
#pragma unroll
      for (int t = 0; t < 13; t++) {
        bv[t] = win[off0 + t];  // 0 <= off0 + t < WIN: head >= 6 and R + 27 <= WIN (PEAKS only: the one read of the 6-byte halo either side of the row)
      }
      int sm[7];  // sm[u] = sum bv[u..u+6] (7-tap box, radar_filters.cpp:258-261)
      sm[0] = ((bv[0] + bv[1]) + (bv[2] + bv[3])) + ((bv[4] + bv[5]) + bv[6]);
#pragma unroll
      for (int u = 1; u < 7; u++) sm[u] = sm[u - 1] - bv[u - 1] + bv[u + 6];
      bool largest = true;
      if (edge_points) {  // (all seven scores exist otherwise: the masking is skipped for the whole wave)
#pragma unroll
        for (int u = 0; u < 7; u++)
          if (!((covered >> u) & 1u)) sm[u] = 0;
      }
#pragma unroll
      for (int i = 1; i <= 3; i++) {
        if (sm[3 - i] > sm[3] || sm[3] < sm[3 + i]) largest = false;  // :282
      }
      peak = largest ? (1u << 25) : 0u;
    }
    }
    // ---- emit: ascending (intensity, range), unused slots 0 ----
    uint32_t* out = slots + g * (long long)k;
    if (kept) out[kk - 1 - rank] = key | peak;
    if (lane >= kk && lane < k) out[lane] = 0u;
    wave_lds_fence();
  }
}

}  // namespace

// Launch-shape knobs live in the context (cfear_tune, include/cfear_hip.h): occupancy variant and rows per wave.
static cfear_k1_shape launch_shape_of(const cfear_ctx* ctx, int n_scans) {
  return cfear_k1_launch_shape(ctx->A, ctx->R, n_scans, ctx->tune_k1_occ, ctx->tune_k1_rows);
}

int cfear_kstrongest_launch_shape(cfear_ctx* ctx, int n_scans, int* rows_per_wave, int* workgroups, int* occupancy) {
  if (!ctx) return CFEAR_ERR_INVALID;
  if (n_scans <= 0) return cfear_fail(ctx, CFEAR_ERR_INVALID, "kstrongest_launch_shape: n_scans <= 0");
  const cfear_k1_shape s = launch_shape_of(ctx, n_scans);
  if (s.nch == 0) return cfear_fail(ctx, CFEAR_ERR_UNSUPPORTED, "kstrongest: R > 16357 range bins not supported");
  if (rows_per_wave) *rows_per_wave = s.rows_per_wave;
  if (workgroups) *workgroups = (int)s.workgroups;
  if (occupancy) *occupancy = s.occupancy;
  return CFEAR_OK;
}

// peaks: whether the caller's slots carry the suppression's flag (bit 25); the context's FILTER_PEAKS knob overrides it.
template <int NCH, int OCC>
static void launch_k1(bool peaks, dim3 grid, hipStream_t stream, const uint8_t* d_polar, uint32_t* d_slots, int A, int R, long long n_rows, int u_zmin, int k,
                      long long alloc, int rows_per_wave) {
  if (peaks)
    hipLaunchKernelGGL((kstrongest_kernel<NCH, OCC, true>), grid, dim3(256), 0, stream, d_polar, d_slots, A, R, n_rows, u_zmin, k, alloc, rows_per_wave);
  else
    hipLaunchKernelGGL((kstrongest_kernel<NCH, OCC, false>), grid, dim3(256), 0, stream, d_polar, d_slots, A, R, n_rows, u_zmin, k, alloc, rows_per_wave);
}

int cfear_launch_kstrongest(cfear_ctx* ctx, const uint8_t* d_polar, int n_scans, uint32_t* d_slots, hipStream_t stream, bool peaks, int u_zmin_override) {
  const int A = ctx->A, R = ctx->R, k = ctx->par.k_strongest;
  if (!d_polar || !d_slots || n_scans <= 0) return cfear_fail(ctx, CFEAR_ERR_INVALID, "kstrongest: null buffer or n_scans <= 0");
  if (k < 1 || k > 64) return cfear_fail(ctx, CFEAR_ERR_UNSUPPORTED, "kstrongest: k_strongest must be in 1..64");
  if ((reinterpret_cast<uintptr_t>(d_polar) & 15) != 0) return cfear_fail(ctx, CFEAR_ERR_INVALID, "kstrongest: polar buffer must be 16-byte aligned");
  const long long n_rows = (long long)n_scans * A;
  const long long alloc = n_rows * R;
  // float -> int (radar_filters.cpp:198) -> uchar (:212); a batched odometry object with per-sequence z_min filters with the smallest of them
  const int u_zmin = u_zmin_override >= 0 ? u_zmin_override : (int)(uint8_t)(int)ctx->par.z_min;
  const cfear_k1_shape s = launch_shape_of(ctx, n_scans);  // (kstrongest_shape.h: occupancy variant, rows per wave, workgroups)
  const int rows_per_wave = s.rows_per_wave;
  if (ctx->tune_k1_peaks >= 0) peaks = ctx->tune_k1_peaks != 0;
  dim3 grid((unsigned)s.workgroups);
  if (s.nch == 0) return cfear_fail(ctx, CFEAR_ERR_UNSUPPORTED, "kstrongest: R > 16357 range bins not supported");
  if (s.nch == 4 && s.occupancy == 7)
    launch_k1<4, 7>(peaks, grid, stream, d_polar, d_slots, A, R, n_rows, u_zmin, k, alloc, rows_per_wave);
  else if (s.nch == 4 && s.occupancy == 5)
    launch_k1<4, 5>(peaks, grid, stream, d_polar, d_slots, A, R, n_rows, u_zmin, k, alloc, rows_per_wave);
  else if (s.nch == 4)
    launch_k1<4, 6>(peaks, grid, stream, d_polar, d_slots, A, R, n_rows, u_zmin, k, alloc, rows_per_wave);
  else if (s.nch == 8)
    launch_k1<8, 3>(peaks, grid, stream, d_polar, d_slots, A, R, n_rows, u_zmin, k, alloc, rows_per_wave);
  else
    launch_k1<16, 2>(peaks, grid, stream, d_polar, d_slots, A, R, n_rows, u_zmin, k, alloc, rows_per_wave);
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  return CFEAR_OK;
}
