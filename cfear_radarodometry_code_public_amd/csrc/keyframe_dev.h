// keyframe_dev.h -- the keyframe log of a batched odometry object (AddToGraph, odometrykeyframefuser.cpp:428-445; RadarScan,
// types.h:93-143; Constraint3d, types.h:155-190): KfLog, the log as the device sees it, KeyframeLog, its owner on the host (the member
// `kf` of cfear_odometry), and the two launchers of keyframes.hip that pipeline.hip's sweep calls. The setters and the reading routes are
// keyframes.hip's own.
#pragma once
#include "common.h"
#include "odometry_step_dev.h"

static_assert(sizeof(cfear_keyframe_node) == 376 && sizeof(cfear_keyframe_cell) == 72, "the public layouts (capi.KEYFRAME_NODE_DTYPE / KEYFRAME_CELL_DTYPE)");

namespace cfear_dev {

// The log of all sequences: sequence q owns nodes [q * max_kf, (q + 1) * max_kf), cells [q * max_cells, (q + 1) * max_cells) and its
// four counters; only q's recorder workgroup writes them.
struct KfLog {
  int what, max_kf, max_cells, pad_;
  cfear_keyframe_node* nodes;  // [B][max_kf]
  cfear_keyframe_cell* cells;  // [B][max_cells]; null without CFEAR_KF_CELLS
  int* cell_off;               // [B][max_kf] where a node's cells start in the sequence's cells
  int* counts;                 // [B][4]: nodes recorded, keyframes dropped, cells used, 0
  double* tmot;                // [B][6] SeqState::Tmot at the end of the previous sweep (l0 .. l3, t0, t1): what the feature stage of THIS sweep
                               // compensated with - the registration stage has overwritten the state's own by the time the recorder runs
  // the point log (CFEAR_KF_CLOUD; cfear_odometry_set_keyframe_clouds): cloud_nopeaks_ and cloud_peaks_ of every node (types.h:93-143), the
  // filtered cloud first, the peaks cloud right behind it. Sequence q owns points [q * max_points, (q + 1) * max_points)
  int max_points, pad2_;
  float* points;               // [B][max_points][3] x, y, intensity (+ one point of slack at the end: KeyframeLog::d_points); null without CFEAR_KF_CLOUD
  int* point_off;              // [B][max_kf][3] per node: where its clouds start in the sequence's points, points of the filtered cloud, of the peaks cloud
  int* cloud_word;             // [B][4] what the cloud stage leaves for the recorder of the same sweep: 1 = the sequence fused and its clouds are
                               // written and fit (0: they do not fit, or nothing was written), points of the filtered cloud, of the peaks cloud, 0
};
// counts[q]: nodes recorded, keyframes dropped, cells used, points used

}  // namespace cfear_dev

// The log's owner: what is recorded (`what`: CFEAR_KF_* bits, 0 = off), the capacities per sequence and the device memory. The setters of
// keyframes.hip size it; they drain the streams before a buffer goes (DevBuf: when one may go is the caller's to know).
struct __attribute__((visibility("hidden"))) KeyframeLog {
  int what = 0, max_kf = 0, max_cells = 0, max_points = 0;
  DevBuf<cfear_keyframe_node> d_nodes;  // [B][max_kf]
  DevBuf<cfear_keyframe_cell> d_cells;  // [B][max_cells] (CFEAR_KF_CELLS)
  DevBuf<int> d_cell_off;               // [B][max_kf] a node's first cell in its sequence's cells
  DevBuf<int> d_counts;                 // [B][4] nodes recorded, keyframes dropped, cells used, points used
  DevBuf<double> d_tmot;                // [B][6] the recorder's copy of SeqState::Tmot (KfLog::tmot)
  // the point log (CFEAR_KF_CLOUD / CFEAR_KF_PEAKS): the cloud stage runs in front of the recorder; with CFEAR_KF_PEAKS the object's filters
  // compute the slots' peak flag
  DevBuf<float> d_points;               // [B][max_points][3] + one point: the general cloud pass reads the point at its output's start back whatever
                                        // it wrote. With no room left that is the first point of the NEXT sequence's region (which its workgroup may be
                                        // writing) or, for the last sequence, this slack; the value lands in lanes that hold no point and is discarded
  DevBuf<int> d_point_off;              // [B][max_kf][3] per node: first point, points of the filtered cloud, of the peaks cloud
  DevBuf<int> d_cloud_word;             // [B][4] the cloud stage's verdict and counts of the sweep (KfLog::cloud_word)

  bool records_clouds() const { return (what & CFEAR_KF_CLOUD) != 0; }
  bool records_peaks() const { return (what & CFEAR_KF_PEAKS) != 0; }
  // what the kernels - and the reading routes - take
  KfLog view() const {
    KfLog L;
    L.what = what; L.max_kf = max_kf; L.max_cells = max_cells; L.pad_ = 0;
    L.nodes = d_nodes; L.cells = d_cells; L.cell_off = d_cell_off; L.counts = d_counts; L.tmot = d_tmot;
    L.max_points = max_points; L.pad2_ = 0;
    L.points = d_points; L.point_off = d_point_off; L.cloud_word = d_cloud_word;
    return L;
  }
  // an empty log of B sequences: no nodes, no drops, and the recorder's copy of Tmot the identity the states start with
  int clear(cfear_ctx* ctx, int B) {
    std::vector<double> tm(6 * (size_t)B, 0.0);
    for (int q = 0; q < B; q++) tm[6 * (size_t)q] = tm[6 * (size_t)q + 3] = 1.0;
    CFEAR_HIP_CHECK(ctx, hipMemsetAsync(d_counts, 0, sizeof(int) * 4 * (size_t)B, ctx->stream));
    if (d_cloud_word) CFEAR_HIP_CHECK(ctx, hipMemsetAsync(d_cloud_word, 0, sizeof(int) * 4 * (size_t)B, ctx->stream));  // (the point log with the rest)
    CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(d_tmot, tm.data(), sizeof(double) * tm.size(), hipMemcpyHostToDevice, ctx->stream));
    CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // (tm is read until here)
    return CFEAR_OK;
  }
  // the point log goes (no cloud stage is running) ...
  void release_points() {
    what &= ~(CFEAR_KF_CLOUD | CFEAR_KF_PEAKS);
    max_points = 0;
    d_points.release(); d_point_off.release(); d_cloud_word.release();
  }
  // ... and the whole log: recording is off (no recorder is running). The point log is sized by max_kf and goes with the nodes;
  // cfear_odometry_set_keyframe_clouds switches it on again
  void release() { *this = KeyframeLog(); }
};

// keyframes.hip: the recorder stage of `count` sequences from seq0 on, behind the registration stage (and the cost sampling) on `st`
__attribute__((visibility("hidden"))) void cfear_launch_keyframe_record(const KfLog& L, const OdoParams& P, int count, hipStream_t st, const SeqState* states,
                                                                       const double* cov_work);
// ... in front of it on the same stream when the log keeps clouds (KfLog::points): the cloud stage. The sequences that fused write their
// filtered cloud - and with CFEAR_KF_PEAKS their peaks cloud - behind the points their log holds and leave the verdict in KfLog::cloud_word.
// slots: the sweep's filter output (read through cloud_step_block, as the feature stage read it), or null on the cloud routes, where the
// compensated cloud is copied from the scan's xyi
__attribute__((visibility("hidden"))) void cfear_launch_keyframe_clouds(const KfLog& L, const OdoParams& P, int count, hipStream_t st, const SeqState* states,
                                                                       const uint32_t* slots, const double* trig);
