// keyframe_dev.h -- the keyframe log of a batched odometry object (AddToGraph, odometrykeyframefuser.cpp:428-445; RadarScan,
// types.h:93-143; Constraint3d, types.h:155-190) as the device sees it, and the launchers of keyframes.hip that pipeline.hip calls.
#pragma once
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
  float* points;               // [B][max_points][3] x, y, intensity (+ one point of slack at the end: cfear_odometry::d_kf_points); null without CFEAR_KF_CLOUD
  int* point_off;              // [B][max_kf][3] per node: where its clouds start in the sequence's points, points of the filtered cloud, of the peaks cloud
  int* cloud_word;             // [B][4] what the cloud stage leaves for the recorder of the same sweep: 1 = the sequence fused and its clouds are
                               // written and fit (0: they do not fit, or nothing was written), points of the filtered cloud, of the peaks cloud, 0
};
// counts[q]: nodes recorded, keyframes dropped, cells used, points used

// One scan to rebuild from the log (cfear_odometry_keyframe_scans): the header of its block, its cells in the log and the working memory
// of its workgroup (the uniform grid's cursors; under NN_TIE_RULE = 2 the kd build's activation stack).
struct KfScanJob {
  ScanDev hdr;                     // written to the front of the block by the kernel (hdr's pointers point into the block)
  ScanDev* dst;                    // the block
  const cfear_keyframe_cell* src;  // n cells
  int n, part_doubles;
  int* vcur;                       // [CFEAR_GRID_CAP + 4]
  double* part;                    // [part_doubles], or null
};

}  // namespace cfear_dev

// keyframes.hip: the recorder stage of `count` sequences from seq0 on, behind the registration stage (and the cost sampling) on `st`
__attribute__((visibility("hidden"))) void cfear_launch_keyframe_record(const KfLog& L, const OdoParams& P, int count, hipStream_t st, const SeqState* states,
                                                                       const double* cov_work);
// ... in front of it on the same stream when the log keeps clouds (KfLog::points): the cloud stage. The sequences that fused write their
// filtered cloud - and with CFEAR_KF_PEAKS their peaks cloud - behind the points their log holds and leave the verdict in KfLog::cloud_word.
// slots: the sweep's filter output (read through cloud_step_block, as the feature stage read it), or null on the cloud routes, where the
// compensated cloud is copied from the scan's xyi
__attribute__((visibility("hidden"))) void cfear_launch_keyframe_clouds(const KfLog& L, const OdoParams& P, int count, hipStream_t st, const SeqState* states,
                                                                       const uint32_t* slots, const double* trig);
// ... and m scans from the log, a workgroup each
__attribute__((visibility("hidden"))) void cfear_launch_keyframe_scans(const KfScanJob* d_jobs, int m, const FeatureParams& P, hipStream_t st);
