// seq_groups.h -- the registration launch groups of a batched odometry object with per-sequence shapes (cfear_odometry_set_sequence_shapes):
// host arithmetic only, shared by seq_config.h (cfear_seq_config::groups, built by odometry_seq.hip's seq_table_upload), pipeline.hip
// (launch_register_kernel, which launches by them) and host/seq_groups_check (tests/test_seq_shape_cpu.py).
//
// A sequence's group is (cost, small or not small). The batched registration kernels exist once per cost metric (the evaluation inline), and
// register_step.hip's are compiled for at most `small_scans` scans: their per-scan LDS arrays hold that many, so a registration of more
// scans in them writes past the arrays. cfear_seq_group() is the ONE place that decides which sequences may run them:
//
//   small  <=>  submap_scan_size + 1 <= small_scans     (the keyframes of the ring and the current scan)
//
// The list holds the sequences sorted by group, ascending index inside a group; each non-empty group is one launch over its segment.
#pragma once
#include <vector>

constexpr int CFEAR_SEQ_GROUPS = 6;  // three costs x (small, not small); group id = 2 * cost + (small ? 0 : 1)

inline bool cfear_seq_is_small(int submap_scan_size, int small_scans) { return submap_scan_size >= 1 && submap_scan_size + 1 <= small_scans; }
// -1: not a cost metric or not a submap size (the caller refuses the row before anything is built)
inline int cfear_seq_group(int cost, int submap_scan_size, int small_scans) {
  if (cost < 0 || cost > 2 || submap_scan_size < 1) return -1;
  return 2 * cost + (cfear_seq_is_small(submap_scan_size, small_scans) ? 0 : 1);
}

struct cfear_seq_groups {
  int n_sequences = 0;
  int offset[CFEAR_SEQ_GROUPS] = {0, 0, 0, 0, 0, 0};  // first entry of the group's segment of `list`
  int count[CFEAR_SEQ_GROUPS] = {0, 0, 0, 0, 0, 0};   // sequences of the group (0: no launch)
  int n_launches = 0;                                  // non-empty groups
  int n_large = 0, max_large_submap = 0;               // the sequences that are not small, over all costs, and the largest submap among them
  std::vector<int> list;                               // [n_sequences] the sequences sorted by group, ascending inside a group
  std::vector<int> group;                              // [n_sequences] the group of every sequence
  static int cost_of(int g) { return g >> 1; }
  static bool small_of(int g) { return (g & 1) == 0; }
};

// false (and nothing usable in G): a row whose cost / submap_scan_size is none
inline bool cfear_seq_groups_build(const int* cost, const int* submap_scan_size, int n, int small_scans, cfear_seq_groups& G) {
  G = cfear_seq_groups();
  G.n_sequences = n;
  G.group.assign((size_t)(n > 0 ? n : 0), 0);
  for (int q = 0; q < n; q++) {
    const int g = cfear_seq_group(cost[q], submap_scan_size[q], small_scans);
    if (g < 0) return false;
    G.group[(size_t)q] = g;
    G.count[g]++;
    if (!cfear_seq_groups::small_of(g)) { G.n_large++; if (submap_scan_size[q] > G.max_large_submap) G.max_large_submap = submap_scan_size[q]; }
  }
  int at = 0;
  for (int g = 0; g < CFEAR_SEQ_GROUPS; g++) { G.offset[g] = at; at += G.count[g]; if (G.count[g] > 0) G.n_launches++; }
  G.list.assign((size_t)(n > 0 ? n : 0), 0);
  int fill[CFEAR_SEQ_GROUPS] = {0, 0, 0, 0, 0, 0};
  for (int q = 0; q < n; q++) { const int g = G.group[(size_t)q]; G.list[(size_t)(G.offset[g] + fill[g]++)] = q; }
  return true;
}
