// cfar_grid.h -- which detections a CA-CFAR grid launch makes (cfear_filter_cfar_grid_device, cfear_odometry_set_sequence_detectors): host
// arithmetic only, shared by cfar.hip and host/cfar_grid_check (tests/test_cfar_grid_cpu.py).
//
// Cloud c is the detections of source image source[c] under the detector dets[c]. Clouds that agree in (source, window_size, nb_guard_cells,
// false_alarm_rate, z_min) are the same detection: it is made once - a PAIR - and every such cloud is emitted from its masks. The pairs are
// sorted by source (ascending set inside a source), so that the workgroup of a source row walks one segment of the list:
//   pair_begin[s] .. pair_begin[s + 1]   the pairs of source s
// and the distinct detectors - the SETS, in order of first appearance - are what the per-set route (row shapes the shared kernel does not
// take) runs the one-detector kernels over.
#pragma once
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/cfear_hip.h"

struct cfear_cfar_grid_plan {
  int n_clouds = 0, n_sources = 0;
  int max_reach = 0;                      // the largest nb_guard_cells + window_size of the sets
  std::vector<cfear_seq_detector> sets;   // the distinct detectors
  std::vector<int> pair_src, pair_set;    // [n_pairs] sorted by (source, set)
  std::vector<int> pair_begin;            // [n_sources + 1]
  std::vector<int> cloud_pair, cloud_set, cloud_src;  // [n_clouds]
  int n_sets() const { return (int)sets.size(); }
  int n_pairs() const { return (int)pair_src.size(); }
};

inline bool cfear_seq_detector_equal(const cfear_seq_detector& a, const cfear_seq_detector& b) {
  return a.window_size == b.window_size && a.nb_guard_cells == b.nb_guard_cells && memcmp(&a.false_alarm_rate, &b.false_alarm_rate, sizeof(float)) == 0 &&
         memcmp(&a.z_min, &b.z_min, sizeof(float)) == 0;
}

// source == null: cloud c reads source c (n_sources = n_clouds). false (nothing usable in G): a source outside [0, n_sources)
inline bool cfear_cfar_grid_plan_build(const cfear_seq_detector* dets, const int32_t* source, int n_clouds, int n_sources, cfear_cfar_grid_plan& G) {
  G = cfear_cfar_grid_plan();
  if (n_clouds < 1 || n_sources < 1 || (!source && n_sources != n_clouds)) return false;
  G.n_clouds = n_clouds; G.n_sources = n_sources;
  G.cloud_set.assign((size_t)n_clouds, 0); G.cloud_src.assign((size_t)n_clouds, 0); G.cloud_pair.assign((size_t)n_clouds, 0);
  for (int c = 0; c < n_clouds; c++) {
    const int s = source ? (int)source[c] : c;
    if (s < 0 || s >= n_sources) return false;
    G.cloud_src[(size_t)c] = s;
    int k = 0;
    while (k < G.n_sets() && !cfear_seq_detector_equal(G.sets[(size_t)k], dets[c])) k++;
    if (k == G.n_sets()) G.sets.push_back(dets[c]);
    G.cloud_set[(size_t)c] = k;
    G.max_reach = std::max(G.max_reach, dets[c].nb_guard_cells + dets[c].window_size);
  }
  std::vector<long long> keys((size_t)n_clouds);
  const long long ns = G.n_sets();
  for (int c = 0; c < n_clouds; c++) keys[(size_t)c] = (long long)G.cloud_src[(size_t)c] * ns + G.cloud_set[(size_t)c];
  std::vector<long long> uniq(keys);
  std::sort(uniq.begin(), uniq.end());
  uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
  G.pair_begin.assign((size_t)n_sources + 1, 0);
  for (long long k : uniq) {
    G.pair_src.push_back((int)(k / ns)); G.pair_set.push_back((int)(k % ns));
    G.pair_begin[(size_t)(k / ns) + 1]++;
  }
  for (int s = 0; s < n_sources; s++) G.pair_begin[(size_t)s + 1] += G.pair_begin[(size_t)s];
  for (int c = 0; c < n_clouds; c++) G.cloud_pair[(size_t)c] = (int)(std::lower_bound(uniq.begin(), uniq.end(), keys[(size_t)c]) - uniq.begin());
  return true;
}
