// cfar_grid_check: prints which detections a CA-CFAR grid launch makes (csrc/cfar_grid.h, the arithmetic cfear_filter_cfar_grid_device and
// cfear_odometry_set_sequence_detectors build their tables from) for the arguments  n_sources  source_0 window_0 guard_0 rate_0 zmin_0  source_1 ...  :
//   sets <distinct detectors> pairs <distinct (source, detector)> max_reach <largest guard + window>
//   set <k> <window> <guard> <rate> <z_min>          for every distinct detector, in order of first appearance
//   pair <p> source <s> set <k>                      for every pair, sorted by (source, set)
//   pair_begin <n_sources + 1 offsets into the pairs>
//   cloud <c> source <s> set <k> pair <p>            for every cloud
// "invalid" (exit status 1) for a source outside [0, n_sources). Needs no GPU and no library: tests/test_cfar_grid_cpu.py drives it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../csrc/cfar_grid.h"

int main(int argc, char** argv) {
  if (argc < 2 || (argc - 2) % 5 != 0) {
    fprintf(stderr, "usage: %s n_sources [source window guard rate z_min ...]\n", argv[0]);
    return 2;
  }
  const int n_sources = atoi(argv[1]);
  std::vector<cfear_seq_detector> dets;
  std::vector<int32_t> src;
  for (int i = 2; i + 4 < argc; i += 5) {
    cfear_seq_detector d;
    src.push_back(atoi(argv[i]));
    d.window_size = atoi(argv[i + 1]); d.nb_guard_cells = atoi(argv[i + 2]); d.false_alarm_rate = (float)atof(argv[i + 3]); d.z_min = (float)atof(argv[i + 4]);
    dets.push_back(d);
  }
  cfear_cfar_grid_plan G;
  if (!cfear_cfar_grid_plan_build(dets.data(), src.data(), (int)dets.size(), n_sources, G)) { printf("invalid\n"); return 1; }
  printf("sets %d pairs %d max_reach %d\n", G.n_sets(), G.n_pairs(), G.max_reach);
  for (int k = 0; k < G.n_sets(); k++)
    printf("set %d %d %d %g %g\n", k, (int)G.sets[k].window_size, (int)G.sets[k].nb_guard_cells, (double)G.sets[k].false_alarm_rate, (double)G.sets[k].z_min);
  for (int p = 0; p < G.n_pairs(); p++) printf("pair %d source %d set %d\n", p, G.pair_src[p], G.pair_set[p]);
  printf("pair_begin");
  for (int v : G.pair_begin) printf(" %d", v);
  printf("\n");
  for (int c = 0; c < G.n_clouds; c++) printf("cloud %d source %d set %d pair %d\n", c, G.cloud_src[c], G.cloud_set[c], G.cloud_pair[c]);
  return 0;
}
