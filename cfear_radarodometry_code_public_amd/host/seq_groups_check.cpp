// seq_groups_check: prints the registration launch groups of a batched odometry object with per-sequence shapes (csrc/seq_groups.h, the
// arithmetic cfear_odometry_set_sequence_shapes builds its launches from) for the arguments  small_scans cost_0 s_0 cost_1 s_1 ...  :
//   launches <non-empty groups> large <sequences that are not small> max_large_submap <their largest submap_scan_size>
//   group <id> cost <c> small <0|1> offset <o> count <n>        for each of the six groups (count 0: no launch)
//   list <the sequences sorted by group>
// "invalid" (exit status 1) for a cost or submap_scan_size that is none. Needs no GPU and no library: tests/test_seq_shape_cpu.py drives it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../csrc/seq_groups.h"

int main(int argc, char** argv) {
  if (argc < 2 || (argc - 2) % 2 != 0) {
    fprintf(stderr, "usage: %s small_scans [cost submap_scan_size ...]\n", argv[0]);
    return 2;
  }
  const int small_scans = atoi(argv[1]);
  std::vector<int> cost, sub;
  for (int i = 2; i + 1 < argc; i += 2) { cost.push_back(atoi(argv[i])); sub.push_back(atoi(argv[i + 1])); }
  cfear_seq_groups G;
  if (!cfear_seq_groups_build(cost.data(), sub.data(), (int)cost.size(), small_scans, G)) { printf("invalid\n"); return 1; }
  printf("launches %d large %d max_large_submap %d\n", G.n_launches, G.n_large, G.max_large_submap);
  for (int g = 0; g < CFEAR_SEQ_GROUPS; g++)
    printf("group %d cost %d small %d offset %d count %d\n", g, cfear_seq_groups::cost_of(g), cfear_seq_groups::small_of(g) ? 1 : 0, G.offset[g], G.count[g]);
  printf("list");
  for (int q : G.list) printf(" %d", q);
  printf("\n");
  return 0;
}
