// odometry_plan_check: prints the plans of a batched odometry object (csrc/odometry_plan.h, the arithmetic cfear_odometry_create and the
// replay share) for every command on the command line, one line each:
//   masks ncu filter_cus                                                  -> "masks W f <W hex words> o <W hex words>" (W = 0: no masks)
//   chunk on_device cfar sweep_bytes slots n_sweeps have_chunk have_polar -> "chunk N"
//   caps cfar A k cfar_max_points submap max_cells tie_rule               -> "caps cap_points cap_cells pair_cap"
//   overlap tune B cfar                                                   -> "overlap N"
// Needs no GPU and no library: tests/test_odometry_plan_cpu.py pins the documented plans with it.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../csrc/odometry_plan.h"

int main(int argc, char** argv) {
  int i = 1;
  auto num = [&](int k) { return atoll(argv[i + k]); };
  while (i < argc) {
    const char* cmd = argv[i];
    const int left = argc - i - 1;
    if (strcmp(cmd, "masks") == 0 && left >= 2) {
      std::vector<uint32_t> f, o;
      cfear_cu_masks((int)num(1), (int)num(2), f, o);
      printf("masks %zu f", f.size());
      for (uint32_t w : f) printf(" %08x", w);
      printf(" o");
      for (uint32_t w : o) printf(" %08x", w);
      printf("\n");
      i += 3;
    } else if (strcmp(cmd, "chunk") == 0 && left >= 7) {
      printf("chunk %d\n", cfear_replay_chunk(num(1) != 0, num(2) != 0, (size_t)num(3), (size_t)num(4), (int)num(5), (int)num(6), (int)num(7)));
      i += 8;
    } else if (strcmp(cmd, "caps") == 0 && left >= 7) {
      const cfear_odo_caps C = cfear_odo_capacities(num(1) != 0, (int)num(2), (int)num(3), (int)num(4), (int)num(5), (int)num(6), (int)num(7));
      printf("caps %d %d %d\n", C.cap_points, C.cap_cells, C.pair_cap);
      i += 8;
    } else if (strcmp(cmd, "overlap") == 0 && left >= 3) {
      printf("overlap %d\n", cfear_odo_overlap((int)num(1), (int)num(2), num(3) != 0));
      i += 4;
    } else {
      fprintf(stderr, "usage: %s [masks ncu filter_cus | chunk on_device cfar sweep_bytes slots n_sweeps have_chunk have_polar | "
              "caps cfar A k cfar_max_points submap max_cells tie_rule | overlap tune B cfar] ...\n", argv[0]);
      return 2;
    }
  }
  return argc > 1 ? 0 : 2;
}
