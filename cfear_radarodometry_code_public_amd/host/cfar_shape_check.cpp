// cfar_shape_check: prints the launch plan of the CA-CFAR detector (csrc/cfar_shape.h, the arithmetic the launcher and cfear_cfar_launch_plan
// share) for every group of arguments  R window guard rate compute_units  (one group may leave compute_units out: 256), as one line
//   kernel <owner|fast16|fast32|general> TB NW RS FULL sh kopen rmin rmax cr0 cr1 cr2 cr3 cq0 cq1 cq2 cq3 padl fill lds_bytes per_cu workgroups
// (workgroups: of a batch with more rows than the device holds workgroups.) With the arguments "reach" and  TB : per (guard 0 .. 64, window 1 .. 1000) one line "guard window rmin rmax" of the row offsets for TB bins
// per thread. Needs no GPU and no library: tests/test_cfar_shape_cpu.py pins the documented plans and the reach of the GPU tests' case tables with it.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../csrc/cfar_shape.h"

int main(int argc, char** argv) {
  if (argc == 3 && strcmp(argv[1], "reach") == 0) {
    const int TB = atoi(argv[2]);
    if (TB < 4 || TB > 32) return 2;
    for (int g = 0; g <= 64; g++)
      for (int w = 1; w <= 1000; w++) {
        const CfarOwnerOffsets O = cfear_cfar_owner_offsets(g, w, TB);
        printf("%d %d %d %d\n", g, w, O.rmin, O.rmax);
      }
    return 0;
  }
  if (argc < 5 || ((argc - 1) % 5 != 0 && argc != 5)) {
    fprintf(stderr, "usage: %s R window guard rate [compute_units] [...]  |  %s reach TB\n", argv[0], argv[0]);
    return 2;
  }
  static const char* names[4] = {"owner", "fast16", "fast32", "general"};
  for (int i = 1; i + 3 < argc; i += 5) {
    const int cus = i + 4 < argc ? atoi(argv[i + 4]) : 256;
    const cfear_cfar_plan p = cfear_cfar_plan_of(atoi(argv[i]), atoi(argv[i + 1]), atoi(argv[i + 2]), (float)atof(argv[i + 3]), true, cus, (size_t)1 << 30);
    printf("kernel %s %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", names[p.kernel], p.TB, p.NW, p.RS, p.full, p.sh, p.kopen, p.rmin, p.rmax,
           p.cr[0], p.cr[1], p.cr[2], p.cr[3], p.cq[0], p.cq[1], p.cq[2], p.cq[3], p.padl, p.fill, p.lds_bytes, p.per_cu, p.workgroups);
  }
  return 0;
}
