// filter_shape_check: prints the launch shape of the k-strongest filter (csrc/kstrongest_shape.h, the arithmetic the launcher and
// cfear_kstrongest_launch_shape share) for every group of five arguments  A R n_scans occupancy_knob rows_knob  as one line
// "rows_per_wave workgroups occupancy nch". Needs no GPU and no library: tests/test_filter_shape_cpu.py pins the documented shapes with it.
#include <cstdio>
#include <cstdlib>

#include "../csrc/kstrongest_shape.h"

int main(int argc, char** argv) {
  if (argc < 6 || (argc - 1) % 5 != 0) {
    fprintf(stderr, "usage: %s A R n_scans occupancy_knob rows_knob [...]\n", argv[0]);
    return 2;
  }
  for (int i = 1; i + 4 < argc; i += 5) {
    const cfear_k1_shape s = cfear_k1_launch_shape(atoi(argv[i]), atoi(argv[i + 1]), atoi(argv[i + 2]), atoi(argv[i + 3]), atoi(argv[i + 4]));
    printf("%d %lld %d %d\n", s.rows_per_wave, s.workgroups, s.occupancy, s.nch);
  }
  return 0;
}
