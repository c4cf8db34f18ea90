// kstrongest_shape.h -- launch shape of the k-strongest filter (kstrongest.hip): host only, plain C++, no HIP.
// The one copy of the arithmetic: cfear_launch_kstrongest launches what this returns, cfear_kstrongest_launch_shape
// (include/cfear_hip.h) reads it back, host/filter_shape_check.cpp prints it for the CPU test of the documented shapes.
#pragma once

struct cfear_k1_shape {
  int nch;            // 16-byte chunk groups of the row window held per lane: 4, 8 or 16 (0: R + 27 > 16 KiB, no kernel)
  int occupancy;      // launch bound (workgroups per compute unit) of the kernel that runs: 7 / 6 / 5, 3 (nch 8), 2 (nch 16)
  int rows_per_wave;  // consecutive rows a wave walks
  long long workgroups;  // of 256 threads = four waves
};

// tune_occ / tune_rows: the context's CFEAR_TUNE_FILTER_OCCUPANCY / CFEAR_TUNE_FILTER_ROWS_PER_WAVE
static inline cfear_k1_shape cfear_k1_launch_shape(int A, int R, int n_scans, int tune_occ, int tune_rows) {
  cfear_k1_shape s;
  const long long n_rows = (long long)n_scans * A;
  s.nch = R + 27 <= 4 * 1024 ? 4 : (R + 27 <= 8 * 1024 ? 8 : (R + 27 <= 16 * 1024 ? 16 : 0));
  // one resident wave per SIMD slot (256 CUs x 4 SIMDs x occupancy); each wave walks consecutive rows
  const int occ_eff = s.nch == 4 ? (tune_occ >= 7 ? 7 : (tune_occ <= 5 ? 5 : 6)) : (s.nch == 8 ? 3 : 2);
  // A wave walks a few consecutive rows (the threshold of one azimuth is the first guess for the next): four rows
  // per wave measured best from 256-scan to 1024-scan launches (shorter: every row pays the cold threshold search;
  // longer: fewer, longer workgroups balance worse), six from 1536 scans up (round 3, inside the bench's timed region at 4608
  // scans: 1041 -> 1014 us, 0.754 -> 0.774 of the HBM peak; 8 and 12 the same, 16 worse at 1536). Small launches spread their
  // rows over the resident slots.
  const long long slots_total = 1024LL * occ_eff;
  int rows_per_wave = (int)((n_rows + slots_total - 1) / slots_total);
  const int rows_cap = tune_rows > 0 ? tune_rows : (n_scans >= 1536 ? 6 : 4);
  if (rows_per_wave > rows_cap) rows_per_wave = rows_cap;
  if (rows_per_wave < 1) rows_per_wave = 1;
  s.occupancy = occ_eff;
  s.rows_per_wave = rows_per_wave;
  const long long n_waves = (n_rows + rows_per_wave - 1) / rows_per_wave;
  s.workgroups = (n_waves + 3) / 4;
  return s;
}
