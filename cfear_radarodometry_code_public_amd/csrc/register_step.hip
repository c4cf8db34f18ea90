// register_step.hip -- the batched registration step kernel as it runs in production: compiled for registrations of at most
// CFEAR_STEP_SMALL_SCANS scans (submap_scan_size <= 7: the reference's presets use 3 and 4). The per-scan arrays of the workgroup's
// shared state shrink from 64 entries to 8, and the ~10 KB of LDS that frees go to the match array: 784 residual blocks with all
// eight arrays instead of 622 (P2L, seven arrays: 896 instead of 710; P2P, five: 1254 instead of 995) at the same three workgroups
// per compute unit. A city-block scene at k = 12 builds 650-750 blocks per registration: with 710 in LDS two out of five
// registrations evaluated part of their matches from memory. pipeline.hip keeps an instantiation for larger submaps.
#define CFEAR_REG_MAX_SCANS 8
#ifndef CFEAR_MATCH_LDS_CAP  // (tools/reg_resources.sh, tools/build_variant.sh: A/B builds)
#define CFEAR_MATCH_LDS_CAP 784
#endif
#include "common.h"
#include "odometry_step_dev.h"

static_assert(CFEAR_REG_MAX_SCANS == CFEAR_STEP_SMALL_SCANS, "common.h tells pipeline.hip when to launch these kernels");

// pipeline.hip (launch_register_kernel)
void cfear_launch_register_step_small(const OdoParams& P, int count, hipStream_t st, SeqState* states, const BlockScratch* scratch, double* cov_work,
                                      cfear_reg_summary* summaries, double* poses_out) {
  CFEAR_LAUNCH_REG_BY_COST(register_step_kernel, P, count, st, states, nullptr, scratch, nullptr, cov_work, summaries, poses_out);
}
