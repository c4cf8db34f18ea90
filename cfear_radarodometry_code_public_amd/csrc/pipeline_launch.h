// pipeline_launch.h -- the per-call kernels of pipeline.hip as typed launch functions, for the two kernel-free units that run them:
// percall.hip (clouds, scans, Register, GetCost, GetSurface, the cost-sampling covariance) and odometry_cov.hip (the surfaces of a batched
// object). Each enqueues its kernel(s) on `st` and nothing else: no context, no copies, no synchronisation; the caller reads
// hipGetLastError(). A kernel is launched only by the unit that defines it (a unit is one optimisation domain).
#pragma once
#include "common.h"
#include "odometry_step_dev.h"
#include "surface_dev.h"

// the filter's slots -> the filtered cloud c0 and, with c1, the peaks cloud (radar_driver.cpp:59-60); each with its host mirror where it has one
__attribute__((visibility("hidden"))) void cfear_launch_cloud(const uint32_t* d_slots, int A, int k, const double* d_trig, float range_res, float min_distance,
                                                             cfear_cloud* c0, cfear_cloud* c1 /* null: no peaks cloud */, hipStream_t st);
// Compensate (utils.cpp:96-113) of c0 and, with c1, of a second cloud by the same motion (x, y, theta)
__attribute__((visibility("hidden"))) void cfear_launch_compensate(cfear_cloud* c0, cfear_cloud* c1 /* null: one cloud */, double m0, double m1, double m2, int ccw,
                                                                  hipStream_t st);
// MapPointNormal of a cloud on the device into the blank scan d_scan ...
__attribute__((visibility("hidden"))) void cfear_launch_features(ScanDev* d_scan, const float* d_xyi, const int* d_n, const FeatureParams& P, const BlockScratch& B,
                                                                hipStream_t st);
// ... and from the n cells already in d_scan->cells
__attribute__((visibility("hidden"))) void cfear_launch_scan_from_cells(ScanDev* d_scan, int n, const FeatureParams& P, const BlockScratch& B, hipStream_t st);
// GetClosestIdx of nq queries under tie rule `rule`
__attribute__((visibility("hidden"))) void cfear_launch_closest(const ScanDev* d_scan, const double* d_q, int nq, double d, int* d_idx, int rule, hipStream_t st);
// RegisterTimeContinuous: the prologue writes the view of `src` (the last scan, `cells` cells or its capacity) compensated by the sweep
// velocity behind `hdr`, which then takes the last scan's place in the registration
struct TcLaunch { const ScanDev* src; ScanDev* hdr; double* view; int view_cells, cells; double vx, vy, vth; int ccw; };
// Register of n scans; with tc the time-continuous one (a prologue that fails to launch leaves its error for the caller and launches no more)
__attribute__((visibility("hidden"))) void cfear_launch_register(ScanDev* const* d_scans, int n, double* d_poses, double* d_cov6, const RegParams& P, const BlockScratch& B,
                                                                cfear_reg_summary* d_out, const double* d_prior_cov6, const TcLaunch* tc, hipStream_t st);
// GetCost of one problem: score, the first `cap` residuals and their number
__attribute__((visibility("hidden"))) void cfear_launch_get_cost(ScanDev* const* d_scans, int n, const double* d_poses, const RegParams& P, const BlockScratch& B, int itr,
                                                                double* d_score, double* d_residuals, int cap, int* d_nres, hipStream_t st);
// ... of m candidate poses of the last scan, one workgroup each with match arrays of `cap` pairs at d_match / d_assoc
__attribute__((visibility("hidden"))) void cfear_launch_get_cost_samples(ScanDev* const* d_scans, int n, const double* d_poses, const double* d_samples, int m,
                                                                        const RegParams& P, double* d_match, int* d_assoc, int cap, int itr, double* d_costs,
                                                                        int* d_nres, hipStream_t st);
// the build stage of one surface problem (cfear_get_surface) ...
__attribute__((visibility("hidden"))) void cfear_launch_surface_build(ScanDev* const* d_scans, int n, const double* d_poses, const RegParams& P, const BlockScratch& B, int itr,
                                                                     const double* d_prior_cov6, SurfHdr* d_hdr, const double* d_coords, const int* d_nxy, int pixels,
                                                                     double* d_out, hipStream_t st);
// ... and of every sequence of a batched object around its last registration (cfear_odometry_surface): B problems from OP.cs.ctx
__attribute__((visibility("hidden"))) void cfear_launch_surface_build_step(const OdoParams& OP, int B, const BlockScratch* d_scratch, SurfHdr* d_hdr, const double* d_coords,
                                                                          const int* d_nxy, int pixels, double* d_out, hipStream_t st);
// does the build stage evaluate the pixels itself (the A/B build CFEAR_SURFACE_NAIVE of this unit)? Then no evaluation follows it: the
// switch is read where the kernels are compiled, so a variant build of pipeline.hip alone (tools/build_variant.sh) stays consistent
__attribute__((visibility("hidden"))) bool cfear_surface_build_evaluates();
// the evaluation of `problems` surfaces under P.cost
__attribute__((visibility("hidden"))) void launch_surface_eval(const RegParams& P, int problems, const SurfHdr* d_hdr, const double* d_coords, const int* d_nxy, int pixels,
                                                              double* d_out, hipStream_t st);
