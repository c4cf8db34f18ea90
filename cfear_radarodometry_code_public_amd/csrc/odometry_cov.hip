// odometry_cov.hip -- what a batched odometry object (odometry_obj.h) does with the records of its registrations (d_cov_ctx): the
// cost-sampling covariance of every sweep (cfear_odometry_set_cov_sampling, cfear_odometry_cov_samples) and the cost surfaces around the
// last step's registrations (cfear_odometry_set_surface_recording, cfear_odometry_surface). Host code only: the sample design and its
// pseudo-inverse are cov_design.h's, the sampling stage runs in pipeline.hip's sweep (cov_sampling_dev.h), the surface kernels through its
// launch functions (pipeline_launch.h).
#include <cmath>

#include "odometry_obj.h"
#include "pipeline_launch.h"
#include "cov_design.h"

// the [B] records of the registrations (cost sampling and surface recording share them), all 'nothing recorded'. The streams are idle.
static int odo_ensure_cov_ctx(cfear_ctx* ctx, cfear_odometry* o, const char* what) {
  return o->d_cov_ctx.ensure(ctx, (size_t)o->B, what, true);
}

extern "C" {

// ---- estimate_cov_by_sampling on the batched routes (cov_sampling_dev.h) ------------------------------------------------
int cfear_odometry_set_cov_sampling(cfear_ctx* ctx, cfear_odometry* o, int enable, double xy_range, double yaw_range, int samples_per_axis,
                                    double covariance_scaler) {
  if (!ctx || !o) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_set_cov_sampling: bad argument");
  if (!enable) {  // the buffers stay for a later switch back on; kernels already queued keep the parameters they were given
    o->cov_on = false;
    return CFEAR_OK;
  }
  if (samples_per_axis < 1 || !std::isfinite(xy_range) || !std::isfinite(yaw_range) || !std::isfinite(covariance_scaler))
    return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_set_cov_sampling: samples_per_axis < 1 or a range / scaler that is not finite");
  if (samples_per_axis > 8) return cfear_fail(ctx, CFEAR_ERR_UNSUPPORTED, "odometry_set_cov_sampling: at most 8 samples per axis (512 GetCost per sweep)");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  CFEAR_TRY(odo_join(ctx, o));
  CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // nothing in flight reads the design or the costs while they are replaced
  const int m = samples_per_axis * samples_per_axis * samples_per_axis;
  std::vector<double> offs, A, design((size_t)13 * m);
  cov_sample_design(xy_range, yaw_range, samples_per_axis, offs, A);
  pinv10_svd(m, A.data(), design.data());
  memcpy(design.data() + 10 * (size_t)m, offs.data(), sizeof(double) * 3 * m);
  CFEAR_TRY(odo_ensure_cov_ctx(ctx, o, "hipMalloc cost-sampling buffers"));
  CFEAR_TRY(o->d_cov_design.ensure(ctx, 13 * (size_t)m, "hipMalloc cost-sampling buffers"));
  CFEAR_TRY(o->d_cov_costs.ensure(ctx, (size_t)m * o->B, "hipMalloc cost-sampling buffers"));
  CFEAR_HIP_CHECK(ctx, hipMemset(o->d_cov_costs, 0, sizeof(double) * (size_t)m * o->B));
  CFEAR_HIP_CHECK(ctx, hipMemcpy(o->d_cov_design, design.data(), sizeof(double) * 13 * (size_t)m, hipMemcpyHostToDevice));
  // no sweep sampled yet under these settings (n = 0: cov_samples reads zeros and 'not sampled')
  CFEAR_HIP_CHECK(ctx, hipMemset(o->d_cov_ctx, 0, sizeof(CovSampleCtx) * (size_t)o->B));
  o->cov_m = m; o->cov_scaler = covariance_scaler; o->cov_on = true;
  return CFEAR_OK;
}

// ---- cost surfaces on the batched step (surface_dev.h) ---------------------------------------------------------------
int cfear_odometry_set_surface_recording(cfear_ctx* ctx, cfear_odometry* o, int enable) {
  if (!ctx || !o) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_set_surface_recording: bad argument");
  if (!enable) { o->surf_on = false; return CFEAR_OK; }
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (!o->d_cov_ctx) {
    CFEAR_TRY(odo_join(ctx, o));
    CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    CFEAR_TRY(odo_ensure_cov_ctx(ctx, o, "hipMalloc surface records"));
  }
  o->surf_on = true;
  return CFEAR_OK;
}

int cfear_odometry_surface(cfear_ctx* ctx, cfear_odometry* o, double res, int width, double* d_surface, int* n_used, int* itr_used,
                           double* poses_used) {
  if (!ctx || !o || !d_surface) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_surface: bad argument");
  if (!o->surf_on && !o->cov_on)
    return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_surface: nothing is recorded (cfear_odometry_set_surface_recording)");
  int pixels = 0, vx = 0, vy = 0;
  {
    const int rc = cfear_surface_dims(res, width, 0.0, 0.0, &pixels, &vx, &vy);
    if (rc == CFEAR_ERR_INVALID) return cfear_fail(ctx, rc, "odometry_surface: res must be finite and > 0, width >= 0");
    if (rc != CFEAR_OK) return cfear_fail(ctx, rc, "odometry_surface: more than CFEAR_SURFACE_MAX_SIDE pixels per side");
  }
  if (const int q = o->cfg.other_cost()) {
    char msg[320];
    snprintf(msg, sizeof(msg), "odometry_surface: the sequences' shapes differ in cost (sequence 0: %d, sequence %d: %d; cfear_odometry_set_sequence_shapes) - the "
             "evaluation is one launch per cost metric over all problems; surfaces run under shapes of one cost (any submap_scan_size)",
             (int)o->cfg.shapes[0].cost, q, (int)o->cfg.shapes[(size_t)q].cost);
    return cfear_fail(ctx, CFEAR_ERR_UNSUPPORTED, msg);
  }
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  CFEAR_TRY(odo_seq_sync(ctx, o, "odometry_surface"));
  CFEAR_TRY(odo_join(ctx, o));
  const int B = o->B;
  // what the last step's registrations used: the grid of each is centred on its recorded pose (computed here, on the host)
  std::vector<CovSampleCtx> rec;
  if (o->surf_ready) {
    rec.resize((size_t)B);
    CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(rec.data(), o->d_cov_ctx, sizeof(CovSampleCtx) * (size_t)B, hipMemcpyDeviceToHost, ctx->stream));
  }
  CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  const int cap_rc = odo_capacity_check(ctx, o, "odometry_surface");  // (the stream is idle: the surfaces are computed all the same)
  CFEAR_TRY(o->d_surf_hdr.ensure(ctx, (size_t)B, "hipMalloc surface buffers"));
  CFEAR_TRY(o->d_surf_coords.ensure(ctx, 2 * (size_t)pixels * B, "hipMalloc surface buffers"));
  CFEAR_TRY(o->d_surf_nxy.ensure(ctx, 2 * (size_t)B, "hipMalloc surface buffers"));
  std::vector<double> coords(2 * (size_t)pixels * B, 0.0);
  std::vector<int> nxy(2 * (size_t)B, 0);
  for (int q = 0; q < B; q++) {
    const int n = o->surf_ready ? rec[q].n : 0;
    if (n >= 2) {
      const double* last = rec[q].pose + 3 * (n - 1);
      nxy[2 * q] = cfear_surface_axis(last[0], res, width, pixels, coords.data() + (size_t)q * 2 * pixels);
      nxy[2 * q + 1] = cfear_surface_axis(last[1], res, width, pixels, coords.data() + (size_t)q * 2 * pixels + pixels);
    }
    if (n_used) n_used[q] = n >= 2 ? n : 0;
    if (itr_used) itr_used[q] = n >= 2 ? rec[q].itr : 0;
    if (poses_used) {
      double* d = poses_used + (size_t)q * 3 * MAX_SCANS;
      for (int i = 0; i < 3 * MAX_SCANS; i++) d[i] = (n >= 2 && i < 3 * n) ? rec[q].pose[i] : 0.0;
    }
  }
  CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(o->d_surf_coords, coords.data(), sizeof(double) * coords.size(), hipMemcpyHostToDevice, ctx->stream));
  CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(o->d_surf_nxy, nxy.data(), sizeof(int) * nxy.size(), hipMemcpyHostToDevice, ctx->stream));
  OdoParams OP = odo_params(ctx, o);
  OP.cs.ctx = o->d_cov_ctx;
  if (o->surf_ready) {
    cfear_launch_surface_build_step(OP, B, o->d_scratch_hdr, o->d_surf_hdr, o->d_surf_coords, o->d_surf_nxy, pixels, d_surface, ctx->stream);
    CFEAR_HIP_CHECK(ctx, hipGetLastError());
  } else {  // no step since the last reset / replay: no blocks, no visited cells (all NaN)
    CFEAR_HIP_CHECK(ctx, hipMemsetAsync(o->d_surf_hdr, 0, sizeof(SurfHdr) * (size_t)B, ctx->stream));
  }
  if (!cfear_surface_build_evaluates() || !o->surf_ready) {
    RegParams eval_rp = OP.rp;
    eval_rp.cost = o->cfg.effective(0, ctx->par).par.cost;  // (one cost: checked above)
    launch_surface_eval(eval_rp, B, o->d_surf_hdr, o->d_surf_coords, o->d_surf_nxy, pixels, d_surface, ctx->stream);
    CFEAR_HIP_CHECK(ctx, hipGetLastError());
  }
  return cap_rc;
}

int cfear_odometry_cov_samples(cfear_ctx* ctx, cfear_odometry* o, int sequence, double* costs, int* sampled) {
  if (!ctx || !o || sequence < 0 || sequence >= o->B || (!costs && !sampled)) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_cov_samples: bad argument");
  if (!o->cov_on) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_cov_samples: cost sampling is off (cfear_odometry_set_cov_sampling)");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  CFEAR_TRY(odo_join(ctx, o));
  CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (costs) CFEAR_HIP_CHECK(ctx, hipMemcpy(costs, o->d_cov_costs + (size_t)sequence * o->cov_m, sizeof(double) * o->cov_m, hipMemcpyDeviceToHost));
  if (sampled) {
    CovSampleCtx c;
    CFEAR_HIP_CHECK(ctx, hipMemcpy(&c, o->d_cov_ctx + sequence, sizeof(c), hipMemcpyDeviceToHost));
    *sampled = c.n >= 2 ? c.sampled : 0;
  }
  return odo_capacity_check(ctx, o, "odometry_cov_samples");
}

}  // extern "C"
