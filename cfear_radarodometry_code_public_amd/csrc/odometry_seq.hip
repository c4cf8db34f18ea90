// odometry_seq.hip -- the per-sequence configuration of a batched odometry object (the grids of utils/worker:26-99 as sequences of one
// object): the five setters and their getters, the device table the kernels read (SeqParams, OdoParams::seq) and the ONE path by which a
// configuration reaches the object. Host code only: no kernel lives here.
//
// Every rule is a pure function of seq_config.h (tests/test_seq_config_cpu.py checks them without a GPU). A setter is cfear_seq_set_* -
// the call's checks, a candidate that is the object's configuration with one table replaced, the candidate's consistency - and
// odo_commit_config of the candidate.
#include <algorithm>

#include "odometry_obj.h"

static SeqParams seq_row_of(const cfear_seq_config::effective_t& e) {
  const cfear_params& p = e.par;
  SeqParams r;
  memset(&r, 0, sizeof(r));
  r.loss_limit = p.loss_limit; r.covar_scale = p.covar_scale; r.regularization = p.regularization;
  r.min_keyframe_dist = p.min_keyframe_dist; r.min_keyframe_rot_deg = p.min_keyframe_rot_deg;
  r.radius = (float)p.res; r.weight_intensity = p.weight_intensity; r.loss = p.loss; r.weight_opt = p.weight_opt;
  r.max_outer = p.max_itr_association; r.min_itr = p.min_itr; r.max_inner = p.max_solver_iterations;
  r.compensate = p.compensate; r.use_keyframe = p.use_keyframe;
  r.z_min = (int)(uint8_t)(int)p.z_min;  // as the filter takes it (radar_filters.cpp:198, :212)
  r.source = e.source;
  r.k = p.k_strongest;
  r.shape = seq_shape_pack(p.cost, p.submap_scan_size);
  r.fuser = (e.fuser.soft_constraint ? SEQ_FUSER_SOFT : 0) | (e.fuser.use_guess ? 0 : SEQ_FUSER_NO_GUESS);
  return r;
}
// (re)builds the launch groups and the device table from the object's configuration; frees them when it needs none. The context stream and
// the object's streams are idle when this is called.
static int seq_table_upload(cfear_ctx* ctx, cfear_odometry* o) {
  const cfear_seq_config& C = o->cfg;
  if (C.shapes.empty()) { o->groups = cfear_seq_groups(); o->d_group_list.release(); o->d_seq_group.release(); }
  o->seq_zmin = C.filter_zmin();
  if (!C.needs_table()) {
    o->d_seq.release();
    return CFEAR_OK;
  }
  if (!C.shapes.empty()) {  // the launch groups of the registration stage and their static list (launch_register_kernel)
    cfear_seq_groups G;
    if (!C.groups(CFEAR_STEP_SMALL_SCANS, G))
      return cfear_fail(ctx, CFEAR_ERR_INVALID, "sequence shapes: a cost or submap_scan_size that is none");  // (refused by the caller before: never reached)
    CFEAR_TRY(o->d_group_list.ensure(ctx, (size_t)o->B, "hipMalloc sequence group list"));
    CFEAR_TRY(o->d_seq_group.ensure(ctx, (size_t)o->B, "hipMalloc sequence group list"));
    CFEAR_HIP_CHECK(ctx, hipMemcpy(o->d_group_list, G.list.data(), sizeof(int) * (size_t)o->B, hipMemcpyHostToDevice));
    CFEAR_HIP_CHECK(ctx, hipMemcpy(o->d_seq_group, G.group.data(), sizeof(int) * (size_t)o->B, hipMemcpyHostToDevice));
    o->groups = G;
    o->order_ready = false;  // (no sweep since create / reset: nothing was recorded)
  }
  std::vector<SeqParams> t((size_t)o->B);
  for (int q = 0; q < o->B; q++) t[q] = seq_row_of(C.effective(q, ctx->par));
  CFEAR_TRY(o->d_seq.ensure(ctx, t.size(), "hipMalloc sequence parameter table"));
  CFEAR_HIP_CHECK(ctx, hipMemcpy(o->d_seq, t.data(), sizeof(SeqParams) * t.size(), hipMemcpyHostToDevice));
  o->seq_par_seen = ctx->par;
  return CFEAR_OK;
}
__attribute__((visibility("hidden"))) int odo_seq_resync(cfear_ctx* ctx, cfear_odometry* o, const char* what) {
  CFEAR_SEQ_TRY(ctx, cfear_seq_config_check(o->cfg, odo_seq_object(ctx, o), what, msg));
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  CFEAR_TRY(odo_join(ctx, o));
  CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return seq_table_upload(ctx, o);
}

// the staging and replay chunk buffers are sized per input sweep of a step and per detection: released, allocated again by the next call that needs them
static void odo_release_chunk_buffers(cfear_odometry* o) {
  o->d_polar.release();
  for (int i = 0; i < 2; i++) { o->rp_polar[i].release(); o->rp_slots[i].release(); }
  o->rp_cfar_rows.release();
  o->rp_chunk = 0; o->rp_polar_chunk = 0; o->rp_used_pending[0] = o->rp_used_pending[1] = false;
}
// THE way a checked candidate becomes the object's configuration (the candidate leaves with the previous one). grid: the detectors' new plan
// and tables, which may be none (null: the detectors did not change, the object's grid stays). A failure leaves the object with the
// configuration, the table and the buffers it had, and its text in the context.
static int odo_commit_config(cfear_ctx* ctx, cfear_odometry* o, cfear_seq_config& cand, cfear_cfar_grid_ptr* grid = nullptr) {
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  CFEAR_TRY(odo_join(ctx, o));
  if (o->rp_stream) CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(o->rp_stream));
  CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  // what the candidate needs of memory first, the new beside the old: a failure leaves the object as it was
  const bool resweep = cand.sources(o->B) != odo_sources(o);
  DevBuf<uint32_t> ns[2];  // both parities of the filter-ahead slot buffers hold one slot block per input sweep
  if (resweep && o->filter != CFEAR_FILTER_CACFAR) {
    const size_t n = (size_t)cand.sources(o->B) * o->cap_points;
    const char* what = "hipMalloc filter slot buffers for the source map";
    if (ns[0].ensure(ctx, n, what) != CFEAR_OK || ns[1].ensure(ctx, n, what) != CFEAR_OK) return cfear_fail(ctx, CFEAR_ERR_NOMEM, what);
  }
  if (grid)  // the step's row scratch for the new detections
    CFEAR_TRY(o->d_cfar_rows.ensure(ctx, *grid ? cfear_cfar_grid_scratch_ints(ctx, grid->get(), 1) : cfear_cfar_scratch_ints(ctx, (size_t)o->B), "hipMalloc cfar rows"));
  std::swap(o->cfg, cand);
  const int rc = seq_table_upload(ctx, o);
  if (rc != CFEAR_OK) {  // the previous configuration and its table; the text of the failure stays
    const std::string err = ctx->err;
    std::swap(o->cfg, cand);
    (void)seq_table_upload(ctx, o);
    ctx->err = err;
    return rc;
  }
  if (grid) o->det_grid.swap(*grid);  // (the previous grid goes with the caller's owner: nothing in flight reads it)
  if (ns[0]) for (int i = 0; i < 2; i++) { o->d_slots[i] = std::move(ns[i]); o->filt_pending[i] = false; }
  if (resweep || grid) odo_release_chunk_buffers(o);
  return CFEAR_OK;
}

// ---- per-sequence parameters and shared input sweeps (odometrykeyframefuser.h:72-114; utils/worker:26-99) -----------------------------
int cfear_odometry_set_sequence_params(cfear_ctx* ctx, cfear_odometry* o, const cfear_params* rows, int n_rows) {
  cfear_seq_config cand;
  CFEAR_SEQ_TRY(ctx, cfear_seq_set_params(rows, n_rows, odo_seq_object(ctx, o), cand, msg));
  return odo_commit_config(ctx, o, cand);
}

int cfear_odometry_sequence_params(cfear_ctx* ctx, cfear_odometry* o, int sequence, cfear_params* out) {
  if (!ctx || !o || !out || sequence < 0 || sequence >= o->B) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_sequence_params: bad argument");
  *out = o->cfg.effective(sequence, ctx->par).par;
  return CFEAR_OK;
}

int cfear_odometry_set_sequence_sources(cfear_ctx* ctx, cfear_odometry* o, const int32_t* source, int n_sequences, int n_sources) {
  cfear_seq_config cand;
  CFEAR_SEQ_TRY(ctx, cfear_seq_set_sources(source, n_sequences, n_sources, odo_seq_object(ctx, o), cand, msg));
  return odo_commit_config(ctx, o, cand);
}

// ---- per-sequence cost metric and submap size (utils/worker:49-52) --------------------------------------------------------------------
int cfear_odometry_set_sequence_shapes(cfear_ctx* ctx, cfear_odometry* o, const cfear_seq_shape* shapes, int n_rows) {
  cfear_seq_config cand;
  CFEAR_SEQ_TRY(ctx, cfear_seq_set_shapes(shapes, n_rows, odo_seq_object(ctx, o), cand, msg));
  return odo_commit_config(ctx, o, cand);
}

int cfear_odometry_sequence_shape(cfear_ctx* ctx, cfear_odometry* o, int sequence, cfear_seq_shape* out) {
  if (!ctx || !o || !out || sequence < 0 || sequence >= o->B) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_sequence_shape: bad argument");
  const cfear_params p = o->cfg.effective(sequence, ctx->par).par;
  out->cost = p.cost; out->submap_scan_size = p.submap_scan_size;
  return CFEAR_OK;
}

// ---- per-sequence CA-CFAR detectors over shared sweeps (params/kstrong_vs_cfar/oxford-cfear-3-ca-cfar: window_size x false_alarm_rate) ---------
int cfear_odometry_set_sequence_detectors(cfear_ctx* ctx, cfear_odometry* o, const cfear_seq_detector* dets, int n_rows, const int32_t* source, int n_sources) {
  const char* what = "odometry_set_sequence_detectors";
  const cfear_seq_object O = odo_seq_object(ctx, o);
  CFEAR_SEQ_TRY(ctx, cfear_seq_detectors_call_check(dets, n_rows, source, n_sources, O, what, msg));
  cfear_cfar_grid_ptr grid;
  if (dets) {
    cfear_cfar_grid* g = nullptr;
    CFEAR_TRY(cfear_cfar_grid_create(ctx, dets, source, o->B, source ? n_sources : o->B, what, &g));
    grid.reset(g);
  }
  cfear_seq_config cand;
  CFEAR_SEQ_TRY(ctx, cfear_seq_set_detectors(dets, n_rows, source, n_sources, O, what, cand, msg));
  return odo_commit_config(ctx, o, cand, &grid);
}

int cfear_odometry_sequence_detector(cfear_ctx* ctx, cfear_odometry* o, int sequence, cfear_seq_detector* out) {
  if (!ctx || !o || !out || sequence < 0 || sequence >= o->B) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_sequence_detector: bad argument");
  *out = o->cfg.detector(sequence, ctx->par);
  return CFEAR_OK;
}

// ---- the fuser's own switches (odometrykeyframefuser.h:94; odometrykeyframefuser.cpp:165-168, :186) per sequence ------------------------
int cfear_odometry_set_fuser_options(cfear_ctx* ctx, cfear_odometry* o, const cfear_fuser_options* rows, int n_rows) {
  cfear_seq_config cand;
  CFEAR_SEQ_TRY(ctx, cfear_seq_set_fuser(rows, n_rows, odo_seq_object(ctx, o), cand, msg));
  return odo_commit_config(ctx, o, cand);
}

int cfear_odometry_fuser_options(cfear_ctx* ctx, cfear_odometry* o, int sequence, cfear_fuser_options* out) {
  if (!ctx || !o || !out || sequence < 0 || sequence >= o->B) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_fuser_options: bad argument");
  *out = o->cfg.effective(sequence, ctx->par).fuser;
  return CFEAR_OK;
}
