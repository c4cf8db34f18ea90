// odometry_run.hip -- the life of a batched odometry object (struct cfear_odometry, odometry_obj.h): creation, reset and destruction, the step
// entry points, the phase times and the profile, the replay of a recording, and the plain reads (poses, covariances, status, summary). No kernel is defined here: the sweeps go through the launch
// layer of pipeline.hip (odo_params, odo_launch_sweep, odo_launch_cfar), the filters through kstrongest.hip / cfar.hip, the persistent replay
// through replay.hip; the sizes and schedules are odometry_plan.h's. What the object does with the records of its registrations
// (cost-sampling covariance, cost surfaces) is odometry_cov.hip's.
#include <algorithm>
#include <memory>
#include <new>

#include "odometry_obj.h"
#include "odometry_plan.h"

// the overflow flags of `o`, all clear: created with the object when a scan can overflow its cells or the filter's clouds their points, by
// cfear_odometry_step_cloud_device otherwise (the caller's clouds may) when it is first used
int odo_ensure_flags(cfear_ctx* ctx, cfear_odometry* o) {
  if (o->d_flags) return CFEAR_OK;
  CFEAR_TRY(o->d_flags.ensure(ctx, (size_t)o->B + 1, "hipMalloc odometry state"));
  CFEAR_HIP_CHECK(ctx, hipMemsetAsync(o->d_flags, 0, sizeof(int) * o->d_flags.size(), ctx->stream));
  return CFEAR_OK;
}

// the streams and events every object (ev_copied) or an object with overlap has; false: one of them could not be made
static bool odo_make_streams(cfear_ctx* ctx, cfear_odometry* o) {
  if (o->ev_copied.create(hipEventDisableTiming) != hipSuccess) return false;
  if (!o->overlap) return true;
  int least = 0, greatest = 0;  // numerically lower = higher priority
  if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) return false;
  std::vector<uint32_t> mask_f, mask_o;  // cfear_tune FILTER_CUS: the filter's compute units and the odometry streams' (odometry_plan.h)
  int ncu = 0;
  if (ctx->tune_filter_cus > 0 && hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess) ncu = 0;
  cfear_cu_masks(ncu, ctx->tune_filter_cus, mask_f, mask_o);
  if ((mask_f.empty() ? o->sf.create_with_priority(hipStreamNonBlocking, least) : o->sf.create_with_cu_mask(mask_f)) != hipSuccess) return false;
  for (int i = 0; i < o->overlap; i++) {
    Stream st;
    if ((mask_o.empty() ? st.create_with_priority(hipStreamNonBlocking, greatest) : st.create_with_cu_mask(mask_o)) != hipSuccess) return false;
    o->so.push_back(std::move(st));
    for (auto* v : {&o->ev_free[0], &o->ev_free[1], &o->ev_done}) {
      Event e;
      if (e.create(hipEventDisableTiming) != hipSuccess) return false;
      v->push_back(std::move(e));
    }
  }
  for (Event* e : {&o->ev_in, &o->ev_filt[0], &o->ev_filt[1]})
    if (e->create(hipEventDisableTiming) != hipSuccess) return false;
  return true;
}

extern "C" {

// ---- batched odometry --------------------------------------------------------------------------
void cfear_odometry_destroy(cfear_ctx* ctx, cfear_odometry* o) {
  if (!o) return;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    const std::vector<hipStream_t> own = o->streams();  // drained, then no longer the context's to wait for
    for (hipStream_t st : own) (void)hipStreamSynchronize(st);
    (void)hipStreamSynchronize(ctx->stream);
    for (hipStream_t st : own) {
      const auto it = std::find(ctx->aux_streams.begin(), ctx->aux_streams.end(), st);
      if (it != ctx->aux_streams.end()) ctx->aux_streams.erase(it);
    }
  }
  delete o;  // (events, streams, then the device buffers and the detectors' grid: the member order of odometry_obj.h)
}

int cfear_odometry_reset(cfear_ctx* ctx, cfear_odometry* o) {
  if (!ctx || !o) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_reset: bad argument");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  CFEAR_TRY(odo_join(ctx, o));
  std::vector<SeqState> st((size_t)o->B);
  for (auto& s : st) {
    memset(&s, 0, sizeof(s));
    s.T_prev.l0 = s.T_prev.l3 = 1; s.Tmot.l0 = s.Tmot.l3 = 1; s.Tcurrent.l0 = s.Tcurrent.l3 = 1;  // odometrykeyframefuser.cpp:34-38
  }
  CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(o->d_states, st.data(), sizeof(SeqState) * st.size(), hipMemcpyHostToDevice, ctx->stream));
  CFEAR_HIP_CHECK(ctx, hipMemsetAsync(o->d_summaries, 0, sizeof(cfear_reg_summary) * (size_t)o->B, ctx->stream));
  CFEAR_HIP_CHECK(ctx, hipMemsetAsync(o->d_poses_out, 0, sizeof(double) * 3 * (size_t)o->B, ctx->stream));
  CFEAR_HIP_CHECK(ctx, hipMemsetAsync(o->d_cov_work, 0, sizeof(double) * 36 * (size_t)o->B, ctx->stream));
  if (o->d_flags) CFEAR_HIP_CHECK(ctx, hipMemsetAsync(o->d_flags, 0, sizeof(int) * ((size_t)o->B + 1), ctx->stream));
  if (o->kf.what) CFEAR_TRY(o->kf.clear(ctx, o->B));  // (the setting stays, the log starts again at keyframe 0)
  o->order_ready = false;
  o->surf_ready = false;
  o->sweeps = 0;  // (the parameter table, the source map and the fuser options stay)
  CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return CFEAR_OK;
}

// the device memory every object has, sized by the fields cfear_odometry_create has set (scratch_bytes: of one sequence's scratch block)
static int odo_alloc_state(cfear_ctx* ctx, cfear_odometry* o, size_t scratch_bytes) {
  const size_t B = (size_t)o->B;
  const char* what = "hipMalloc odometry state";
  CFEAR_TRY(o->d_scans.ensure(ctx, o->scan_stride * B * o->nslots, what));
  CFEAR_TRY(o->d_scratch.ensure(ctx, scratch_bytes * B, what, true));  // dense voxel tables start all-zero
  CFEAR_TRY(o->d_scratch_hdr.ensure(ctx, B, what));
  CFEAR_TRY(o->d_states.ensure(ctx, B, what));
  CFEAR_TRY(o->d_cov_work.ensure(ctx, 36 * B, what));
  CFEAR_TRY(o->d_summaries.ensure(ctx, B, what));
  CFEAR_TRY(o->d_poses_out.ensure(ctx, 3 * B, what));
  if (o->filter == CFEAR_FILTER_CACFAR) {
    CFEAR_TRY(o->d_cloud.ensure(ctx, 3 * B * o->cap_points, what));
    CFEAR_TRY(o->d_cloud_n.ensure(ctx, B, what));
    CFEAR_TRY(o->d_cfar_rows.ensure(ctx, cfear_cfar_scratch_ints(ctx, B), what));
  } else {
    for (auto& slots : o->d_slots) CFEAR_TRY(slots.ensure(ctx, B * o->cap_points, what));
  }
  if (o->cap_cells < o->cap_points || o->filter == CFEAR_FILTER_CACFAR) CFEAR_TRY(odo_ensure_flags(ctx, o));
  if (ctx->tune_reg_order && o->B >= 2) {
    CFEAR_TRY(o->d_order.ensure(ctx, B, what));
    CFEAR_TRY(o->d_work.ensure(ctx, B, what, true));
  }
  return CFEAR_OK;
}

struct odo_destroy_with { cfear_ctx* ctx; void operator()(cfear_odometry* o) const { cfear_odometry_destroy(ctx, o); } };

int cfear_odometry_create(cfear_ctx* ctx, int n_sequences, cfear_odometry** out) {
  if (!ctx || !out || n_sequences <= 0) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_create: bad argument");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  *out = nullptr;
  std::unique_ptr<cfear_odometry, odo_destroy_with> owner(new (std::nothrow) cfear_odometry(), odo_destroy_with{ctx});  // every failure below is an early return
  cfear_odometry* o = owner.get();
  if (!o) return cfear_fail(ctx, CFEAR_ERR_NOMEM, "odometry alloc");
  if (ctx->tune_voxel_order != 0)
    return cfear_fail(ctx, CFEAR_ERR_UNSUPPORTED, "odometry_create: cfear_tune VOXEL_ORDER = 1 (PCL <= 1.9's std::sort order) needs a host round trip per scan: per-call scans only "
                      "(cfear_scan_create; the mirror classes of cfear_host.hpp use it)");
  const int B = n_sequences, s = ctx->par.submap_scan_size;
  o->filter = ctx->par.filter_type;
  o->large_kernel = ctx->tune_large_kernel;
  { int ncu = 0; if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, ctx->device) == hipSuccess && ncu > 0) o->n_cus = ncu; }
  const bool cfar = o->filter == CFEAR_FILTER_CACFAR;
  const cfear_odo_caps C = cfear_odo_capacities(cfar, ctx->A, ctx->par.k_strongest, ctx->par.cfar_max_points, s, ctx->tune_max_cells, ctx->tune_nn_tie);
  o->B = B; o->nslots = s + 1; o->cap_points = C.cap_points; o->cap_cells = C.cap_cells; o->pair_cap = C.pair_cap;
  o->with_kd = ctx->tune_nn_tie == 2;
  size_t scan_bytes = 0, scratch_bytes = 0;
  odo_block_bytes(o, &scan_bytes, &scratch_bytes);
  {  // refuse what cannot fit with a message that names the numbers (a bare NOMEM after gigabytes of partial allocations helps nobody)
    size_t free_b = 0, total_b = 0;
    const size_t per_seq = scan_bytes * (size_t)o->nslots + scratch_bytes + sizeof(uint32_t) * 2 * (size_t)o->cap_points + sizeof(SeqState) + 4096;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && per_seq * (size_t)B > free_b) {
      char msg[512];
      snprintf(msg, sizeof(msg), "odometry_create: %d sequences x %.1f MB (%d scan slots of %.2f MB for %d points / %d cells each + %.1f MB of scratch for %d residual "
               "blocks) = %.1f GB, %.1f GB free: at most %zu sequences fit - or size the scans for fewer cells (cfear_tune CFEAR_TUNE_MAX_CELLS, now %d)",
               B, per_seq / 1048576.0, o->nslots, scan_bytes / 1048576.0, o->cap_points, o->cap_cells, scratch_bytes / 1048576.0, o->pair_cap,
               per_seq * (double)B / 1073741824.0, free_b / 1073741824.0, free_b / per_seq, o->cap_cells);
      return cfear_fail(ctx, CFEAR_ERR_NOMEM, msg);
    }
  }
  o->scan_stride = scan_bytes;
  CFEAR_TRY(odo_alloc_state(ctx, o, scratch_bytes));
  CFEAR_TRY(odo_upload_headers(ctx, o, scratch_bytes));
  CFEAR_TRY(cfear_odometry_reset(ctx, o));
  o->overlap = cfear_odo_overlap(ctx->tune_odo_overlap, B, cfar);
  if (!odo_make_streams(ctx, o)) return cfear_fail(ctx, CFEAR_ERR_HIP, "odometry stream creation");
  for (hipStream_t st : o->streams()) ctx->aux_streams.push_back(st);  // (sf, then so: cfear_synchronize waits for them too)
  *out = owner.release();
  return CFEAR_OK;
}

// one sweep of every sequence from clouds on the device, on the context stream
static int odo_step_clouds(cfear_ctx* ctx, cfear_odometry* o, const float* d_xyi, int capacity, const int* d_counts, bool filter_events) {
  const OdoParams OP = odo_params(ctx, o);
  if (o->profile && !filter_events) {  // (keeps filter_events / stage_events paired per step for the profile readers)
    CFEAR_TRY(o->timers.take(ctx, ctx->stream, o->filter_events));
    CFEAR_TRY(o->timers.take(ctx, ctx->stream, o->filter_events));
  }
  CFEAR_TRY(odo_launch_sweep(ctx, o, OP, SweepPoints::of_clouds(d_xyi, capacity, d_counts), o->B, ctx->stream, o->profile));
  o->surf_ready = OP.cs.ctx != nullptr;
  o->step_no++; o->sweeps++;
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  return CFEAR_OK;
}

int cfear_odometry_step_cloud_device(cfear_ctx* ctx, cfear_odometry* o, const float* d_xyi, int capacity, const int* d_counts) {
  if (!ctx || !o || !d_xyi || !d_counts || capacity <= 0) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_step_cloud: bad argument");
  CFEAR_TRY(odo_shape_check(ctx, o, "odometry_step_cloud"));
  if (!o->cfg.src.empty())
    return cfear_fail(ctx, CFEAR_ERR_UNSUPPORTED, "odometry_step_cloud: the object has a source map (cfear_odometry_set_sequence_sources), which the cloud route does not "
                      "read - it takes one cloud per sequence; clear the map (NULL) first");
  if (o->cfg.dets_mapped)
    return cfear_fail(ctx, CFEAR_ERR_UNSUPPORTED, "odometry_step_cloud: the object has per-sequence detectors with a source map (cfear_odometry_set_sequence_detectors), "
                      "which the cloud route does not read - it takes one cloud per sequence; clear them (NULL) first");
  for (size_t q = 0; q < o->cfg.rows.size(); q++)
    if (o->cfg.rows[q].k_strongest != ctx->par.k_strongest) {
      char msg[256];
      snprintf(msg, sizeof(msg), "odometry_step_cloud: row %d of the object's table has k_strongest = %d, the context %d - a cloud has no slots to take the k strongest "
               "of; the cloud route runs with rows of the context's k_strongest only", (int)q, o->cfg.rows[q].k_strongest, ctx->par.k_strongest);
      return cfear_fail(ctx, CFEAR_ERR_UNSUPPORTED, msg);
    }
  CFEAR_TRY(odo_seq_sync(ctx, o, "odometry_step_cloud"));
  if (capacity > o->cap_points) {
    char msg[256];
    snprintf(msg, sizeof(msg), "odometry_step_cloud: capacity %d exceeds the %d points per scan this object was created for (A * k_strongest, or cfar_max_points with "
             "filter_type CA-CFAR)", capacity, o->cap_points);
    return cfear_fail(ctx, CFEAR_ERR_INVALID, msg);
  }
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  CFEAR_TRY(odo_join(ctx, o));
  CFEAR_TRY(odo_ensure_flags(ctx, o));  // counts beyond `capacity` are reported like every other truncation
  return odo_step_clouds(ctx, o, d_xyi, capacity, d_counts, false);
}

int cfear_odometry_step_device(cfear_ctx* ctx, cfear_odometry* o, const uint8_t* d_polar) {
  if (!ctx || !o || !d_polar) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_step: bad argument");
  CFEAR_TRY(odo_shape_check(ctx, o, "odometry_step"));
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  CFEAR_TRY(odo_seq_sync(ctx, o, "odometry_step"));
  CFEAR_TRY(odo_peaks_check(ctx, o, "odometry_step"));
  if (o->filter == CFEAR_FILTER_CACFAR) {  // radar_driver.cpp:52-56, then the cloud route
    if (o->profile) CFEAR_TRY(o->timers.take(ctx, ctx->stream, o->filter_events));
    CFEAR_TRY(odo_launch_cfar(ctx, o, d_polar, 1, o->d_cloud, o->d_cloud_n, o->d_cfar_rows, ctx->stream));
    if (o->profile) CFEAR_TRY(o->timers.take(ctx, ctx->stream, o->filter_events));
    return odo_step_clouds(ctx, o, o->d_cloud, o->cap_points, o->d_cloud_n, true);
  }
  const OdoParams OP = odo_params(ctx, o);
  const int buf = o->overlap ? (int)(o->step_no & 1) : 0;
  hipStream_t sf = o->overlap ? o->sf : ctx->stream;
  if (o->overlap) {
    CFEAR_HIP_CHECK(ctx, hipEventRecord(o->ev_in, ctx->stream));  // the sweeps are ready at this point of the context stream
    CFEAR_HIP_CHECK(ctx, hipStreamWaitEvent(sf, o->ev_in, 0));
    if (o->filt_pending[buf])  // features(t-2) of every range has read this buffer
      for (hipEvent_t e : o->ev_free[buf]) CFEAR_HIP_CHECK(ctx, hipStreamWaitEvent(sf, e, 0));
  }
  // radar_driver.cpp:58
  if (o->profile) CFEAR_TRY(o->timers.take(ctx, sf, o->filter_events));
  CFEAR_TRY(cfear_launch_kstrongest(ctx, d_polar, odo_sources(o), o->d_slots[buf], sf, odo_filter_peaks(o), o->seq_zmin));  // (once per source sweep, at the smallest z_min of the rows; no peak flag unless the object records peaks clouds: the feature stage does not read it)
  if (o->profile) CFEAR_TRY(o->timers.take(ctx, sf, o->filter_events));
  if (o->overlap) {
    CFEAR_HIP_CHECK(ctx, hipEventRecord(o->ev_filt[buf], sf));
    // d_polar keeps its stream-order meaning for the caller: whatever the context stream is given after this call (the
    // caller's next write into the buffer, its release to a caching allocator) waits for the filter, the only reader
    CFEAR_HIP_CHECK(ctx, hipStreamWaitEvent(ctx->stream, o->ev_filt[buf], 0));
  }
  const int nsub = o->overlap ? o->overlap : 1;
  const int per = (o->B + nsub - 1) / nsub;
  for (int i = 0; i < nsub; i++) {
    OdoParams P = OP;
    P.seq0 = i * per;
    const int count = std::min(per, o->B - P.seq0);
    if (count <= 0) break;
    hipStream_t so = o->overlap ? o->so[i] : ctx->stream;
    if (o->overlap) CFEAR_HIP_CHECK(ctx, hipStreamWaitEvent(so, o->ev_filt[buf], 0));
    // (ev_free: features has consumed the slot buffer - recorded between the two stages; behind the cloud stage on an object that records clouds)
    CFEAR_TRY(odo_launch_sweep(ctx, o, P, SweepPoints::of_slots(o->d_slots[buf]), count, so, o->profile, o->overlap ? (hipEvent_t)o->ev_free[buf][i] : nullptr));
  }
  if (o->overlap) o->filt_pending[buf] = true;
  o->surf_ready = OP.cs.ctx != nullptr;
  o->step_no++; o->sweeps++;
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  return CFEAR_OK;
}

int cfear_odometry_phase_times(cfear_ctx* ctx, cfear_odometry* o, int enable, long long* host_ticks /*[B][32]*/) {
  if (!ctx || !o) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_phase_times: bad argument");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  CFEAR_TRY(odo_join(ctx, o));
  CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  const size_t bytes = sizeof(long long) * 32 * (size_t)o->B;
  if (enable >= 1 && enable <= 4) {  // (any other non-zero value: read without changing the mode)
    o->phase_detail = enable == 1 ? 1 : (enable == 4 ? 2 : 0);
    o->wg_only = enable == 3;
  }
  if (!enable) {
    o->d_phase_times.release();
    return CFEAR_OK;
  }
  if (!o->d_phase_times) return o->d_phase_times.ensure(ctx, 32 * (size_t)o->B, "hipMalloc phase times", true);
  if (host_ticks) {
    CFEAR_HIP_CHECK(ctx, hipMemcpy(host_ticks, o->d_phase_times, bytes, hipMemcpyDeviceToHost));
    CFEAR_HIP_CHECK(ctx, hipMemset(o->d_phase_times, 0, bytes));
  }
  return CFEAR_OK;
}

int cfear_odometry_profile(cfear_ctx* ctx, cfear_odometry* o, int enable) {
  if (!ctx || !o) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_profile: bad argument");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  CFEAR_TRY(odo_join(ctx, o));
  CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  o->filter_events.clear(); o->stage_events.clear(); o->timers.reset();  // the events go back to the pool
  if (enable && o->timers.events.empty()) CFEAR_TRY(o->timers.grow(ctx));  // created here, outside any timed region
  o->profile = enable != 0;
  return CFEAR_OK;
}

int cfear_odometry_profile_read(cfear_ctx* ctx, cfear_odometry* o, double* filter_seconds, int* filter_launches) {
  if (!ctx || !o) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_profile_read: bad argument");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  CFEAR_TRY(odo_join(ctx, o));
  CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  double tf = 0;
  const int nf = (int)(o->filter_events.size() / 2);
  for (int i = 0; i < nf; i++) {
    float a = 0.f;
    CFEAR_HIP_CHECK(ctx, hipEventElapsedTime(&a, o->filter_events[2 * i], o->filter_events[2 * i + 1]));
    tf += a * 1e-3;
  }
  if (filter_seconds) *filter_seconds = tf;
  if (filter_launches) *filter_launches = nf;
  return CFEAR_OK;
}

int cfear_odometry_profile_read_stages(cfear_ctx* ctx, cfear_odometry* o, double* features_seconds, double* registration_seconds, int* launches) {
  if (!ctx || !o) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_profile_read_stages: bad argument");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  CFEAR_TRY(odo_join(ctx, o));
  CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  double tf = 0, tr = 0;
  const int n = (int)(o->stage_events.size() / 3);
  for (int i = 0; i < n; i++) {
    float a = 0.f, b = 0.f;
    CFEAR_HIP_CHECK(ctx, hipEventElapsedTime(&a, o->stage_events[3 * i], o->stage_events[3 * i + 1]));
    CFEAR_HIP_CHECK(ctx, hipEventElapsedTime(&b, o->stage_events[3 * i + 1], o->stage_events[3 * i + 2]));
    tf += a * 1e-3; tr += b * 1e-3;
  }
  if (features_seconds) *features_seconds = tf;
  if (registration_seconds) *registration_seconds = tr;
  if (launches) *launches = n;
  return CFEAR_OK;
}

int cfear_odometry_step_host(cfear_ctx* ctx, cfear_odometry* o, const uint8_t* h_polar) {
  if (!ctx || !o || !h_polar) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_step_host: bad argument");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const size_t bytes = (size_t)odo_sources(o) * ctx->A * ctx->R;  // (cfear_odometry_set_sequence_sources releases a staging buffer of another size)
  CFEAR_TRY(o->d_polar.ensure(ctx, bytes + 64, "hipMalloc polar batch"));
  // the staging buffer is reused: the copy waits for the filter of the previous sweep (its only reader), not for that
  // sweep's features / registration
  if (o->overlap && o->step_no > 0) CFEAR_HIP_CHECK(ctx, hipStreamWaitEvent(ctx->stream, o->ev_filt[(o->step_no - 1) & 1], 0));
  CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(o->d_polar, h_polar, bytes, hipMemcpyHostToDevice, ctx->stream));
  // h_polar belongs to the caller again when this returns (pinned memory makes the copy truly asynchronous)
  CFEAR_HIP_CHECK(ctx, hipEventRecord(o->ev_copied, ctx->stream));
  const int rc = cfear_odometry_step_device(ctx, o, o->d_polar);
  CFEAR_HIP_CHECK(ctx, hipEventSynchronize(o->ev_copied));
  return rc;
}

// ---- replay of a recording without a host round trip per sweep (offline_odometry.cpp:103-125) -----------------------
int cfear_host_alloc(cfear_ctx* ctx, size_t bytes, void** out) {
  if (!ctx || !out || bytes == 0) return cfear_fail(ctx, CFEAR_ERR_INVALID, "host_alloc: bad argument");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  *out = nullptr;
  if (hipHostMalloc(out, bytes, hipHostMallocDefault) != hipSuccess) return cfear_fail(ctx, CFEAR_ERR_NOMEM, "hipHostMalloc");
  return CFEAR_OK;
}
void cfear_host_free(cfear_ctx* ctx, void* p) {
  if (!p) return;
  if (ctx) (void)hipSetDevice(ctx->device);
  (void)hipHostFree(p);
}

// chunk: sweeps per chunk the slot buffers must hold; staging: the host route also needs the two polar staging buffers of that many
// sweeps (the device route filters the frames where they lie and never touches them: for thousands of sequences they would be
// gigabytes allocated for nothing)
static int replay_ensure(cfear_ctx* ctx, cfear_odometry* o, int chunk, bool staging, size_t n_records) {
  if (!o->rp_stream) {  // the events first, the stream last: "the stream exists" says all of them do (a failure half-way leaves what was made to its owner)
    for (Event* e : {&o->rp_filt[0], &o->rp_filt[1], &o->rp_used[0], &o->rp_used[1], &o->rp_in})
      CFEAR_TRY(e->ensure(ctx, hipEventDisableTiming, "hipEventCreateWithFlags(e, hipEventDisableTiming)"));
    const hipError_t e = o->rp_stream.create(hipStreamNonBlocking);
    if (e != hipSuccess) return cfear_fail(ctx, CFEAR_ERR_HIP, "hipStreamCreateWithFlags(&o->rp_stream, hipStreamNonBlocking)", e);
    ctx->aux_streams.push_back(o->rp_stream);
  }
  // (a CA-CFAR object's clouds are one per sequence whatever the sweeps they come from)
  const size_t sweep = (size_t)odo_sources(o) * ctx->A * ctx->R, slots = (size_t)(o->filter == CFEAR_FILTER_CACFAR ? o->B : odo_sources(o)) * o->cap_points;
  if (chunk > o->rp_chunk) {
    CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(o->rp_stream));
    CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    o->rp_chunk = 0;  // (until every buffer holds `chunk` sweeps)
    o->rp_used_pending[0] = o->rp_used_pending[1] = false;
    for (int i = 0; i < 2; i++) {
      if (o->filter == CFEAR_FILTER_CACFAR) {  // a cloud of cap_points points + its count per sweep and sequence
        CFEAR_TRY(o->rp_cloud[i].ensure(ctx, 3 * slots * chunk, "hipMalloc replay cloud buffers"));
        CFEAR_TRY(o->rp_cloud_n[i].ensure(ctx, (size_t)o->B * chunk, "hipMalloc replay cloud buffers"));
      } else {
        CFEAR_TRY(o->rp_slots[i].ensure(ctx, slots * chunk, "hipMalloc replay slot buffers"));
      }
    }
    if (o->filter == CFEAR_FILTER_CACFAR)
      CFEAR_TRY(o->rp_cfar_rows.ensure(ctx, o->det_grid ? cfear_cfar_grid_scratch_ints(ctx, o->det_grid.get(), (size_t)chunk) : cfear_cfar_scratch_ints(ctx, (size_t)o->B * chunk),
                                       "hipMalloc replay cfar rows"));
    o->rp_chunk = chunk;
  }
  if (staging && chunk > o->rp_polar_chunk) {
    CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(o->rp_stream));
    CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    o->rp_polar_chunk = 0;
    for (auto& polar : o->rp_polar) CFEAR_TRY(polar.ensure(ctx, sweep * chunk + 64, "hipMalloc replay staging"));
    o->rp_polar_chunk = chunk;
  }
  if (n_records > o->d_records.size()) {
    CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    CFEAR_TRY(o->d_records.ensure(ctx, n_records, "hipMalloc sweep records"));
  }
  return CFEAR_OK;
}

// frames: n_sweeps x B x A x R bytes on the host (copied chunk by chunk into the staging buffers) or on the device (filtered where
// they lie); d_records: where the per-sweep records go on the device (null: none)
static int replay_impl_queue(cfear_ctx* ctx, cfear_odometry* o, const uint8_t* frames, bool on_device, int n_sweeps, cfear_sweep_record* d_records,
                             double* d_cov6) {
  const int nsrc = odo_sources(o);  // input sweeps per step: the sequences, or the sources of a source map
  const size_t sweep = (size_t)nsrc * ctx->A * ctx->R, slots = (size_t)(o->filter == CFEAR_FILTER_CACFAR ? o->B : nsrc) * o->cap_points;
  const bool cfar = o->filter == CFEAR_FILTER_CACFAR;
  const int chunk = cfear_replay_chunk(on_device, cfar, sweep, slots, n_sweeps, o->rp_chunk, o->rp_polar_chunk);  // sweeps per chunk (odometry_plan.h)
  int rc = replay_ensure(ctx, o, chunk, !on_device, 0);
  if (rc != CFEAR_OK) return rc;
  const int nchunks = (n_sweeps + chunk - 1) / chunk;
  OdoParams OP = odo_params(ctx, o);
  if (!o->cov_on) OP.cs.ctx = nullptr;  // the replay routes do not record for cost surfaces
  o->surf_ready = false;
  // (the keyframe recorder is a stage behind the registration stage: with recording on the sweeps run as two launches, like the timed ones)
  const bool persistent = o->B <= ctx->tune_replay_persistent_max && !OP.phase_times && !OP.wg_times && !o->kf.what;
  if (on_device) {  // the sweeps are ready at this point of the context stream: the replay stream (which reads them) starts there
    CFEAR_HIP_CHECK(ctx, hipEventRecord(o->rp_in, ctx->stream));
    CFEAR_HIP_CHECK(ctx, hipStreamWaitEvent(o->rp_stream, o->rp_in, 0));
  }
  auto stage = [&](int c) -> int {  // copy + filter of chunk c on the replay stream
    const int b = c & 1, t0 = c * chunk, cnt = std::min(chunk, n_sweeps - t0);
    if (o->rp_used_pending[b]) CFEAR_HIP_CHECK(ctx, hipStreamWaitEvent(o->rp_stream, o->rp_used[b], 0));  // its slots were consumed
    const uint8_t* src = frames + sweep * (size_t)t0;
    if (!on_device) {
      CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(o->rp_polar[b], src, sweep * (size_t)cnt, hipMemcpyHostToDevice, o->rp_stream));
      src = o->rp_polar[b];
    }
    const int frc = cfar ? odo_launch_cfar(ctx, o, src, cnt, o->rp_cloud[b], o->rp_cloud_n[b], o->rp_cfar_rows, o->rp_stream)  // radar_driver.cpp:52-56
                         : cfear_launch_kstrongest(ctx, src, cnt * nsrc, o->rp_slots[b], o->rp_stream, odo_filter_peaks(o), o->seq_zmin);  // radar_driver.cpp:58, pose-independent
    if (frc != CFEAR_OK) return frc;
    CFEAR_HIP_CHECK(ctx, hipEventRecord(o->rp_filt[b], o->rp_stream));
    return CFEAR_OK;
  };
  rc = stage(0);
  if (rc != CFEAR_OK) return rc;
  for (int c = 0; c < nchunks; c++) {
    const int b = c & 1, t0 = c * chunk, cnt = std::min(chunk, n_sweeps - t0);
    CFEAR_HIP_CHECK(ctx, hipStreamWaitEvent(ctx->stream, o->rp_filt[b], 0));
    // odometrykeyframefuser.cpp:143-259 sweep after sweep. Few sequences: one persistent workgroup per sequence walks the whole
    // chunk (no launch in between; a workgroup needs a compute unit's LDS to itself, so this pays while the sequences fit the
    // chip at one per compute unit). Many sequences: the batched kernels, two launches per sweep, whose occupancy is what counts.
    OP.cs.cov_out = d_cov6 ? d_cov6 + (size_t)t0 * o->B * 36 : nullptr;  // (the persistent kernels step it on per sweep)
    if (persistent && cfar) {
      cfear_launch_replay_chunk_cloud(o->rp_cloud[b], o->cap_points, o->rp_cloud_n[b], cnt, o->B, OP, o->d_states, o->d_scratch_hdr, o->d_cov_work, o->d_summaries,
                                      o->d_poses_out, d_records ? d_records + (size_t)t0 * o->B : nullptr, ctx->stream);
    } else if (persistent) {
      cfear_launch_replay_chunk(o->rp_slots[b], cnt, o->B, ctx->d_trig, OP, o->d_states, o->d_scratch_hdr, o->d_cov_work, o->d_summaries,
                                o->d_poses_out, d_records ? d_records + (size_t)t0 * o->B : nullptr, ctx->stream);
    } else {
      for (int t = 0; t < cnt; t++) {
        OP.records = d_records ? d_records + (size_t)(t0 + t) * o->B : nullptr;
        OP.cs.cov_out = d_cov6 ? d_cov6 + (size_t)(t0 + t) * o->B * 36 : nullptr;
        const SweepPoints src = cfar ? SweepPoints::of_clouds(o->rp_cloud[b] + 3 * slots * (size_t)t, o->cap_points, o->rp_cloud_n[b] + (size_t)o->B * t)
                                     : SweepPoints::of_slots(o->rp_slots[b] + slots * (size_t)t);
        CFEAR_TRY(odo_launch_sweep(ctx, o, OP, src, o->B, ctx->stream, false));  // (no stage events, whatever the profile says)
      }
    }
    CFEAR_HIP_CHECK(ctx, hipEventRecord(o->rp_used[b], ctx->stream));
    o->rp_used_pending[b] = true;
    o->step_no += cnt; o->sweeps += cnt;
    if (c + 1 < nchunks && (rc = stage(c + 1)) != CFEAR_OK) return rc;  // (queued after this chunk's launches: a copy from pageable memory blocks the host)
  }
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  return CFEAR_OK;
}
static int replay_impl(cfear_ctx* ctx, cfear_odometry* o, const uint8_t* frames, bool on_device, int n_sweeps, cfear_sweep_record* d_records,
                       double* d_cov6) {
  const int rc = replay_impl_queue(ctx, o, frames, on_device, n_sweeps, d_records, d_cov6);
  if (rc != CFEAR_OK && o->rp_stream) {
    // an error after work was queued: copies out of the caller's frames and kernels that read them may be in flight - nothing of
    // this call is left running when it returns (the error text is kept)
    const std::string keep = ctx->err;
    (void)hipStreamSynchronize(o->rp_stream);
    (void)hipStreamSynchronize(ctx->stream);
    ctx->err = keep;
  }
  return rc;
}

static int replay_check(cfear_ctx* ctx, cfear_odometry* o, const uint8_t* frames, int n_sweeps) {
  if (!ctx || !o || !frames || n_sweeps <= 0) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_replay: bad argument");
  CFEAR_TRY(odo_shape_check(ctx, o, "odometry_replay"));
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  CFEAR_TRY(odo_seq_sync(ctx, o, "odometry_replay"));
  CFEAR_TRY(odo_peaks_check(ctx, o, "odometry_replay"));
  // CA-CFAR reads the images as dwords: every chunk of the replay starts a whole number of sweeps (of B images, or of the sources the sequences'
  // detectors share) after `frames`, so the base and the sweep size decide the alignment of all of them - refused here, before any chunk has
  // advanced the sequences' state
  if (o->filter == CFEAR_FILTER_CACFAR && ((reinterpret_cast<uintptr_t>(frames) & 3) != 0 || (n_sweeps > 1 && (((size_t)odo_sources(o) * ctx->A * ctx->R) & 3) != 0)))
    return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_replay: filter_type CA-CFAR needs a 4-byte aligned recording and B * A * R a multiple of 4 (the detector reads whole "
                      "dwords; B: the input sweeps per step)");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return odo_join(ctx, o);
}

int cfear_odometry_replay_host_cov(cfear_ctx* ctx, cfear_odometry* o, const uint8_t* h_frames, int n_sweeps, cfear_sweep_record* records, double* cov6) {
  int rc = replay_check(ctx, o, h_frames, n_sweeps);
  if (rc != CFEAR_OK) return rc;
  if (records && (rc = replay_ensure(ctx, o, 0, false, (size_t)n_sweeps * o->B)) != CFEAR_OK) return rc;
  const size_t ncov = cov6 ? (size_t)n_sweeps * o->B * 36 : 0;
  if (ncov > o->d_cov_seq.size()) {
    CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    CFEAR_TRY(o->d_cov_seq.ensure(ctx, ncov, "hipMalloc per-sweep covariances"));
  }
  rc = replay_impl(ctx, o, h_frames, false, n_sweeps, records ? o->d_records : nullptr, cov6 ? o->d_cov_seq : nullptr);
  if (rc != CFEAR_OK) return rc;
  if (records) CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(records, o->d_records, sizeof(cfear_sweep_record) * (size_t)n_sweeps * o->B, hipMemcpyDeviceToHost, ctx->stream));
  if (cov6) CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(cov6, o->d_cov_seq, sizeof(double) * ncov, hipMemcpyDeviceToHost, ctx->stream));
  CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return odo_capacity_check(ctx, o, "odometry_replay_host");
}
int cfear_odometry_replay_host(cfear_ctx* ctx, cfear_odometry* o, const uint8_t* h_frames, int n_sweeps, cfear_sweep_record* records) {
  return cfear_odometry_replay_host_cov(ctx, o, h_frames, n_sweeps, records, nullptr);
}

int cfear_odometry_replay_device_cov(cfear_ctx* ctx, cfear_odometry* o, const uint8_t* d_frames, int n_sweeps, cfear_sweep_record* d_records, double* d_cov6) {
  const int rc = replay_check(ctx, o, d_frames, n_sweeps);
  if (rc != CFEAR_OK) return rc;
  return replay_impl(ctx, o, d_frames, true, n_sweeps, d_records, d_cov6);  // asynchronous: nothing is waited for
}
int cfear_odometry_replay_device(cfear_ctx* ctx, cfear_odometry* o, const uint8_t* d_frames, int n_sweeps, cfear_sweep_record* d_records) {
  return cfear_odometry_replay_device_cov(ctx, o, d_frames, n_sweeps, d_records, nullptr);
}

// ---- the plain reads: what the last sweep left, through the context stream ---------------------------------------------------------------
int cfear_odometry_poses(cfear_ctx* ctx, cfear_odometry* o, double* poses_xyt) {
  if (!ctx || !o || !poses_xyt) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_poses: bad argument");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  CFEAR_TRY(odo_join(ctx, o));
  CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(poses_xyt, o->d_poses_out, sizeof(double) * 3 * (size_t)o->B, hipMemcpyDeviceToHost, ctx->stream));
  CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return odo_capacity_check(ctx, o, "odometry_poses");
}

int cfear_odometry_covariances(cfear_ctx* ctx, cfear_odometry* o, double* cov6) {
  if (!ctx || !o || !cov6) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_covariances: bad argument");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  CFEAR_TRY(odo_join(ctx, o));
  CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(cov6, o->d_cov_work, sizeof(double) * 36 * (size_t)o->B, hipMemcpyDeviceToHost, ctx->stream));
  CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return odo_capacity_check(ctx, o, "odometry_covariances");
}

int cfear_odometry_status(cfear_ctx* ctx, cfear_odometry* o, int32_t* per_sequence) {
  if (!ctx || !o) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_status: bad argument");
  CFEAR_TRY(odo_drain(ctx, o));
  if (per_sequence) {
    if (o->d_flags) CFEAR_HIP_CHECK(ctx, hipMemcpy(per_sequence, o->d_flags + 1, sizeof(int) * (size_t)o->B, hipMemcpyDeviceToHost));
    else memset(per_sequence, 0, sizeof(int) * (size_t)o->B);
  }
  return odo_capacity_check(ctx, o, "odometry_status");
}

int cfear_odometry_summary(cfear_ctx* ctx, cfear_odometry* o, int sequence, cfear_reg_summary* summary, int* n_cells,
                           int* n_keyframes) {
  if (!ctx || !o || sequence < 0 || sequence >= o->B) return cfear_fail(ctx, CFEAR_ERR_INVALID, "odometry_summary: bad argument");
  CFEAR_TRY(odo_drain(ctx, o));
  if (summary) CFEAR_HIP_CHECK(ctx, hipMemcpy(summary, o->d_summaries + sequence, sizeof(cfear_reg_summary), hipMemcpyDeviceToHost));
  if (n_cells || n_keyframes) {
    SeqState st;
    CFEAR_HIP_CHECK(ctx, hipMemcpy(&st, o->d_states + sequence, sizeof(st), hipMemcpyDeviceToHost));
    if (n_keyframes) *n_keyframes = st.nkf;
    if (n_cells) {  // cells of the scan built by the last step
      ScanDev h;
      CFEAR_HIP_CHECK(ctx, hipMemcpy(&h, o->d_scans + o->scan_stride * ((size_t)sequence * o->nslots + st.last_slot), sizeof(h), hipMemcpyDeviceToHost));
      *n_cells = h.n_cells;
    }
  }
  return odo_capacity_check(ctx, o, "odometry_summary");
}

}  // extern "C"
