// odometry_obj.h -- the batched odometry object (cfear_odometry) and the few helpers that more than one translation unit needs:
// pipeline.hip (the step's kernels and the launch layer that names them, the object's scan and scratch blocks over scan_layout.h),
// odometry_run.hip (the object's life: creation, reset, destruction, the steps, the profile, the replay, and the plain reads: poses,
// covariances, status, summary), odometry_seq.hip (the per-sequence configuration: setters, getters, the device table), odometry_cov.hip
// (the cost-sampling and surface routes over the registrations' records) and keyframes.hip (the keyframe graph: its four kernels, its
// setters and its reading routes over KeyframeLog, keyframe_dev.h). The middle three hold no kernel.
#pragma once
#include <memory>

#include "common.h"
#include "odometry_step_dev.h"
#include "surface_dev.h"
#include "seq_config.h"
#include "keyframe_dev.h"

struct cfear_cfar_grid_delete { void operator()(cfear_cfar_grid* g) const { cfear_cfar_grid_destroy(g); } };
typedef std::unique_ptr<cfear_cfar_grid, cfear_cfar_grid_delete> cfear_cfar_grid_ptr;

// The timing events of a profiled object: created in blocks of 1024 outside any timed region (cfear_odometry_profile; a run that outlasts
// them grows the pool where it stands), handed out in order, all of them free again after reset().
struct EventPool {
  std::vector<Event> events;
  size_t used = 0;
  int grow(cfear_ctx* ctx) {
    for (int i = 0; i < 1024; i++) {
      Event e;
      CFEAR_TRY(e.ensure(ctx, hipEventDefault, "hipEventCreate(&e)"));
      events.push_back(std::move(e));
    }
    return CFEAR_OK;
  }
  // the next event, appended to `list` and recorded on `st`
  int take(cfear_ctx* ctx, hipStream_t st, std::vector<hipEvent_t>& list) {
    if (used == events.size()) CFEAR_TRY(grow(ctx));
    hipEvent_t e = events[used++];
    list.push_back(e);
    CFEAR_HIP_CHECK(ctx, hipEventRecord(e, st));
    return CFEAR_OK;
  }
  void reset() { used = 0; }
};

// Members are destroyed last first, and the order below is chosen for that: the events (the last block), then the streams, then the
// device buffers and the detectors' grid. cfear_odometry_destroy drains the streams and takes them out of the context's list first.

struct cfear_odometry {
  int B = 0, nslots = 0, cap_points = 0, cap_cells = 0, pair_cap = 0;
  DevBuf<int> d_order; DevBuf<unsigned> d_work;  // registration workgroups longest first (cfear_tune REGISTRATION_ORDER): see order_kernel
  bool order_ready = false;  // d_work holds the keys of a registration launch
  bool with_kd = false;  // the scans carry FLANN kd-tree arrays (cfear_tune NN_TIE_RULE = 2 at creation)
  int large_kernel = 0, n_cus = 256;  // cfear_tune LARGE_SUBMAP_KERNEL at creation; compute units of the device
  DevBuf<int> d_flags;  // bit 0: a scan had more cells than cap_cells, bit 1: a cloud had more points than cap_points (only allocated when either can happen)
  DevBuf<unsigned char> d_scans;       // B * nslots flat scan blocks
  size_t scan_stride = 0;              // bytes between consecutive scan slots of d_scans
  DevBuf<unsigned char> d_scratch;     // B scratch blocks
  DevBuf<BlockScratch> d_scratch_hdr;
  DevBuf<SeqState> d_states;
  DevBuf<double> d_cov_work;
  DevBuf<cfear_reg_summary> d_summaries;
  DevBuf<double> d_poses_out;
  DevBuf<uint32_t> d_slots[2];  // filter output, double-buffered: the filter runs one sweep ahead
  DevBuf<uint8_t> d_polar;  // staging for step_host
  // filter_type CA-CFAR (radar_driver.cpp:52-56): the filter's output is a cloud per sequence instead of A * k slots
  int filter = CFEAR_FILTER_KSTRONG;
  DevBuf<float> d_cloud;         // [B][cap_points][3]
  DevBuf<int> d_cloud_n;         // [B] detections per sequence (may exceed cap_points: the cloud keeps the first cap_points)
  DevBuf<int> d_cfar_rows;       // row counts / row bases / hit masks of one sweep (cfear_cfar_scratch_ints)
  DevBuf<float> rp_cloud[2];     // replay: clouds of a chunk of sweeps, double-buffered like rp_slots
  DevBuf<int> rp_cloud_n[2];
  DevBuf<int> rp_cfar_rows;      // ... of a chunk (the replay stream runs one filter at a time)
  // cfear_odometry_replay_host: chunks of sweeps are copied and filtered on a stream of their own (rp_stream), two chunks
  // in flight (staging + slots double-buffered), while the context stream runs features -> registration sweep after sweep
  DevBuf<uint8_t> rp_polar[2];
  DevBuf<uint32_t> rp_slots[2];
  bool rp_used_pending[2] = {false, false};
  int rp_chunk = 0;            // sweeps per chunk the slot buffers are sized for
  int rp_polar_chunk = 0;      // ... and the staging buffers (allocated on the first replay from host memory only)
  DevBuf<cfear_sweep_record> d_records;
  DevBuf<long long> d_phase_times;  // optional [B][32] (cfear_odometry_phase_times)
  int phase_detail = 1;
  bool wg_only = false;  // the table only receives the workgroups' start / end clocks, from the production kernels
  // The filter of a sweep needs nothing but its input, and it is bound by HBM while features / registration are chains
  // of short dependent phases. With overlap on it runs on a stream of its own (sf) into the slot buffer of its parity;
  // features / registration follow on a second stream (so) once their slot buffer is written (ev_filt) and release it
  // when features has consumed it (ev_free). The host issues step t+1 while so still works on step t, so filter(t+1)
  // can start on compute units that the last rounds of registration(t) leave idle. The context stream joins in the
  // reading calls (odo_join). With overlap off (the default, see DESIGN.md: the three kernels want the same registers and
  // LDS of a compute unit, so running them side by side stretches all of them) they run in turn on the context stream.
  int overlap = 0;  // 0: the three kernels in turn on the context stream; n >= 1: filter stream + n odometry streams (below)
  long long step_no = 0;
  // overlap = n: the filter runs on a LOW-priority stream of its own (sf) into the slot buffer of its parity, one sweep ahead;
  // the sequences are cut into n contiguous ranges whose features / registration kernels run on n HIGH-priority streams
  // (so[i]). Different ranges are at different points of their features -> registration chain, so the ragged last round of one
  // kernel is filled with workgroups of another (a features workgroup and a registration workgroup fit a compute unit
  // together), and the filter takes what is left.
  bool filt_pending[2] = {false, false};  // ev_filt / ev_free have been recorded at least once
  // profiling: timing events taken from a pool that is created up front (and grown in blocks)
  bool profile = false;
  std::vector<hipEvent_t> filter_events;  // 2 per profiled filter launch (borrowed from the pool, `timers` below)
  std::vector<hipEvent_t> stage_events;   // 3 per profiled step: before features, between, after registration
  // estimate_cov_by_sampling (cfear_odometry_set_cov_sampling): the sampling stage runs after every registration while cov_on
  bool cov_on = false;
  int cov_m = 0;                          // samples per sweep (samples_per_axis^3)
  double cov_scaler = 4.0;
  DevBuf<CovSampleCtx> d_cov_ctx;         // [B] what each registration used (register_step_body)
  DevBuf<double> d_cov_design;            // [10][m] pseudo-inverse of the sample design, then [m][3] sample offsets
  DevBuf<double> d_cov_costs;             // [B][m] sampled costs of the last sweep
  DevBuf<double> d_cov_seq;               // cfear_odometry_replay_host_cov: cov_current of every sweep ([n][B][36])
  // cost surfaces (cfear_odometry_set_surface_recording / cfear_odometry_surface): the registration records what it used in d_cov_ctx
  // (as for the sampling stage, which does not run unless cov_on)
  bool surf_on = false;
  bool surf_ready = false;  // d_cov_ctx holds the last step's registrations (a step ran with recording since the last reset / replay)
  DevBuf<SurfHdr> d_surf_hdr;        // [B]
  DevBuf<double> d_surf_coords;      // [B][2][pixels]
  DevBuf<int> d_surf_nxy;            // [B][2]
  // what the sequences run with (seq_config.h): parameter rows, source map, shapes, detectors, fuser options - replaced as a whole by
  // odo_commit_config (odometry_seq.hip), which also rebuilds what the device and the launches read of it:
  cfear_seq_config cfg;
  DevBuf<SeqParams> d_seq;             // [B] what the kernels read (OdoParams::seq); exists while cfg.needs_table()
  cfear_params seq_par_seen;           // the context's parameters d_seq was built and the rows were checked against
  int seq_zmin = -1;                   // the filter's threshold, cfg.filter_zmin(): the smallest z_min of the rows (-1: the context's)
  // per-sequence cost and submap size: the registration stage runs as one launch per group
  cfear_seq_groups groups;             // the launch groups of cfg.shapes (seq_groups.h), built with the device table
  DevBuf<int> d_group_list;            // [B] groups.list: what OdoParams::order points into until a sweep's work keys exist
  DevBuf<int> d_seq_group;             // [B] groups.group (order_groups_kernel)
  // per-sequence CA-CFAR detectors over shared sweeps: the filter stage runs cfear_launch_cfar_grid
  cfear_cfar_grid_ptr det_grid;        // the plan and device tables of cfg.dets and their source map (destroyed with the object: its streams are idle then)
  long long sweeps = 0;               // sweeps processed since cfear_odometry_create / cfear_odometry_reset
  // the keyframe graph (cfear_odometry_set_keyframe_recording / _clouds, keyframes.hip): while kf.what != 0 the recorder stage runs behind
  // every registration stage - with a point log the cloud stage in front of it - and appends the keyframes of the sequences that fused
  KeyframeLog kf;
  // ---- streams (destroyed before everything above) ----
  Stream sf;               // overlap: the filter's
  std::vector<Stream> so;  // ... and the odometry streams
  Stream rp_stream;        // the replay's copies and filters; made by the first replay (replay_ensure), with its events
  std::vector<hipStream_t> streams() const {  // those that exist: what the context is told to wait for, and what is drained before the object goes
    std::vector<hipStream_t> all;
    if (sf) all.push_back(sf);
    for (const Stream& st : so) all.push_back(st);
    if (rp_stream) all.push_back(rp_stream);
    return all;
  }
  // ---- events (destroyed first) ----
  Event ev_in, ev_copied;
  Event ev_filt[2];
  std::vector<Event> ev_free[2], ev_done;  // per odometry stream
  Event rp_filt[2], rp_used[2];  // chunk filtered / chunk consumed by the odometry kernels
  Event rp_in;                   // device-resident frames ready on the context stream
  EventPool timers;              // what filter_events / stage_events borrow from
};
// make everything the internal streams have been given so far visible to the context stream
static int odo_join(cfear_ctx* ctx, cfear_odometry* o) {
  if (o->overlap && o->step_no > 0) {
    for (size_t i = 0; i < o->so.size(); i++) {  // an odometry stream waits for every filter it consumes: joining them joins sf
      CFEAR_HIP_CHECK(ctx, hipEventRecord(o->ev_done[i], o->so[i]));
      CFEAR_HIP_CHECK(ctx, hipStreamWaitEvent(ctx->stream, o->ev_done[i], 0));
    }
  }
  return CFEAR_OK;
}
// ... and wait for it: nothing of the object is in flight (a blocking read; before a buffer is replaced)
static int odo_drain(cfear_ctx* ctx, cfear_odometry* o) {
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  CFEAR_TRY(odo_join(ctx, o));
  CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return CFEAR_OK;
}
static int odo_sources(const cfear_odometry* o) { return o->cfg.sources(o->B); }
// what the rules of seq_config.h need to know of the object and its context (B = 0 without either: a setter's "bad argument")
static cfear_seq_object odo_seq_object(const cfear_ctx* ctx, const cfear_odometry* o) {
  cfear_seq_object O;
  if (!ctx || !o) return O;
  O.B = o->B; O.filter = o->filter; O.max_submap = o->nslots - 1; O.overlap = o->overlap != 0; O.sweeps = o->sweeps;
  O.cfg = &o->cfg; O.par = &ctx->par;
  return O;
}
// a rule of seq_config.h (`msg` is its message argument): a refusal becomes the context's error and the caller's return value
#define CFEAR_SEQ_TRY(ctx, expr)                                           \
  do {                                                                     \
    std::string msg;                                                       \
    const int _rc = (expr);                                                \
    if (_rc != CFEAR_OK) return cfear_fail((ctx), _rc, msg.c_str());       \
  } while (0)
// ---- pipeline.hip: what odometry_run.hip and odometry_cov.hip call of the launch layer ----
// the kernel parameters of one odometry step of `o` under the context's current settings
__attribute__((visibility("hidden"))) OdoParams odo_params(const cfear_ctx* ctx, const cfear_odometry* o);
// Where a sweep's points come from: the filter's slots, or clouds of `cap` points each with their counts
struct SweepPoints {
  const uint32_t* slots = nullptr;
  const float* xyi = nullptr; int cap = 0; const int* counts = nullptr;
  static SweepPoints of_slots(const uint32_t* d_slots) { SweepPoints S; S.slots = d_slots; return S; }
  static SweepPoints of_clouds(const float* d_xyi, int cap, const int* d_counts) { SweepPoints S; S.xyi = d_xyi; S.cap = cap; S.counts = d_counts; return S; }
};
// one sweep of `count` sequences from P.seq0 on, enqueued on `st`: features, then registration with the stages behind it. timed: three
// events of the profile around the two (stage_events); consumed: recorded once the last stage that reads the points has (features; on an
// object that records keyframe clouds the cloud stage behind the registration reads the slots again) (null: nothing is)
__attribute__((visibility("hidden"))) int odo_launch_sweep(cfear_ctx* ctx, cfear_odometry* o, const OdoParams& P, const SweepPoints& src, int count, hipStream_t st,
                                                           bool timed, hipEvent_t consumed = nullptr);
// the CA-CFAR stage of n_steps sweeps of every sequence into clouds of o->cap_points points each, [step][sequence]
__attribute__((visibility("hidden"))) int odo_launch_cfar(cfear_ctx* ctx, cfear_odometry* o, const uint8_t* d_polar, int n_steps, float* d_xyi, int* d_counts, int* d_rows,
                                                          hipStream_t st);
// has the object the shape the context's parameters ask for? (k_strongest / submap_scan_size / the filter cannot change under an object)
__attribute__((visibility("hidden"))) int odo_shape_check(cfear_ctx* ctx, const cfear_odometry* o, const char* what);
// after a synchronising read: an overflow of cells or points since the last one is reported, loudly, as `what`
__attribute__((visibility("hidden"))) int odo_capacity_check(cfear_ctx* ctx, cfear_odometry* o, const char* what);
// the scan and scratch layouts of an object whose capacities are set: bytes of one scan slot and of one sequence's scratch block ...
__attribute__((visibility("hidden"))) void odo_block_bytes(const cfear_odometry* o, size_t* scan_bytes, size_t* scratch_bytes);
// ... and the headers of all of them, built on the host and uploaded ("odometry state upload")
__attribute__((visibility("hidden"))) int odo_upload_headers(cfear_ctx* ctx, cfear_odometry* o, size_t scratch_bytes);
// ---- odometry_run.hip: what the keyframe setters of keyframes.hip call ----
__attribute__((visibility("hidden"))) int odo_ensure_flags(cfear_ctx* ctx, cfear_odometry* o);
// does the object's filter compute the slots' peak flag? (only for a point log with peaks clouds; refused where cfear_tune FILTER_PEAKS = 0 forbids it)
inline bool odo_filter_peaks(const cfear_odometry* o) { return o->kf.records_peaks(); }
// (a CA-CFAR object runs no k-strongest filter and its peaks cloud is empty by definition: nothing to refuse there)
inline int odo_peaks_check(cfear_ctx* ctx, const cfear_odometry* o, const char* what) {
  if (!odo_filter_peaks(o) || ctx->tune_k1_peaks != 0 || o->filter == CFEAR_FILTER_CACFAR) return CFEAR_OK;
  char msg[256];
  snprintf(msg, sizeof(msg), "%s: the object records peaks clouds (CFEAR_KF_PEAKS), which need the filter's peak flag, and cfear_tune FILTER_PEAKS = 0 forbids it: "
           "set the knob to -1 or 1, or record without CFEAR_KF_PEAKS", what);
  return cfear_fail(ctx, CFEAR_ERR_INVALID, msg);
}
// odometry_seq.hip: cfear_set_params since the device table was built - the rows are checked against the new parameters and the table follows them
__attribute__((visibility("hidden"))) int odo_seq_resync(cfear_ctx* ctx, cfear_odometry* o, const char* what);
// before a step / replay / surface call: cfear_set_params since the table was built? The rows are checked against the new parameters
// (loud, never silent) and the table follows them
static int odo_seq_sync(cfear_ctx* ctx, cfear_odometry* o, const char* what) {
  if (!o->d_seq || memcmp(&o->seq_par_seen, &ctx->par, sizeof(cfear_params)) == 0) return CFEAR_OK;
  return odo_seq_resync(ctx, o, what);
}
