// seq_config.h -- what the sequences of a batched odometry object run with, as ONE value: the five per-sequence tables
// (cfear_odometry_set_sequence_params / _sources / _shapes / _detectors, cfear_odometry_set_fuser_options), the one accessor that answers
// "what does sequence q run with?", the facts the launch layer derives from the tables, and every rule a setter refuses by. Host arithmetic
// only (no device, no context): shared by odometry_seq.hip (the setters and the one commit path), pipeline.hip (the step and replay
// launches), odometry_cov.hip (the surface route) and host/seq_config_check (tests/test_seq_config_cpu.py).
//
// A setter is one cfear_seq_set_* call - the call's checks, a candidate that is the object's configuration with one table replaced, the
// consistency check of the candidate - and the commit of the candidate (odo_commit_config); a refused candidate never touches the object.
// The content of detector rows is checked where their plan is built (cfear_cfar_grid_create, cfar.hip).
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/cfear_hip.h"
#include "seq_groups.h"

struct cfear_seq_config {
  // "not set" is an empty vector, everywhere
  std::vector<cfear_params> rows;         // [B] the caller's table; empty: every sequence runs with the context's parameters
  std::vector<int32_t> src;               // [B] the sweep each sequence reads (k-strongest objects); empty: sweep q for sequence q
  int n_sources = 0;                      // sweeps per step with a source map - src's, or the detectors' (0: B)
  std::vector<cfear_seq_shape> shapes;    // [B]; empty: the context's cost and submap_scan_size
  std::vector<cfear_seq_detector> dets;   // [B] (CA-CFAR objects); empty: the context's detector
  bool dets_mapped = false;               // the detectors came with a source map (the clouds stay one per sequence, so src stays empty)
  std::vector<cfear_fuser_options> fuser;  // [B]; empty: the defaults (no prior, constant-velocity guess)

  // what sequence q runs with: par carries the sequence's own cost, submap_scan_size and detector fields
  struct effective_t {
    cfear_params par;
    int source;  // the sweep of a step's input it reads
    cfear_fuser_options fuser;
  };
  // the shape's and the detector's fields of sequence q over p, where those tables are set
  void override_shape_and_detector(cfear_params& p, int q) const {
    if (!shapes.empty()) { p.cost = shapes[(size_t)q].cost; p.submap_scan_size = shapes[(size_t)q].submap_scan_size; }
    if (!dets.empty()) {
      const cfear_seq_detector& d = dets[(size_t)q];
      p.cfar_window_size = d.window_size; p.cfar_nb_guard_cells = d.nb_guard_cells; p.cfar_false_alarm_rate = d.false_alarm_rate; p.z_min = d.z_min;
    }
  }
  effective_t effective(int q, const cfear_params& ctx_par) const {
    effective_t e;
    e.par = rows.empty() ? ctx_par : rows[(size_t)q];
    override_shape_and_detector(e.par, q);
    e.source = src.empty() ? q : src[(size_t)q];
    if (fuser.empty()) { e.fuser.soft_constraint = 0; e.fuser.use_guess = 1; }  // (cfear_default_fuser_options)
    else e.fuser = fuser[(size_t)q];
    return e;
  }
  // the detector of sequence q: its own, or the context's (whatever the rows say: on a k-strongest object a row's z_min is the filter's)
  cfear_seq_detector detector(int q, const cfear_params& c) const {
    if (!dets.empty()) return dets[(size_t)q];
    cfear_seq_detector d;
    d.window_size = c.cfar_window_size; d.nb_guard_cells = c.cfar_nb_guard_cells; d.false_alarm_rate = c.cfar_false_alarm_rate; d.z_min = c.z_min;
    return d;
  }
  // do the kernels need a device table (OdoParams::seq)? The detectors alone need none: they act in the filter stage
  bool needs_table() const { return !rows.empty() || !src.empty() || !fuser.empty() || !shapes.empty(); }
  // the threshold of the one k-strongest pass all sequences share: the smallest z_min of the rows as the filter takes it
  // (radar_filters.cpp:198, :212); -1: the context's
  int filter_zmin() const {
    if (rows.empty()) return -1;
    int zmin = 255;
    for (const cfear_params& r : rows) zmin = std::min(zmin, (int)(uint8_t)(int)r.z_min);
    return zmin;
  }
  // input sweeps per step
  int sources(int B) const { return n_sources > 0 ? n_sources : B; }
  // the first sequence whose shape has another cost than sequence 0's; 0: one cost (or no shapes)
  int other_cost() const {
    for (size_t q = 1; q < shapes.size(); q++)
      if (shapes[q].cost != shapes[0].cost) return (int)q;
    return 0;
  }
  // the launch groups of the shapes (seq_groups.h); false: a cost or submap_scan_size that is none
  bool groups(int small_scans, cfear_seq_groups& G) const {
    std::vector<int> cost(shapes.size()), sub(shapes.size());
    for (size_t q = 0; q < shapes.size(); q++) { cost[q] = shapes[q].cost; sub[q] = shapes[q].submap_scan_size; }
    return cfear_seq_groups_build(cost.data(), sub.data(), (int)shapes.size(), small_scans, G);
  }
};

// what the rules need to know of the object and its context (B = 0, null pointers: no object or no context - every setter's "bad argument")
struct cfear_seq_object {
  int B = 0;                          // n_sequences
  int filter = CFEAR_FILTER_KSTRONG;  // filter_type at creation
  int max_submap = 0;                 // the submap_scan_size the object is sized for (its scan slots - 1)
  bool overlap = false;               // runs its sequences as index ranges on overlap streams
  long long sweeps = 0;               // processed since cfear_odometry_create / cfear_odometry_reset
  const cfear_seq_config* cfg = nullptr;  // the object's configuration as it stands
  const cfear_params* par = nullptr;      // the context's parameters
};

// ---- the rules: each returns a code and, refusing, the message ----------------------------------------------------------------------------
// Inside a setter the order is: bad argument, the object's kind (CFEAR_ERR_UNSUPPORTED), sweeps already processed, content, then
// cfear_seq_config_check of the candidate. (N: the size of the buffer the message was always formatted into.)
inline int cfear_seq_refuse(std::string& msg, int code, const char* text) { msg = text; return code; }
template <size_t N, typename... Args>
inline int cfear_seq_refuse(std::string& msg, int code, const char* fmt, Args... args) {
  char buf[N];
  snprintf(buf, sizeof(buf), fmt, args...);
  return cfear_seq_refuse(msg, code, buf);
}

inline int cfear_seq_fresh_check(const cfear_seq_object& O, const char* what, std::string& msg) {
  if (O.sweeps == 0) return CFEAR_OK;
  return cfear_seq_refuse<256>(msg, CFEAR_ERR_INVALID, "%s: the object has processed %lld sweeps since cfear_odometry_create / cfear_odometry_reset - keyframes built under other parameters or "
                               "from other sweeps are not a state the reference can be in; call cfear_odometry_reset first", what, O.sweeps);
}

// the content of one row of the table: the values cfear_set_params would refuse
inline int cfear_seq_row_check(const cfear_params& r, int q, const char* what, std::string& msg) {
  const char* bad = nullptr;
  if (!(r.res > 0.05) || !std::isfinite(r.res)) bad = "res must be finite and > 0.05";
  else if (r.loss < 0 || r.loss > 5) bad = "unknown loss";
  else if (r.max_itr_association < 1 || r.max_itr_association > CFEAR_MAX_OUTER) bad = "max_itr_association must be in 1..64";
  else if (r.max_solver_iterations < 1) bad = "max_solver_iterations must be >= 1";
  else if (r.min_itr < 0) bad = "min_itr must be >= 0";
  else if (!std::isfinite(r.z_min) || !std::isfinite(r.loss_limit)) bad = "z_min and loss_limit must be finite";
  return bad ? cfear_seq_refuse<160>(msg, CFEAR_ERR_INVALID, "%s: row %d: %s", what, q, bad) : CFEAR_OK;
}

// THE consistency check of a whole candidate: may its rows be the sequences of the object under the context's parameters, beside its
// shapes and detectors? The fields that size memory or select a kernel are the object's; cost / submap_scan_size are the sequence's shape's
// and the detector fields the sequence's detector's where those are set. (The source map and the fuser options take part in no rule.)
inline int cfear_seq_config_check(const cfear_seq_config& C, const cfear_seq_object& O, const char* what, std::string& msg) {
  const cfear_params& c = *O.par;
  const bool shapes = !C.shapes.empty(), dets = !C.dets.empty();
  for (int q = 0; q < (int)C.rows.size(); q++) {
    const cfear_params& r = C.rows[(size_t)q];
    cfear_params want = c;  // what the row must carry: the context's values, the shape's, the detector's
    C.override_shape_and_detector(want, q);
    // k_strongest: any k up to the context's K. The filter runs with K and the object is sized for it; a sequence reads the last k of the
    // returns the filter kept of every bearing (cloud_step_block)
    if (r.k_strongest < 1 || r.k_strongest > c.k_strongest)
      return cfear_seq_refuse<256>(msg, CFEAR_ERR_INVALID, "%s: row %d: k_strongest = %d must be in 1..%d, the context's k_strongest (the filter runs with it and the object's memory is sized "
                                   "for it)", what, q, r.k_strongest, c.k_strongest);
    const char* f = nullptr;
    if (O.filter == CFEAR_FILTER_CACFAR && r.k_strongest != c.k_strongest) f = "k_strongest (the CA-CFAR detector has no k)";
    else if (r.cost != want.cost) f = shapes ? "cost (the sequence's shape says otherwise: cfear_odometry_set_sequence_shapes)" : "cost";
    else if (r.submap_scan_size != want.submap_scan_size) f = shapes ? "submap_scan_size (the sequence's shape says otherwise: cfear_odometry_set_sequence_shapes)" : "submap_scan_size";
    else if (r.filter_type != c.filter_type) f = "filter_type";
    else if (r.range_res != c.range_res) f = "range_res";
    else if (r.min_distance != c.min_distance) f = "min_distance";
    else if (r.downsample_factor != c.downsample_factor) f = "downsample_factor";
    else if (r.radar_ccw != c.radar_ccw) f = "radar_ccw";
    else if (r.assoc_radius != c.assoc_radius) f = "assoc_radius";
    else if (r.cfar_window_size != want.cfar_window_size) f = dets ? "cfar_window_size (the sequence's detector says otherwise: cfear_odometry_set_sequence_detectors)" : "cfar_window_size";
    else if (r.cfar_nb_guard_cells != want.cfar_nb_guard_cells) f = dets ? "cfar_nb_guard_cells (the sequence's detector says otherwise: cfear_odometry_set_sequence_detectors)" : "cfar_nb_guard_cells";
    else if (r.cfar_false_alarm_rate != want.cfar_false_alarm_rate) f = dets ? "cfar_false_alarm_rate (the sequence's detector says otherwise: cfear_odometry_set_sequence_detectors)" : "cfar_false_alarm_rate";
    else if (r.cfar_max_points != c.cfar_max_points) f = "cfar_max_points";
    else if (r.cfar_max_distance != c.cfar_max_distance) f = "cfar_max_distance";
    else if (O.filter == CFEAR_FILTER_CACFAR && r.z_min != want.z_min)
      f = dets ? "z_min (the sequence's detector says otherwise: cfear_odometry_set_sequence_detectors)" : "z_min (the CA-CFAR detector's static threshold)";
    if (f)
      return cfear_seq_refuse<640>(msg, CFEAR_ERR_INVALID, "%s: row %d differs from the context's parameters in %s, which sizes memory or selects a kernel for the whole object "
                                   "(cost and submap_scan_size per sequence: cfear_odometry_set_sequence_shapes; per-sequence: z_min, k_strongest (<= the context's), res, weight_intensity, loss, loss_limit, weight_opt, covar_scale, regularization, compensate, "
                                   "the keyframe rule, the iteration limits)", what, q, f);
    const int rc = cfear_seq_row_check(r, q, what, msg);
    if (rc != CFEAR_OK) return rc;
  }
  return CFEAR_OK;
}

// ---- the setters: the call's checks, then `cand` = the object's configuration with the one table replaced, then its consistency ---------
// cfear_odometry_set_sequence_params (the rows' content is cfear_seq_config_check's, row by row beside the other tables)
inline int cfear_seq_set_params(const cfear_params* rows, int n_rows, const cfear_seq_object& O, cfear_seq_config& cand, std::string& msg) {
  if (O.B <= 0 || (rows && n_rows != O.B))
    return cfear_seq_refuse(msg, CFEAR_ERR_INVALID, "odometry_set_sequence_params: bad argument (n_rows must be the object's n_sequences)");
  const int rc = cfear_seq_fresh_check(O, "odometry_set_sequence_params", msg);
  if (rc != CFEAR_OK) return rc;
  cand = *O.cfg;
  cand.rows.assign(rows, rows + (rows ? n_rows : 0));
  return cfear_seq_config_check(cand, O, "odometry_set_sequence_params", msg);
}

// cfear_odometry_set_sequence_sources
inline int cfear_seq_set_sources(const int32_t* source, int n_sequences, int n_sources, const cfear_seq_object& O, cfear_seq_config& cand, std::string& msg) {
  if (O.B <= 0 || (source && (n_sequences != O.B || n_sources < 1 || n_sources > O.B)))
    return cfear_seq_refuse(msg, CFEAR_ERR_INVALID, "odometry_set_sequence_sources: bad argument (n_sequences must be the object's, 1 <= n_sources <= n_sequences)");
  const int rc = cfear_seq_fresh_check(O, "odometry_set_sequence_sources", msg);
  if (rc != CFEAR_OK) return rc;
  if (source && O.filter == CFEAR_FILTER_CACFAR)
    return cfear_seq_refuse(msg, CFEAR_ERR_UNSUPPORTED, "odometry_set_sequence_sources: filter_type CA-CFAR objects take one sweep per sequence (the detector's clouds are "
                            "per sequence); source maps are for k-strongest objects");
  for (int q = 0; source && q < n_sequences; q++)
    if (source[q] < 0 || source[q] >= n_sources)
      return cfear_seq_refuse<160>(msg, CFEAR_ERR_INVALID, "odometry_set_sequence_sources: source[%d] = %d is outside [0, %d)", q, (int)source[q], n_sources);
  cand = *O.cfg;
  cand.src.assign(source, source + (source ? n_sequences : 0));
  cand.n_sources = source ? n_sources : 0;
  return CFEAR_OK;
}

// cfear_odometry_set_sequence_shapes
inline int cfear_seq_set_shapes(const cfear_seq_shape* shapes, int n_rows, const cfear_seq_object& O, cfear_seq_config& cand, std::string& msg) {
  if (O.B <= 0 || (shapes && n_rows != O.B))
    return cfear_seq_refuse(msg, CFEAR_ERR_INVALID, "odometry_set_sequence_shapes: bad argument (n_rows must be the object's n_sequences)");
  if (shapes && O.overlap)
    return cfear_seq_refuse(msg, CFEAR_ERR_UNSUPPORTED, "odometry_set_sequence_shapes: the object runs its sequences as index ranges on overlap streams (cfear_tune "
                            "ODOMETRY_OVERLAP at creation); shapes run as one registration launch per group of sequences and are for objects without them");
  const int rc = cfear_seq_fresh_check(O, "odometry_set_sequence_shapes", msg);
  if (rc != CFEAR_OK) return rc;
  const int S = O.max_submap;
  for (int q = 0; shapes && q < n_rows; q++) {
    if (shapes[q].cost != CFEAR_COST_P2P && shapes[q].cost != CFEAR_COST_P2L && shapes[q].cost != CFEAR_COST_P2D)
      return cfear_seq_refuse<256>(msg, CFEAR_ERR_INVALID, "odometry_set_sequence_shapes: row %d: cost = %d is no cost metric (CFEAR_COST_P2P / _P2L / _P2D)", q, (int)shapes[q].cost);
    if (shapes[q].submap_scan_size < 1 || shapes[q].submap_scan_size > S)
      return cfear_seq_refuse<256>(msg, CFEAR_ERR_INVALID, "odometry_set_sequence_shapes: row %d: submap_scan_size = %d must be in 1..%d, the submap_scan_size the object was created "
                                   "with (its scan slots and scratch are sized for it)", q, (int)shapes[q].submap_scan_size, S);
  }
  cand = *O.cfg;
  cand.shapes.assign(shapes, shapes + (shapes ? n_rows : 0));
  // a table whose rows would then disagree with their shapes (NULL: with the context's values again)
  return cfear_seq_config_check(cand, O, "odometry_set_sequence_shapes", msg);
}

// cfear_odometry_set_sequence_detectors in two steps, the content of the detectors (cfear_cfar_grid_create) between them: the call ...
inline int cfear_seq_detectors_call_check(const cfear_seq_detector* dets, int n_rows, const int32_t* source, int n_sources, const cfear_seq_object& O, const char* what,
                                          std::string& msg) {
  if (O.B <= 0) return cfear_seq_refuse(msg, CFEAR_ERR_INVALID, "odometry_set_sequence_detectors: bad argument");
  if (O.filter != CFEAR_FILTER_CACFAR)
    return cfear_seq_refuse(msg, CFEAR_ERR_UNSUPPORTED, "odometry_set_sequence_detectors: the object runs the k-strongest filter (filter_type at creation); detectors are for "
                            "filter_type CA-CFAR objects (per-sequence k_strongest and z_min: cfear_odometry_set_sequence_params, shared sweeps: cfear_odometry_set_sequence_sources)");
  if (dets && n_rows != O.B) return cfear_seq_refuse<200>(msg, CFEAR_ERR_INVALID, "%s: n_rows = %d must be the object's n_sequences = %d", what, n_rows, O.B);
  if (dets && source && (n_sources < 1 || n_sources > O.B))
    return cfear_seq_refuse<200>(msg, CFEAR_ERR_INVALID, "%s: n_sources = %d must be in 1..%d, the object's n_sequences", what, n_sources, O.B);
  return cfear_seq_fresh_check(O, what, msg);
}
// ... and the candidate: a table whose rows would then disagree with their detectors is refused (NULL: with the context's values again).
// The clouds stay one per sequence, so the configuration's own source map stays empty: n_sources is the detectors'
inline int cfear_seq_set_detectors(const cfear_seq_detector* dets, int n_rows, const int32_t* source, int n_sources, const cfear_seq_object& O, const char* what,
                                   cfear_seq_config& cand, std::string& msg) {
  cand = *O.cfg;
  cand.dets.assign(dets, dets + (dets ? n_rows : 0));
  cand.dets_mapped = dets && source;
  cand.n_sources = cand.dets_mapped ? n_sources : 0;
  return cfear_seq_config_check(cand, O, what, msg);
}

// cfear_odometry_set_fuser_options: one row is every sequence's; all rows at the defaults (or none) leave no table, the object as it was
// before any call
inline int cfear_seq_set_fuser(const cfear_fuser_options* rows, int n_rows, const cfear_seq_object& O, cfear_seq_config& cand, std::string& msg) {
  if (O.B <= 0) return cfear_seq_refuse(msg, CFEAR_ERR_INVALID, "odometry_set_fuser_options: bad argument");
  if (rows && n_rows != 1 && n_rows != O.B)
    return cfear_seq_refuse<200>(msg, CFEAR_ERR_INVALID, "odometry_set_fuser_options: n_rows = %d (1: every sequence, or the object's n_sequences = %d: row q for sequence q)", n_rows, O.B);
  const int rc = cfear_seq_fresh_check(O, "odometry_set_fuser_options", msg);
  if (rc != CFEAR_OK) return rc;
  bool defaults = true;
  for (int q = 0; rows && q < n_rows; q++) {
    const char* f = nullptr;
    int v = 0;
    if (rows[q].soft_constraint != 0 && rows[q].soft_constraint != 1) { f = "soft_constraint"; v = rows[q].soft_constraint; }
    else if (rows[q].use_guess != 0 && rows[q].use_guess != 1) { f = "use_guess"; v = rows[q].use_guess; }
    if (f) return cfear_seq_refuse<200>(msg, CFEAR_ERR_INVALID, "odometry_set_fuser_options: row %d: %s = %d (must be 0 or 1)", q, f, v);
    if (rows[q].soft_constraint != 0 || rows[q].use_guess != 1) defaults = false;
  }
  cand = *O.cfg;
  cand.fuser.clear();
  if (!defaults) for (int q = 0; q < O.B; q++) cand.fuser.push_back(rows[n_rows == 1 ? 0 : q]);
  return CFEAR_OK;
}
