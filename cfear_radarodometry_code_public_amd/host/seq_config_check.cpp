// seq_config_check: drives csrc/seq_config.h - the per-sequence configuration of a batched odometry object as one value, its accessor, its
// derived facts and the rules its setters refuse by - from a script on standard input, one command per line. Needs no GPU and no library:
// tests/test_seq_config_cpu.py drives it (a second time as an -fsanitize=address,undefined build).
//
//   object B filter max_submap overlap sweeps   the object's facts (B 0: no object)
//   ctx name=value ...                          fields of the context's parameters (they start all zero)
//   rows null | rows N, then N lines  name=value ...   (a row starts as the context's parameters)    cfear_odometry_set_sequence_params
//   sources null | sources n_sources s_0 s_1 ...                                                      cfear_odometry_set_sequence_sources
//   shapes null | shapes cost_0 submap_0 cost_1 submap_1 ...                                          cfear_odometry_set_sequence_shapes
//   dets null | dets n_sources|- N, then N lines  window guard rate z_min [source]                    cfear_odometry_set_sequence_detectors
//   fuser null | fuser soft_0 guess_0 soft_1 guess_1 ...                                              cfear_odometry_set_fuser_options
//   check what                                  cfear_seq_config_check of the configuration as it stands (the step routes' re-check)
//   dump | effective | facts
// A setter calls what odometry_seq.hip's calls - cfear_seq_set_*: the call's checks, the candidate with one table replaced, its consistency -
// and commits by assignment (the content of detector rows is cfear_cfar_grid_create's and has no part here). It answers "rc <code> <message>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>

#include "../csrc/seq_config.h"

namespace {
struct Field { const char* name; char type; size_t off; };
#define F(T, NAME) {#NAME, T, offsetof(cfear_params, NAME)}
const Field FIELDS[] = {
    F('f', z_min), F('f', range_res), F('f', min_distance), F('i', k_strongest), F('d', res), F('d', downsample_factor), F('i', weight_intensity),
    F('i', cost), F('i', loss), F('i', weight_opt), F('d', loss_limit), F('d', covar_scale), F('d', regularization), F('i', submap_scan_size),
    F('i', compensate), F('i', radar_ccw), F('i', use_keyframe), F('d', min_keyframe_dist), F('d', min_keyframe_rot_deg), F('i', max_itr_association),
    F('i', min_itr), F('i', max_solver_iterations), F('i', filter_type), F('d', assoc_radius), F('i', cfar_window_size), F('i', cfar_nb_guard_cells),
    F('f', cfar_false_alarm_rate), F('i', cfar_max_points), F('d', cfar_max_distance)};
#undef F

bool set_fields(cfear_params& p, std::istringstream& in) {
  std::string tok;
  while (in >> tok) {
    const size_t eq = tok.find('=');
    if (eq == std::string::npos) return false;
    const std::string name = tok.substr(0, eq);
    const double v = strtod(tok.c_str() + eq + 1, nullptr);
    bool found = false;
    for (const Field& f : FIELDS) {
      if (name != f.name) continue;
      char* at = reinterpret_cast<char*>(&p) + f.off;
      if (f.type == 'f') { const float x = (float)v; memcpy(at, &x, sizeof(x)); }
      else if (f.type == 'd') memcpy(at, &v, sizeof(v));
      else { const int32_t x = (int32_t)v; memcpy(at, &x, sizeof(x)); }
      found = true;
    }
    if (!found) return false;
  }
  return true;
}
void print_params(const cfear_params& p) {
  for (const Field& f : FIELDS) {
    const char* at = reinterpret_cast<const char*>(&p) + f.off;
    if (f.type == 'f') { float x; memcpy(&x, at, sizeof(x)); printf(" %s=%.9g", f.name, (double)x); }
    else if (f.type == 'd') { double x; memcpy(&x, at, sizeof(x)); printf(" %s=%.17g", f.name, x); }
    else { int32_t x; memcpy(&x, at, sizeof(x)); printf(" %s=%d", f.name, (int)x); }
  }
}
void dump(const cfear_seq_config& C) {
  printf("rows %zu\n", C.rows.size());
  for (const cfear_params& r : C.rows) { printf("row"); print_params(r); printf("\n"); }
  printf("src %d", C.n_sources);
  for (int32_t s : C.src) printf(" %d", (int)s);
  printf("\nshapes");
  for (const cfear_seq_shape& s : C.shapes) printf(" %d %d", (int)s.cost, (int)s.submap_scan_size);
  printf("\ndets %d", C.dets_mapped ? 1 : 0);
  for (const cfear_seq_detector& d : C.dets) printf(" %d %d %.9g %.9g", (int)d.window_size, (int)d.nb_guard_cells, (double)d.false_alarm_rate, (double)d.z_min);
  printf("\nfuser");
  for (const cfear_fuser_options& f : C.fuser) printf(" %d %d", (int)f.soft_constraint, (int)f.use_guess);
  printf("\nend\n");
}
template <typename T>
std::vector<T> rest(std::istringstream& in) {
  std::vector<T> v;
  double x;
  while (in >> x) v.push_back((T)x);
  return v;
}
}  // namespace

int main() {
  cfear_seq_object O;
  cfear_params ctx;
  memset(&ctx, 0, sizeof(ctx));
  cfear_seq_config cfg;
  O.cfg = &cfg; O.par = &ctx;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, arg;
    if (!(in >> cmd)) continue;
    std::string msg;
    int rc = CFEAR_OK;
    cfear_seq_config cand;
    if (cmd == "object") {
      int overlap = 0;
      in >> O.B >> O.filter >> O.max_submap >> overlap >> O.sweeps;
      O.overlap = overlap != 0;
      continue;
    } else if (cmd == "ctx") {
      if (!set_fields(ctx, in)) { fprintf(stderr, "bad field: %s\n", line.c_str()); return 2; }
      continue;
    } else if (cmd == "dump") {
      dump(cfg);
      continue;
    } else if (cmd == "facts") {
      printf("needs_table %d zmin %d sources %d other_cost %d\n", cfg.needs_table() ? 1 : 0, cfg.filter_zmin(), cfg.sources(O.B), cfg.other_cost());
      continue;
    } else if (cmd == "effective") {
      for (int q = 0; q < O.B; q++) {
        const cfear_seq_config::effective_t e = cfg.effective(q, ctx);
        printf("seq %d source=%d soft_constraint=%d use_guess=%d", q, e.source, (int)e.fuser.soft_constraint, (int)e.fuser.use_guess);
        print_params(e.par);
        printf("\n");
      }
      continue;
    } else if (cmd == "check") {
      in >> arg;
      rc = cfear_seq_config_check(cfg, O, arg.c_str(), msg);
    } else if (cmd == "rows") {
      in >> arg;
      std::vector<cfear_params> rows;
      for (int i = 0; arg != "null" && i < atoi(arg.c_str()); i++) {
        rows.push_back(ctx);
        if (!std::getline(std::cin, line)) return 2;
        std::istringstream rin(line);
        if (!set_fields(rows.back(), rin)) { fprintf(stderr, "bad field: %s\n", line.c_str()); return 2; }
      }
      rc = cfear_seq_set_params(arg == "null" ? nullptr : rows.data(), (int)rows.size(), O, cand, msg);
    } else if (cmd == "sources") {
      in >> arg;
      const std::vector<int32_t> src = rest<int32_t>(in);
      rc = cfear_seq_set_sources(arg == "null" ? nullptr : src.data(), (int)src.size(), atoi(arg.c_str()), O, cand, msg);
    } else if (cmd == "shapes") {
      const std::vector<int32_t> v = rest<int32_t>(in);  // ("null" reads as no number: no rows)
      std::vector<cfear_seq_shape> shapes(v.size() / 2);
      for (size_t q = 0; q < shapes.size(); q++) { shapes[q].cost = v[2 * q]; shapes[q].submap_scan_size = v[2 * q + 1]; }
      rc = cfear_seq_set_shapes(line.find("null") != std::string::npos ? nullptr : shapes.data(), (int)shapes.size(), O, cand, msg);
    } else if (cmd == "dets") {
      in >> arg;
      const bool null = arg == "null", mapped = !null && arg != "-";
      int n = 0;
      in >> n;
      std::vector<cfear_seq_detector> dets;
      std::vector<int32_t> src;
      for (int i = 0; !null && i < n; i++) {
        if (!std::getline(std::cin, line)) return 2;
        std::istringstream din(line);
        cfear_seq_detector d;
        int s = 0;
        din >> d.window_size >> d.nb_guard_cells >> d.false_alarm_rate >> d.z_min >> s;
        dets.push_back(d); src.push_back(s);
      }
      const char* what = "odometry_set_sequence_detectors";
      const cfear_seq_detector* dp = null ? nullptr : dets.data();
      const int32_t* sp = mapped ? src.data() : nullptr;
      rc = cfear_seq_detectors_call_check(dp, n, sp, atoi(arg.c_str()), O, what, msg);
      if (rc == CFEAR_OK) rc = cfear_seq_set_detectors(dp, n, sp, atoi(arg.c_str()), O, what, cand, msg);
    } else if (cmd == "fuser") {
      const std::vector<int32_t> v = rest<int32_t>(in);
      std::vector<cfear_fuser_options> rows(v.size() / 2);
      for (size_t q = 0; q < rows.size(); q++) { rows[q].soft_constraint = v[2 * q]; rows[q].use_guess = v[2 * q + 1]; }
      rc = cfear_seq_set_fuser(line.find("null") != std::string::npos ? nullptr : rows.data(), (int)rows.size(), O, cand, msg);
    } else {
      fprintf(stderr, "unknown command: %s\n", line.c_str());
      return 2;
    }
    if (rc == CFEAR_OK && cmd != "check") cfg = cand;
    printf("rc %d %s\n", rc, msg.c_str());
  }
  return 0;
}
