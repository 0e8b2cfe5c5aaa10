// Host-only enumeration and checks of the planners of the calls with per-instance records (quaternion-mpc_amd/csrc/qmpc_plan.h:
// plan_instances, plan_convex_instances, plan_loop_instances), built like plan_host.cpp (hipcc -x hip --offload-host-only; no
// device code, no device needed).  One knob table, one batch enumeration and ONE way into the planner, record_plan(sel,
// settings, facts): every model and mode, the knob sets below, the batch sizes around every switch-over, every setting of a
// handle (qmpc_instances_policy, hand-off records failed, qmpc_set_loop_warm_records, qmpc_set_convex_records) and every fact
// of a call (status records, controller records, warm start, first tick).
//   records_plan_host              the table on stdout: per configuration one section per (call, settings, facts), one row per
//                                  run of enumerated batch sizes with the same plan; a section that is NONE at every batch is one
//                                  line, a section equal to the one before it is `=`.  tests/test_plan_cpu.py compares it with
//                                  tests/golden/record_plans.txt.gz (the horizons of plan_host.cpp).
//   records_plan_host --write F    ... into F
//   records_plan_host --kernels    every plan of that enumeration names a kernel of the launch table it is launched from
//                                  (qmpc_kernel_slots.h)
//   records_plan_host --check S    the rule restated, over the horizons 1..32; S one of
//       instances         qmpc_solve_instances* under the default settings against the plain solve's plan
//       instances-policy  ... under QMPC_INSTANCES_AUTO: the switch-over and the lane fields of the plain solve
//       loop              qmpc_loop_run_instances* under the default settings: refusals, persistent / per-tick threshold
//       loop-policy       ... under QMPC_INSTANCES_AUTO: the larger of two switch-overs, the lane fields of the plain cold tick
//       loop-warm         ... on a handle that opted in to warm-started ticks with controller records, and their first tick
//       convex            qmpc_convex_solve_instances* and the loops on a ConvexMpc handle that opted in
//     each prints its summary line and `passed: 0 failures`; exit status 0 when nothing failed.
#define QMPC_FUSED_TU 1      // the templates of the kernel headers only: no kernel is instantiated here
#include "../../quaternion-mpc_amd/csrc/qmpc_kernels.hip"
#include "../../quaternion-mpc_amd/csrc/qmpc_wform.h"
#include "../../quaternion-mpc_amd/csrc/qmpc_kernel_slots.h"
#include "../../quaternion-mpc_amd/csrc/qmpc_plan_fill.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

namespace {

using qmpc::qmpc_plan;
using qmpc::qmpc_select;

// ---- the one way into the planner -------------------------------------------------------------------------------------------
typedef qmpc::qmpc_opts Settings;      // a handle's run-time settings
enum Call { INSTANCES, CONVEX_INSTANCES, LOOP };
struct Facts {
  Call call;
  int batch;
  bool has_info = true;                                  // INSTANCES: the call passes status records
  bool has_ctrl = false, warm = false, first = false;    // LOOP: controller records, lp->warm_start, the first tick of the call
};
qmpc_plan record_plan(const qmpc_select& s, const Settings& o, const Facts& f) {
  switch (f.call) {
    case INSTANCES: return qmpc::plan_instances(s, o, f.batch, f.has_info);
    case CONVEX_INSTANCES: return qmpc::plan_convex_instances(s, f.batch);
    default: return qmpc::plan_loop_instances(s, o, f.batch, f.has_ctrl, f.warm, f.first);
  }
}
Settings settings(int policy, bool hf = false, bool wr = false, bool crec = false) {
  Settings o;
  o.inst_policy = policy;
  o.handoff_failed = hf;
  o.loop_warm_records = wr;
  o.convex_records = crec;
  return o;
}
qmpc_plan instances(const qmpc_select& s, const Settings& o, int b, bool has_info = true) {
  Facts f{INSTANCES, b};
  f.has_info = has_info;
  return record_plan(s, o, f);
}
qmpc_plan loop(const qmpc_select& s, const Settings& o, int b, bool has_ctrl, bool warm, bool first = false) {
  Facts f{LOOP, b};
  f.has_ctrl = has_ctrl;
  f.warm = warm;
  f.first = first;
  return record_plan(s, o, f);
}

// ---- the enumeration --------------------------------------------------------------------------------------------------------
struct Knobs {
  const char* name;
  const char* var;        // the environment variable it sets (or null)
  const char* value;
  bool no_slot;           // no lane parameter slot was left for the handle
};
const Knobs kKnobs[] = {
    {"default", nullptr, nullptr, false},
    {"QMPC_VARIANT=1", "QMPC_VARIANT", "1", false},
    {"QMPC_VARIANT=2", "QMPC_VARIANT", "2", false},
    {"QMPC_VARIANT=3", "QMPC_VARIANT", "3", false},
    {"QMPC_VARIANT=4", "QMPC_VARIANT", "4", false},
    {"QMPC_WFORM=0", "QMPC_WFORM", "0", false},
    {"QMPC_WFORM=3", "QMPC_WFORM", "3", false},
    {"no-lane-slot", nullptr, nullptr, true},
    {"QMPC_LANE_MIN=1", "QMPC_LANE_MIN", "1", false},
    {"QMPC_LANE_MIN=8192", "QMPC_LANE_MIN", "8192", false},
    {"QMPC_LANE_MIN=30000", "QMPC_LANE_MIN", "30000", false},
    {"QMPC_LANE_REF_MIN=8192", "QMPC_LANE_REF_MIN", "8192", false},
    {"QMPC_LANE_INST_MIN=1", "QMPC_LANE_INST_MIN", "1", false},
    {"QMPC_LANE_INST_MIN=40000", "QMPC_LANE_INST_MIN", "40000", false},
    {"QMPC_LANE_CAP=0", "QMPC_LANE_CAP", "0", false},
    {"QMPC_LANE_CAP=12", "QMPC_LANE_CAP", "12", false},
    {"QMPC_LANE_CAP_LOOP=0", "QMPC_LANE_CAP_LOOP", "0", false},
    {"QMPC_LANE_CAP_LOOP=9", "QMPC_LANE_CAP_LOOP", "9", false},
    {"QMPC_LANE_CAP_WARM=0", "QMPC_LANE_CAP_WARM", "0", false},
    {"QMPC_LANE_CAP_WARM=5", "QMPC_LANE_CAP_WARM", "5", false},
    {"QMPC_LOOP_FUSED=0", "QMPC_LOOP_FUSED", "0", false},
    {"QMPC_LOOP_FUSED=1", "QMPC_LOOP_FUSED", "1", false},
    {"QMPC_REF_WFORM_MAXN=12", "QMPC_REF_WFORM_MAXN", "12", false},
};
const char* kModel[] = {"quat", "convex", "quat8"};
const char* kMode[] = {"converged", "reference"};

struct Config {
  int model, mode, N;
  const Knobs* k;
  qmpc_select sel;
  std::set<int> batches;
  char name[128];
  bool knob(const char* name_) const { return std::strcmp(k->name, name_) == 0; }
};

// every configuration qmpc_create accepts, with the batch sizes around every LDS and switch-over boundary
template <class F>
void for_each_config(const std::vector<int>& horizons, F&& f) {
  for (int model = 0; model < 3; ++model)
    for (int mode = 0; mode < 2; ++mode)
      for (int N : horizons)
        for (const Knobs& k : kKnobs) {
          Config c;
          c.model = model, c.mode = mode, c.N = N, c.k = &k;
          qmpc_params params;
          std::memset(&params, 0, sizeof params);
          params.model = model;
          params.mode = mode;
          params.horizon = N;
          // qmpc_default_*_params: 10 AL iterations in the reference mode (ConvexMpc: 5), 120 interior-point iterations otherwise
          params.iterations_max = mode == QMPC_MODE_REFERENCE ? (model == QMPC_MODEL_CONVEX ? 5 : 10) : 120;
          auto env = [&k](const char* name) -> const char* { return (k.var && std::strcmp(name, k.var) == 0) ? k.value : nullptr; };
          if (!qmpc::qmpc_fill_select(&c.sel, &params, env, !k.no_slot)) continue;      // qmpc_create refuses the horizon
          c.batches = {1,     2,     65,    96,    255,   256,   257,   512,   513,   768,   769,   1023,  1024,
                       1025,  2047,  2048,  2049,  3000,  4095,  4096,  4097,  8192,  14335, 14336, 16384, 18431,
                       18432, 18433, 20479, 20480, 20481, 29999, 30000, 32768, 39999, 40000, 40960, 65536, 262144};
          for (const auto& table : c.sel.lds)
            for (size_t lds : table)
              if (lds > 0)
                for (int d = -1; d <= 1; ++d) c.batches.insert(256 * (int)((160 * 1024) / lds) + d);
          for (int t : {c.sel.lane_min_batch, c.sel.lane_min_inst, c.sel.lane_min_loop_cold, c.sel.lane_min_warm, c.sel.lane_ref_min,
                        qmpc::kLaneRefMinLoop})
            for (int d = -1; d <= 1; ++d) c.batches.insert(t + d);
          c.batches.erase(c.batches.begin(), c.batches.lower_bound(1));
          std::snprintf(c.name, sizeof c.name, "%s %s N=%d %s", kModel[model], kMode[mode], N, k.name);
          f(c);
        }
}
const std::vector<int> kTableHorizons = {1, 2, 4, 10, 12, 13, 16, 20, 21, 22, 23, 32};
std::vector<int> all_horizons() {
  std::vector<int> h;
  for (int N = 1; N <= QMPC_MAX_HORIZON; ++N) h.push_back(N);
  return h;
}

// every (settings, facts) of a call of each kind, as `visit(section name, settings, facts without the batch)`
template <class F>
void for_each_section(F&& visit) {
  char name[96];
  for (int policy : {QMPC_INSTANCES_WAVE, QMPC_INSTANCES_AUTO})
    for (int has_info = 0; has_info < 2; ++has_info)
      for (int hf = 0; hf < 2; ++hf) {
        std::snprintf(name, sizeof name, "instances policy=%d info=%d hf=%d", policy, has_info, hf);
        Facts f{INSTANCES, 0};
        f.has_info = has_info;
        visit(name, settings(policy, hf), f);
      }
  visit("convex-instances", Settings(), Facts{CONVEX_INSTANCES, 0});
  for (int ctrl = 0; ctrl < 2; ++ctrl)
    for (int warm = 0; warm < 2; ++warm)
      for (int policy : {QMPC_INSTANCES_WAVE, QMPC_INSTANCES_AUTO})
        for (int hf = 0; hf < 2; ++hf)
          for (int wr = 0; wr < 2; ++wr)
            for (int first = 0; first < 2; ++first)
              for (int crec = 0; crec < 2; ++crec) {
                std::snprintf(name, sizeof name, "loop ctrl=%d warm=%d policy=%d hf=%d wr=%d first=%d crec=%d", ctrl, warm, policy, hf, wr,
                              first, crec);
                Facts f{LOOP, 0};
                f.has_ctrl = ctrl, f.warm = warm, f.first = first;
                visit(name, settings(policy, hf, wr, crec), f);
              }
}

std::string row(const qmpc_plan& p) {
  char b[128];
  std::snprintf(b, sizeof b, "%d %d %zu %d %d %d %d %d %d %d", p.family, p.variant, p.lds, (int)p.gws, p.handoff_variant, p.iter_cap,
                p.handoff_grid, (int)p.upload_params, (int)p.order_prev, (int)p.fused);
  return b;
}

int write_table(FILE* out) {
  std::fprintf(out, "# per configuration and section (call, settings, facts), from the smallest batch of each run with one plan: batch | family "
                    "variant lds gws handoff_variant iter_cap handoff_grid upload_params order_prev fused; NONE: at every batch; =: the section "
                    "above\n");
  for_each_config(kTableHorizons, [&](const Config& c) {
    std::fprintf(out, "# %s\n", c.name);
    std::string above;
    for_each_section([&](const char* name, const Settings& o, Facts f) {
      std::string body, prev;
      bool none = true;
      for (int b : c.batches) {
        f.batch = b;
        const qmpc_plan p = record_plan(c.sel, o, f);
        none = none && p.family == QMPC_KERNEL_NONE;
        const std::string r = row(p);
        if (r == prev) continue;
        body += std::to_string(b) + " | " + r + "\n";
        prev = r;
      }
      if (none) std::fprintf(out, "%s NONE\n", name);
      else if (body == above) std::fprintf(out, "%s =\n", name);
      else std::fprintf(out, "%s\n%s", name, body.c_str());
      above = body;
    });
  });
  return out == stdout ? 0 : (std::fclose(out) == 0 ? 0 : 1);
}

// ---- every plan names a kernel ----------------------------------------------------------------------------------------------
// the slot the launchers take for plan p (qmpc_hip.hip: inst_solve, loop_tick_solve, loop_records_device): the per-instance
// kernels and the persistent kernels with records are instantiated on the wrench-form variants; a call without controller
// records runs the plain loop's tick
bool has_kernel(const qmpc_select& s, const qmpc_plan& p, const Facts& f) {
  using namespace qmpc;
  const bool convex = s.model == QMPC_MODEL_CONVEX;
  if (p.family == QMPC_KERNEL_NONE || p.family == QMPC_KERNEL_LANE) return true;
  if (f.call == CONVEX_INSTANCES) return wform_convex_inst_slot(p.variant) >= 0;
  if (f.call == INSTANCES || f.has_ctrl) {
    if (p.family == QMPC_KERNEL_LANE_HANDOFF) return wform_list_inst_slot(p.handoff_variant) >= 0;
    if (p.fused || !f.warm || f.first) return (convex ? wform_convex_inst_slot(p.variant) : wform_index(p.variant)) >= 0;
    return wform_inst_warm_slot(p.variant) >= 0;
  }
  if (p.fused) return wform_index(p.variant) >= 0 && fused_slot(p.variant, false, convex, false) >= 0;
  if (p.family == QMPC_KERNEL_LANE_HANDOFF) return wform_list_slot(p.handoff_variant) >= 0;
  if (f.warm && !f.first) return warm_slot(p.variant, convex) >= 0;
  if (p.variant >= 3)
    return convex ? wform_slot(s.model, false, p.variant, wform_ref_one_wave(f.batch, p.lds)) >= 0 : wform_quat_slot(p.variant, false) >= 0;
  return dense_solve_slot(s.model, p.variant, false) >= 0;
}

int check_kernels() {
  long checked = 0, missing = 0;
  for_each_config(kTableHorizons, [&](const Config& c) {
    for_each_section([&](const char* name, const Settings& o, Facts f) {
      for (int b : c.batches) {
        f.batch = b;
        const qmpc_plan p = record_plan(c.sel, o, f);
        ++checked;
        if (!(p.lds <= 160 * 1024 && has_kernel(c.sel, p, f)) && ++missing <= 20)
          std::fprintf(stderr, "no kernel: %s, %s batch %d: family %d variant %d lds %zu\n", c.name, name, b, p.family, p.variant, p.lds);
      }
    });
  });
  std::printf("%ld record plans checked, %ld without a kernel\n", checked, missing);
  return missing ? 1 : 0;
}

// ---- the rule restated ------------------------------------------------------------------------------------------------------
int failures = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      if (failures < 20) {                        \
        std::printf("FAIL %s: ", #cond);          \
        std::printf(__VA_ARGS__);                 \
        std::printf("\n");                        \
      }                                           \
      ++failures;                                 \
    }                                             \
  } while (0)

bool same(const qmpc_plan& a, const qmpc_plan& b) {
  return a.family == b.family && a.variant == b.variant && a.lds == b.lds && a.gws == b.gws && a.handoff_variant == b.handoff_variant &&
         a.iter_cap == b.iter_cap && a.handoff_grid == b.handoff_grid && a.upload_params == b.upload_params &&
         a.order_prev == b.order_prev && a.fused == b.fused;
}
bool wform_family(int f) { return f == QMPC_KERNEL_WFORM_LDS || f == QMPC_KERNEL_WFORM_WS; }
bool lane_family(int f) { return f == QMPC_KERNEL_LANE || f == QMPC_KERNEL_LANE_HANDOFF; }
const int kPolicies[] = {QMPC_INSTANCES_WAVE, QMPC_INSTANCES_AUTO};

// a lane plan with per-lane parameters: the pure lane kernel, or the hand-off to the per-instance list kernel at `cap`
// (0: whatever cap the plan carries); counts it in *lane or *handoff
void check_lane_fields(const Config& c, int b, const qmpc_plan& a, int cap, bool may_hand_off, long* lane, long* handoff) {
  const qmpc_select& sel = c.sel;
  if (a.family == QMPC_KERNEL_LANE_HANDOFF) {
    ++*handoff;
    CHECK(may_hand_off, "%s B=%d: hand-off", c.name, b);
    CHECK(qmpc::wform_list_inst_slot(a.handoff_variant) >= 0 && (cap == 0 || a.iter_cap == cap) && a.iter_cap > 0 &&
              a.iter_cap < sel.iterations_max && (a.handoff_grid == 512 || a.handoff_grid == 1024) &&
              a.lds == sel.lds[0][a.handoff_variant] && a.lds <= 160 * 1024 && a.gws == (a.handoff_variant == 5),
          "%s B=%d: hand-off variant %d cap %d grid %d", c.name, b, a.handoff_variant, a.iter_cap, a.handoff_grid);
  } else {
    ++*lane;
    CHECK(a.family == QMPC_KERNEL_LANE && a.iter_cap == 0 && a.handoff_variant == 0, "%s B=%d: family %d", c.name, b, a.family);
  }
}

// qmpc_solve_instances* under the default settings: QuatMpc's problem in the converged mode takes a wave wrench-form kernel
// (never the lane kernel), the very variant, LDS and workspace of a plain solve wherever that solve is a wave kernel, and NONE
// where the plain solve would take no wrench-form kernel; every other handle gets NONE.
void check_instances() {
  long cases = 0, wave_equal = 0, above_lane = 0, none = 0;
  for_each_config(all_horizons(), [&](const Config& c) {
    const qmpc_select& sel = c.sel;
    const bool supported = c.model == QMPC_MODEL_QUAT && c.mode == QMPC_MODE_CONVERGED && sel.wform;
    for (int b : c.batches)
      for (int hf = 0; hf < 2; ++hf) {
        ++cases;
        const qmpc_plan r = instances(sel, Settings(), b);
        const qmpc_plan pp = qmpc::plan(sel, b, qmpc::QMPC_CALL_PLAIN, true, hf);
        CHECK(!lane_family(r.family) && r.family != QMPC_KERNEL_DENSE_LDS && r.family != QMPC_KERNEL_DENSE_WS, "%s B=%d: family %d", c.name, b,
              r.family);
        if (!supported) {
          CHECK(r.family == QMPC_KERNEL_NONE, "%s B=%d: family %d, want none", c.name, b, r.family);
          continue;
        }
        if (r.family == QMPC_KERNEL_NONE) {
          ++none;
        } else {
          CHECK(r.variant == 3 || r.variant == 5 || r.variant == 6, "%s B=%d: variant %d", c.name, b, r.variant);
          CHECK(r.family == (r.variant == 3 ? QMPC_KERNEL_WFORM_LDS : QMPC_KERNEL_WFORM_WS), "%s B=%d", c.name, b);
          CHECK(r.lds == sel.lds[0][r.variant] && r.lds <= 160 * 1024 && r.gws == (r.variant != 3), "%s B=%d: lds %zu gws %d", c.name, b, r.lds,
                (int)r.gws);
          CHECK(r.handoff_variant == 0 && r.iter_cap == 0 && !r.fused, "%s B=%d", c.name, b);
        }
        if (lane_family(pp.family)) {
          ++above_lane;
          // the default knobs leave the wrench form at every batch size: the workspace form beyond the lane switch-over
          if (!c.k->var) CHECK(wform_family(r.family), "%s B=%d: none above the lane switch-over", c.name, b);
        } else if (wform_family(pp.family)) {
          ++wave_equal;
          CHECK(r.family == pp.family && r.variant == pp.variant && r.lds == pp.lds && r.gws == pp.gws, "%s B=%d: variant %d, plain solve %d",
                c.name, b, r.variant, pp.variant);
        } else {
          CHECK(r.family == QMPC_KERNEL_NONE, "%s B=%d: family %d where the plain solve takes family %d", c.name, b, r.family, pp.family);
        }
      }
  });
  std::printf("instances planner: %ld cases, %ld equal to a plain wave-kernel solve, %ld beyond the lane switch-over, %ld none\n", cases,
              wave_equal, above_lane, none);
  CHECK(wave_equal > 0 && above_lane > 0 && none > 0, "every branch visited");
}

// ... under the handle's policy.  WAVE: neither the status records nor failed hand-off records change the plan.  AUTO: the
// WAVE plan where that is NONE, on a handle without a slot of the lane kernel's parameter table and below lane_min_inst; from
// the switch-over on exactly the lane fields of the plain solve's plan (the plain plan of a handle whose own switch-over is
// not above the batch).  QMPC_LANE_INST_MIN moves the switch-over, QMPC_VARIANT=4 selects the pure lane kernel at every batch.
void check_instances_policy() {
  long cases = 0, wave = 0, lane = 0, handoff = 0, none = 0;
  for_each_config(all_horizons(), [&](const Config& c) {
    const qmpc_select& sel = c.sel;
    // the knob and its defaults (one value up to N = 12, one beyond)
    if (c.k->var && std::strcmp(c.k->var, "QMPC_LANE_INST_MIN") == 0)
      CHECK(sel.lane_min_inst == std::atoi(c.k->value), "%s: lane_min_inst %d", c.name, sel.lane_min_inst);
    else
      CHECK(sel.lane_min_inst == (c.N <= 12 ? qmpc::kLaneMinInst : qmpc::kLaneMinInstLong), "%s: lane_min_inst %d", c.name, sel.lane_min_inst);
    const bool forced = sel.variant == 4;
    for (int b : c.batches) {
      const qmpc_plan w = instances(sel, Settings(), b);
      for (int has_info = 0; has_info < 2; ++has_info)
        for (int hf = 0; hf < 2; ++hf) {
          ++cases;
          CHECK(same(instances(sel, settings(QMPC_INSTANCES_WAVE, hf), b, has_info), w), "%s B=%d: WAVE differs", c.name, b);
          const qmpc_plan a = instances(sel, settings(QMPC_INSTANCES_AUTO, hf), b, has_info);
          CHECK((a.family == QMPC_KERNEL_NONE) == (w.family == QMPC_KERNEL_NONE), "%s B=%d: NONE under one policy only", c.name, b);
          if (w.family == QMPC_KERNEL_NONE || !sel.lane_slot || (!forced && b < sel.lane_min_inst) || (sel.variant != 0 && !forced)) {
            CHECK(same(a, w), "%s B=%d info %d hf %d: AUTO family %d, want the wave plan's %d", c.name, b, has_info, hf, a.family, w.family);
            if (w.family == QMPC_KERNEL_NONE) ++none; else ++wave;
            // the wave plan's kernel exists
            if (w.family != QMPC_KERNEL_NONE) CHECK(qmpc::wform_index(a.variant) >= 0, "%s B=%d: variant %d", c.name, b, a.variant);
            continue;
          }
          // the plain solve's plan for this batch on a handle whose plain switch-over is not above it
          qmpc_select pl = sel;
          if (pl.lane_min_batch > b) pl.lane_min_batch = b;
          const qmpc_plan pp = qmpc::plan(pl, b, qmpc::QMPC_CALL_PLAIN, has_info, hf);
          CHECK(pp.variant == 4, "%s B=%d: the plain plan is not a lane plan", c.name, b);
          CHECK(same(a, pp), "%s B=%d info %d hf %d: AUTO family %d cap %d, plain solve family %d cap %d", c.name, b, has_info, hf, a.family,
                a.iter_cap, pp.family, pp.iter_cap);
          CHECK(a.variant == 4 && a.upload_params && !a.order_prev && !a.fused, "%s B=%d", c.name, b);
          check_lane_fields(c, b, a, 0, has_info && !hf && !forced, &lane, &handoff);
          if (forced) CHECK(a.family == QMPC_KERNEL_LANE, "%s B=%d: QMPC_VARIANT=4 gives family %d", c.name, b, a.family);
        }
    }
  });
  std::printf("instance lane planner: %ld cases, %ld wave, %ld lane, %ld lane with hand-off, %ld none\n", cases, wave, lane, handoff, none);
  CHECK(wave > 0 && lane > 0 && handoff > 0 && none > 0, "every branch visited");
}

// qmpc_loop_run_instances* under the default settings: refusals, the persistent / per-tick threshold of the plain loop, the
// variant of the plain loop's persistent kernel where the persistent form is taken, and the tick's plan where it is not.
void check_loop() {
  long cases = 0, persistent = 0, per_tick = 0, none = 0;
  for_each_config(all_horizons(), [&](const Config& c) {
    const qmpc_select& sel = c.sel;
    const bool quat = c.model == QMPC_MODEL_QUAT && c.mode == QMPC_MODE_CONVERGED;
    for (int b : c.batches)
      for (int has_ctrl = 0; has_ctrl < 2; ++has_ctrl)
        for (int warm = 0; warm < 2; ++warm)
          for (int hf = 0; hf < 2; ++hf) {
            ++cases;
            const qmpc_plan r = loop(sel, settings(QMPC_INSTANCES_WAVE, hf), b, has_ctrl, warm);
            if (!quat || (has_ctrl && (warm || !sel.wform))) {
              CHECK(r.family == QMPC_KERNEL_NONE, "%s B=%d ctrl %d warm %d: family %d, want none", c.name, b, has_ctrl, warm, r.family);
              ++none;
              continue;
            }
            // the plain loop of the same batch
            const qmpc_plan pl = qmpc::plan(sel, b, warm ? qmpc::QMPC_CALL_WARM_LOOP : qmpc::QMPC_CALL_LOOP, true, hf);
            const bool threshold = c.k->var && std::strcmp(c.k->var, "QMPC_LOOP_FUSED") == 0 ? c.k->value[0] == '1' : b <= (warm ? 4096 : 2048);
            CHECK(pl.fused == threshold, "%s B=%d warm %d: plain loop fused %d", c.name, b, warm, (int)pl.fused);
            if (pl.fused && qmpc::wform_index(pl.variant) >= 0) {
              ++persistent;
              CHECK(r.fused && r.variant == pl.variant && r.lds == pl.lds && r.gws == pl.gws && r.family == pl.family,
                    "%s B=%d ctrl %d warm %d: persistent variant %d, plain loop %d", c.name, b, has_ctrl, warm, r.variant, pl.variant);
              continue;
            }
            CHECK(!r.fused, "%s B=%d: persistent form without a wrench-form variant", c.name, b);
            if (has_ctrl) {
              const qmpc_plan pi = instances(sel, Settings(), b);
              CHECK(r.family == pi.family && r.variant == pi.variant && r.lds == pi.lds, "%s B=%d: per-tick %d vs instances %d", c.name, b,
                    r.variant, pi.variant);
            } else {
              const qmpc_plan pt = qmpc::plan(sel, b, warm ? qmpc::QMPC_CALL_WARM_LOOP_TICK : qmpc::QMPC_CALL_LOOP_TICK, true, hf);
              CHECK(r.family == pt.family && r.variant == pt.variant && r.iter_cap == pt.iter_cap, "%s B=%d warm %d: per-tick %d vs the plain tick %d",
                    c.name, b, warm, r.variant, pt.variant);
            }
            if (r.family == QMPC_KERNEL_NONE) ++none;
            else ++per_tick;
          }
  });
  std::printf("loop records planner: %ld cases, %ld persistent, %ld per tick, %ld refused\n", cases, persistent, per_tick, none);
  CHECK(persistent > 0 && per_tick > 0 && none > 0, "every branch visited");
}

// ... under the handle's policy.  AUTO equals WAVE without controller records, where WAVE refuses the call or takes the
// persistent kernel, on a handle without a slot of the lane kernel's parameter table and below the switch-over
// max(lane_min_inst, lane_min_loop_cold) (QMPC_VARIANT=4: no switch-over); from the switch-over on exactly the lane fields of
// the plain loop's cold tick (the plan of a handle whose own loop switch-over is not above the batch): cap lane_cap_loop,
// hand-off variant and grid, order_prev, no upload.  Never the persistent form with variant 4, NONE exactly where WAVE is.
// QMPC_LANE_INST_MIN and QMPC_LANE_MIN move the switch-over as they move its two terms (16384 with the defaults of QuatMpc's
// problem: 16384 and 14336 / 14848).
void check_loop_policy() {
  long cases = 0, old = 0, lane = 0, handoff = 0, none = 0, persistent = 0;
  for_each_config(all_horizons(), [&](const Config& c) {
    const qmpc_select& sel = c.sel;
    const int sw = std::max(sel.lane_min_inst, sel.lane_min_loop_cold);
    // the switch-over is derived from the two it combines: 16384 with the defaults of QuatMpc's problem, moved by the knobs
    if (c.model == QMPC_MODEL_QUAT && !c.k->var) CHECK(sw == 16384, "%s: switch-over %d", c.name, sw);
    if (c.knob("QMPC_LANE_INST_MIN=40000")) CHECK(sw == 40000, "%s: switch-over %d", c.name, sw);
    if (c.knob("QMPC_LANE_MIN=30000")) CHECK(sw == 30000, "%s: switch-over %d", c.name, sw);
    if (c.knob("QMPC_LANE_MIN=1")) CHECK(sw == sel.lane_min_inst, "%s: switch-over %d", c.name, sw);
    if (c.knob("QMPC_LANE_INST_MIN=1")) CHECK(sw == sel.lane_min_loop_cold, "%s: switch-over %d", c.name, sw);
    const bool forced = sel.variant == 4;
    for (int b : c.batches)
      for (int has_ctrl = 0; has_ctrl < 2; ++has_ctrl)
        for (int warm = 0; warm < 2; ++warm)
          for (int hf = 0; hf < 2; ++hf) {
            ++cases;
            const qmpc_plan w = loop(sel, settings(QMPC_INSTANCES_WAVE, hf), b, has_ctrl, warm);
            const qmpc_plan a = loop(sel, settings(QMPC_INSTANCES_AUTO, hf), b, has_ctrl, warm);
            CHECK((a.family == QMPC_KERNEL_NONE) == (w.family == QMPC_KERNEL_NONE), "%s B=%d ctrl %d warm %d: NONE", c.name, b, has_ctrl, warm);
            CHECK(!(a.fused && a.variant == 4), "%s B=%d: persistent with variant 4", c.name, b);
            if (!has_ctrl || w.family == QMPC_KERNEL_NONE || w.fused || !sel.lane_slot || (!forced && b < sw) || (sel.variant != 0 && !forced)) {
              CHECK(same(a, w), "%s B=%d ctrl %d warm %d hf %d: AUTO family %d, want %d", c.name, b, has_ctrl, warm, hf, a.family, w.family);
              if (w.family == QMPC_KERNEL_NONE) ++none; else if (w.fused) ++persistent; else ++old;
              if (has_ctrl && w.family != QMPC_KERNEL_NONE) CHECK(qmpc::wform_index(a.variant) >= 0, "%s B=%d: variant %d", c.name, b, a.variant);
              continue;
            }
            // the plain loop's cold tick for this batch on a handle whose loop switch-over is not above it
            qmpc_select pl = sel;
            if (pl.lane_min_loop_cold > b) pl.lane_min_loop_cold = b;
            const qmpc_plan pp = qmpc::plan(pl, b, qmpc::QMPC_CALL_LOOP_TICK, true, hf);
            CHECK(pp.variant == 4, "%s B=%d: the plain tick is not a lane plan", c.name, b);
            CHECK(same(a, pp), "%s B=%d hf %d: AUTO family %d cap %d, plain tick family %d cap %d", c.name, b, hf, a.family, a.iter_cap, pp.family,
                  pp.iter_cap);
            CHECK(a.variant == 4 && !a.upload_params && a.order_prev && !a.fused && !warm, "%s B=%d", c.name, b);
            check_lane_fields(c, b, a, sel.lane_cap_loop, !hf && !forced, &lane, &handoff);
            if (forced) CHECK(a.family == QMPC_KERNEL_LANE, "%s B=%d: QMPC_VARIANT=4 gives family %d", c.name, b, a.family);
          }
  });
  std::printf("loop instance lane planner: %ld cases, %ld as before, %ld persistent, %ld lane, %ld lane with hand-off, %ld none\n", cases, old,
              persistent, lane, handoff, none);
  CHECK(old > 0 && persistent > 0 && lane > 0 && handoff > 0 && none > 0, "every branch visited");
}

// ... on a handle that opted in to warm-started loops with controller records (qmpc_set_loop_warm_records).  Without
// controller records or without the warm start the setting changes nothing, for the tick and for the first tick.  With both:
//   NONE exactly for another model or mode, for a handle without wrench-form kernels, or where qmpc_solve_instances* has none;
//   persistent: where plan(QMPC_CALL_WARM_LOOP) is fused on variant 3 / 5 / 6, that plan (the rule of plant records only);
//   per tick, wave: otherwise the plan of qmpc_solve_instances* under the default settings with fused = false;
//   per tick, lane: under AUTO with a lane slot from max(lane_min_inst, lane_min_warm) on (QMPC_VARIANT=4: everywhere), the
//                   lane fields of the plain warm tick on a handle whose own switch-over is not above the batch: cap
//                   lane_cap_warm, hand-off variant and grid, order_prev, no upload;
//   the first tick: the same wave plan, or the plain QMPC_CALL_WARM_LOOP_FIRST lane plan (no cap, no hand-off);
// never fused on variant 4, and every planned variant has a slot in the launch tables it is launched from.
void check_loop_warm() {
  long cases = 0, off = 0, persistent = 0, wave = 0, lane = 0, handoff = 0, none = 0;
  for_each_config(all_horizons(), [&](const Config& c) {
    const qmpc_select& sel = c.sel;
    const int sw = std::max(sel.lane_min_inst, sel.lane_min_warm);
    // the switch-over with the defaults of QuatMpc's problem: 18432, 20480 at N = 13 ... 22
    if (c.model == QMPC_MODEL_QUAT && c.mode == QMPC_MODE_CONVERGED && !c.k->var && !c.k->no_slot)
      CHECK(sw == ((c.N >= 13 && c.N <= 22) ? 20480 : 18432), "%s: switch-over %d", c.name, sw);
    const bool forced = sel.variant == 4;
    for (int b : c.batches)
      for (int has_ctrl = 0; has_ctrl < 2; ++has_ctrl)
        for (int warm = 0; warm < 2; ++warm)
          for (int policy : kPolicies)
            for (int hf = 0; hf < 2; ++hf)
              for (int first = 0; first < 2; ++first) {
                ++cases;
                // the setting off: the first tick is the tick
                const qmpc_plan before = loop(sel, settings(policy, hf), b, has_ctrl, warm);
                CHECK(same(loop(sel, settings(policy, hf), b, has_ctrl, warm, first), before), "%s B=%d ctrl %d warm %d policy %d hf %d first %d: "
                      "setting off differs", c.name, b, has_ctrl, warm, policy, hf, first);
                const qmpc_plan a = loop(sel, settings(policy, hf, true), b, has_ctrl, warm, first);
                CHECK(!(a.fused && a.variant == 4), "%s B=%d: persistent with variant 4", c.name, b);
                if (!has_ctrl || !warm) {
                  CHECK(same(a, before), "%s B=%d ctrl %d warm %d policy %d: setting on differs without ctrl and warm", c.name, b, has_ctrl, warm,
                        policy);
                  ++off;
                  continue;
                }
                CHECK(before.family == QMPC_KERNEL_NONE, "%s B=%d: ctrl with warm accepted without the setting", c.name, b);
                const qmpc_plan inst = instances(sel, Settings(), b);
                const qmpc_plan f = qmpc::plan(sel, b, qmpc::QMPC_CALL_WARM_LOOP, true, hf);
                const bool pers = f.fused && qmpc::wform_index(f.variant) >= 0;
                if (c.model != QMPC_MODEL_QUAT || c.mode != QMPC_MODE_CONVERGED || !sel.wform || (!pers && inst.family == QMPC_KERNEL_NONE)) {
                  CHECK(a.family == QMPC_KERNEL_NONE, "%s B=%d: family %d, want NONE", c.name, b, a.family);
                  ++none;
                  continue;
                }
                if (pers) {      // the rule of a call with plant records only
                  CHECK(same(a, f) && same(a, loop(sel, settings(policy, hf), b, false, true)), "%s B=%d: persistent plan differs from the "
                        "plant-only call's", c.name, b);
                  CHECK(b <= 4096 || sel.loop_fused == 1, "%s B=%d: persistent beyond 4096 robots", c.name, b);
                  ++persistent;
                  continue;
                }
                const bool lane_form = policy == QMPC_INSTANCES_AUTO && sel.lane_slot && (forced || (sel.variant == 0 && b >= sw));
                if (!lane_form) {
                  qmpc_plan w = inst;
                  w.fused = false;
                  CHECK(same(a, w), "%s B=%d policy %d: family %d variant %d, want the plan of qmpc_solve_instances*", c.name, b, policy, a.family,
                        a.variant);
                  CHECK(qmpc::wform_inst_warm_slot(a.variant) >= 0 && qmpc::wform_index(a.variant) >= 0 && !a.fused && a.iter_cap == 0 &&
                            a.lds <= 160 * 1024,
                        "%s B=%d: variant %d without a slot", c.name, b, a.variant);
                  ++wave;
                  continue;
                }
                // the plain loop's warm tick (first tick) for this batch on a handle whose switch-over is not above it
                qmpc_select pl = sel;
                if (pl.lane_min_warm > b) pl.lane_min_warm = b;
                const qmpc_plan pp = qmpc::plan(pl, b, first ? qmpc::QMPC_CALL_WARM_LOOP_FIRST : qmpc::QMPC_CALL_WARM_LOOP_TICK, true, hf);
                CHECK(pp.variant == 4, "%s B=%d: the plain warm tick is not a lane plan", c.name, b);
                CHECK(same(a, pp), "%s B=%d hf %d first %d: family %d cap %d, plain warm tick family %d cap %d", c.name, b, hf, first, a.family,
                      a.iter_cap, pp.family, pp.iter_cap);
                CHECK(a.variant == 4 && !a.upload_params && a.order_prev && !a.fused, "%s B=%d", c.name, b);
                check_lane_fields(c, b, a, sel.lane_cap_warm, !hf && !forced && !first, &lane, &handoff);
                if (forced || first) CHECK(a.family == QMPC_KERNEL_LANE, "%s B=%d first %d: family %d", c.name, b, first, a.family);
              }
  });
  std::printf("loop warm records planner: %ld cases, %ld without ctrl and warm, %ld persistent, %ld wave, %ld lane, %ld lane with hand-off, %ld none\n",
              cases, off, persistent, wave, lane, handoff, none);
  CHECK(off > 0 && persistent > 0 && wave > 0 && lane > 0 && handoff > 0 && none > 0, "every branch visited");
}

// ConvexMpc's calls with per-instance records.
//   qmpc_convex_solve_instances*: NONE exactly for another model or mode and without wrench-form kernels; never a dense or lane
//     family; the variant of the plain solve's plan on the wave kernels (lane_slot off) wherever that is 3 / 5 / 6; where the
//     plain plan falls to the round-1 family: 6 under plan()'s own condition for it (N >= 4, lds[6] <= 80 KB), else 5 if
//     lds[5] <= 80 KB, else 3 if it fits a CU, else NONE; LDS and workspace flag of the variant; a slot in the launch table.
//   the loops: qmpc_set_convex_records changes nothing on another model; on a ConvexMpc handle that did not opt in every call
//     is NONE; on one that did:
//     NONE for the reference mode, for ctrl with the warm start (whatever qmpc_set_loop_warm_records says) and for ctrl without
//     wrench-form kernels or where the solve's plan has none;
//     persistent: where the plain ConvexMpc loop's plan is fused on variant 3 / 5 / 6, that plan;
//     per tick: otherwise the solve's plan with ctrl, the plain loop's tick without; fused = false; the policy changes nothing;
//   under every setting a call is NONE under AUTO exactly where it is NONE under WAVE.
// Prints the smallest batch that selects each variant at N = 10 and N = 20 with the default knobs.
void check_convex() {
  long cases = 0, off = 0, persistent = 0, tick_ctrl = 0, tick_plant = 0, none = 0, solve_same = 0, solve_fallback = 0, solve_none = 0;
  for_each_config(all_horizons(), [&](const Config& c) {
    const qmpc_select& sel = c.sel;
    const bool convex_ok = c.model == QMPC_MODEL_CONVEX && c.mode == QMPC_MODE_CONVERGED;
    const size_t* lds = sel.lds[0];
    int first_of[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int b : c.batches) {
      // ---- the solve's plan ----
      const qmpc_plan ci = record_plan(sel, Settings(), Facts{CONVEX_INSTANCES, b});
      CHECK(ci.family == QMPC_KERNEL_NONE || wform_family(ci.family), "%s B=%d: family %d", c.name, b, ci.family);
      CHECK(!ci.fused && ci.iter_cap == 0 && ci.handoff_variant == 0 && !ci.upload_params && !ci.order_prev, "%s B=%d: lane fields", c.name, b);
      if (!convex_ok || !sel.wform) {
        CHECK(ci.family == QMPC_KERNEL_NONE, "%s B=%d: family %d, want NONE", c.name, b, ci.family);
        ++solve_none;
      } else {
        qmpc_select w = sel;
        w.lane_slot = false;
        const qmpc_plan pp = qmpc::plan(w, b, qmpc::QMPC_CALL_PLAIN, true, false);
        if (wform_family(pp.family)) {
          CHECK(same(ci, pp), "%s B=%d: variant %d, the plain solve's %d", c.name, b, ci.variant, pp.variant);
          ++solve_same;
        } else {
          const int want = (c.N >= 4 && lds[6] <= 80 * 1024) ? 6 : lds[5] <= 80 * 1024 ? 5 : lds[3] <= 160 * 1024 ? 3 : 0;
          CHECK(ci.variant == want && (want != 0) == (ci.family != QMPC_KERNEL_NONE), "%s B=%d: variant %d, want %d", c.name, b, ci.variant, want);
          ++solve_fallback;
        }
        if (ci.family != QMPC_KERNEL_NONE) {
          CHECK(qmpc::wform_convex_inst_slot(ci.variant) >= 0 && ci.lds == lds[ci.variant] && ci.lds <= 160 * 1024 &&
                    ci.gws == (ci.variant != 3) && ci.family == (ci.variant == 3 ? QMPC_KERNEL_WFORM_LDS : QMPC_KERNEL_WFORM_WS),
                "%s B=%d: variant %d lds %zu gws %d", c.name, b, ci.variant, ci.lds, (int)ci.gws);
          if (!c.k->var && !c.k->no_slot && !first_of[ci.variant]) first_of[ci.variant] = b;
        }
      }
      // ---- the loops' plan ----
      for (int has_ctrl = 0; has_ctrl < 2; ++has_ctrl)
        for (int warm = 0; warm < 2; ++warm)
          for (int policy : kPolicies)
            for (int hf = 0; hf < 2; ++hf)
              for (int wr = 0; wr < 2; ++wr)
                for (int first = 0; first < 2; ++first) {
                  ++cases;
                  const qmpc_plan before = loop(sel, settings(policy, hf, wr, false), b, has_ctrl, warm, first);
                  const qmpc_plan a = loop(sel, settings(policy, hf, wr, true), b, has_ctrl, warm, first);
                  if (policy == QMPC_INSTANCES_AUTO)
                    CHECK((before.family == QMPC_KERNEL_NONE) ==
                                  (loop(sel, settings(QMPC_INSTANCES_WAVE, hf, wr, false), b, has_ctrl, warm, first).family == QMPC_KERNEL_NONE) &&
                              (a.family == QMPC_KERNEL_NONE) ==
                                  (loop(sel, settings(QMPC_INSTANCES_WAVE, hf, wr, true), b, has_ctrl, warm, first).family == QMPC_KERNEL_NONE),
                          "%s B=%d ctrl %d warm %d wr %d first %d: NONE under one policy only", c.name, b, has_ctrl, warm, wr, first);
                  if (c.model != QMPC_MODEL_CONVEX) {
                    CHECK(same(a, before), "%s B=%d: setting on differs on another model", c.name, b);
                    ++off;
                    continue;
                  }
                  CHECK(before.family == QMPC_KERNEL_NONE, "%s B=%d: a ConvexMpc handle accepted without the setting", c.name, b);
                  CHECK(!(a.fused && a.variant == 4), "%s B=%d: persistent with variant 4", c.name, b);
                  if (c.mode != QMPC_MODE_CONVERGED || (has_ctrl && (warm || !sel.wform))) {
                    CHECK(a.family == QMPC_KERNEL_NONE, "%s B=%d ctrl %d warm %d: family %d, want NONE", c.name, b, has_ctrl, warm, a.family);
                    ++none;
                    continue;
                  }
                  const qmpc_plan f = qmpc::plan(sel, b, warm ? qmpc::QMPC_CALL_WARM_LOOP : qmpc::QMPC_CALL_LOOP, true, hf);
                  if (f.fused && qmpc::wform_index(f.variant) >= 0) {
                    CHECK(same(a, f), "%s B=%d: persistent plan differs from the plain loop's", c.name, b);
                    CHECK(b <= (warm ? 4096 : 2048) || sel.loop_fused == 1, "%s B=%d: persistent beyond the threshold", c.name, b);
                    ++persistent;
                    continue;
                  }
                  qmpc_plan want = has_ctrl ? ci : qmpc::plan(sel, b, warm ? qmpc::QMPC_CALL_WARM_LOOP_TICK : qmpc::QMPC_CALL_LOOP_TICK, true, hf);
                  want.fused = false;
                  CHECK(same(a, want), "%s B=%d ctrl %d warm %d policy %d: family %d variant %d, want %d / %d", c.name, b, has_ctrl, warm, policy,
                        a.family, a.variant, want.family, want.variant);
                  if (has_ctrl) {
                    CHECK(a.family == QMPC_KERNEL_NONE || (wform_family(a.family) && qmpc::wform_convex_inst_slot(a.variant) >= 0),
                          "%s B=%d: ctrl tick on family %d", c.name, b, a.family);
                    ++tick_ctrl;
                  } else {
                    ++tick_plant;
                  }
                }
    }
    if (convex_ok && !c.k->var && !c.k->no_slot && (c.N == 10 || c.N == 20))
      std::printf("convex instances N=%d: smallest enumerated batch on variant 3: %d, 5: %d, 6: %d (lds %zu / %zu / %zu B)\n", c.N, first_of[3],
                  first_of[5], first_of[6], lds[3], lds[5], lds[6]);
  });
  std::printf("convex records planner: %ld loop cases, %ld on another model, %ld persistent, %ld per tick with ctrl, %ld per tick without, %ld none; "
              "solve: %ld the plain variant, %ld beyond it, %ld none\n",
              cases, off, persistent, tick_ctrl, tick_plant, none, solve_same, solve_fallback, solve_none);
  CHECK(off > 0 && persistent > 0 && tick_ctrl > 0 && tick_plant > 0 && none > 0 && solve_same > 0 && solve_fallback > 0 && solve_none > 0,
        "every branch visited");
}

const struct { const char* name; void (*run)(); } kChecks[] = {
    {"instances", check_instances}, {"instances-policy", check_instances_policy}, {"loop", check_loop},
    {"loop-policy", check_loop_policy}, {"loop-warm", check_loop_warm},           {"convex", check_convex},
};

}  // namespace

int main(int argc, char** argv) {
  if (argc == 1) return write_table(stdout);
  if (argc == 3 && std::strcmp(argv[1], "--write") == 0) {
    FILE* out = std::fopen(argv[2], "w");
    return out ? write_table(out) : 1;
  }
  if (argc == 2 && std::strcmp(argv[1], "--kernels") == 0) return check_kernels();
  if (argc == 3 && std::strcmp(argv[1], "--check") == 0)
    for (const auto& c : kChecks)
      if (std::strcmp(argv[2], c.name) == 0) {
        c.run();
        std::printf("%s: %d failures\n", failures ? "FAILED" : "passed", failures);
        return failures ? 1 : 0;
      }
  std::fprintf(stderr, "usage: records_plan_host [--write FILE | --kernels | --check instances|instances-policy|loop|loop-policy|loop-warm|convex]\n");
  return 2;
}
