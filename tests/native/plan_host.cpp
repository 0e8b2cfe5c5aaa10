// Host-only enumeration of the kernel planner (quaternion-mpc_amd/csrc/qmpc_plan.h): every model and mode, the horizons
// qmpc_create accepts, the knob sets the tests use and one setting of every other selection knob, the batch sizes around
// every switch-over, every kind of call.  One row per (configuration, call kind) and run of enumerated batch sizes with the
// same plan; tests/test_plan_cpu.py compares the output with tests/golden/kernel_plans.txt.gz.
//
// Built with hipcc -x hip --offload-host-only (no device code, no device needed): the layout sizes come from the same
// headers as the library's, and the selection state from the same filler as qmpc_create's.
//   plan_host              the table on stdout
//   plan_host --write F    ... into F
//   plan_host --kernels    check that every plan of the enumeration names a kernel of its unit's launch table
//                          (qmpc_kernel_slots.h)
// The planners of the calls with per-instance records (plan_instances, plan_convex_instances, plan_loop_instances) have a
// program of their own with the same three modes, records_plan_host.cpp.
#define QMPC_FUSED_TU 1      // the templates of the kernel headers only: no kernel is instantiated here
#include "../../quaternion-mpc_amd/csrc/qmpc_kernels.hip"
#include "../../quaternion-mpc_amd/csrc/qmpc_wform.h"
#include "../../quaternion-mpc_amd/csrc/qmpc_kernel_slots.h"
#include "../../quaternion-mpc_amd/csrc/qmpc_plan_fill.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

namespace {

struct Knobs {
  const char* name;
  const char* var;        // the environment variable it sets (or null)
  const char* value;
  bool no_slot;           // no lane parameter slot was left for the handle
  int handoff_failed;     // the hand-off records could not be allocated
};
const Knobs kKnobs[] = {
    {"default", nullptr, nullptr, false, 0},       {"QMPC_VARIANT=1", "QMPC_VARIANT", "1", false, 0},
    {"QMPC_VARIANT=2", "QMPC_VARIANT", "2", false, 0}, {"QMPC_VARIANT=3", "QMPC_VARIANT", "3", false, 0},
    {"QMPC_VARIANT=4", "QMPC_VARIANT", "4", false, 0}, {"QMPC_WFORM=0", "QMPC_WFORM", "0", false, 0},
    {"QMPC_WFORM=3", "QMPC_WFORM", "3", false, 0},     {"no-lane-slot", nullptr, nullptr, true, 0},
    {"handoff-failed", nullptr, nullptr, false, 1},
    // the other knobs the choice reads (tools, experiments)
    {"QMPC_VARIANT=4 handoff-failed", "QMPC_VARIANT", "4", false, 1},
    {"QMPC_LANE_MIN=8192", "QMPC_LANE_MIN", "8192", false, 0},
    {"QMPC_LANE_REF_MIN=8192", "QMPC_LANE_REF_MIN", "8192", false, 0},      // (below the closed loop's own switch-over)
    {"QMPC_LANE_CAP=0", "QMPC_LANE_CAP", "0", false, 0},     {"QMPC_LANE_CAP=12", "QMPC_LANE_CAP", "12", false, 0},
    {"QMPC_LANE_CAP_LOOP=0", "QMPC_LANE_CAP_LOOP", "0", false, 0}, {"QMPC_LANE_CAP_WARM=0", "QMPC_LANE_CAP_WARM", "0", false, 0},
    {"QMPC_LOOP_FUSED=0", "QMPC_LOOP_FUSED", "0", false, 0}, {"QMPC_LOOP_FUSED=1", "QMPC_LOOP_FUSED", "1", false, 0},
    {"QMPC_REF_WFORM_MAXN=12", "QMPC_REF_WFORM_MAXN", "12", false, 0},
};
const char* kModel[] = {"quat", "convex", "quat8"};
const char* kMode[] = {"converged", "reference"};
const char* kKind[] = {"plain", "warm", "loop-tick", "warm-loop-first", "warm-loop-tick", "loop", "warm-loop", "profile"};

std::string row(const qmpc::qmpc_plan& p) {
  char b[128];
  std::snprintf(b, sizeof b, "%d %d %zu %d %d %d %d %d %d %d", p.family, p.variant, p.lds, (int)p.gws, p.handoff_variant, p.iter_cap,
                p.handoff_grid, (int)p.upload_params, (int)p.order_prev, (int)p.fused);
  return b;
}

// Whether the launch table slot the launchers take for plan p of a call of kind `call` exists (qmpc_hip.hip: launch_solve,
// loop_tick_solve, qmpc_solve_warm_device, qmpc_debug_profile, loop_run_impl, launch_lane); joint: the JOINT half of the
// persistent kernels.  A plan of no wave kernel (NONE, the lane kernel) needs none.
bool has_kernel(const qmpc::qmpc_select& s, const qmpc::qmpc_plan& p, qmpc::qmpc_call call, int batch, bool joint) {
  using namespace qmpc;
  const bool ref = s.mode == QMPC_MODE_REFERENCE, convex = s.model == QMPC_MODEL_CONVEX;
  const bool warm = call == QMPC_CALL_WARM || call == QMPC_CALL_WARM_LOOP_FIRST || call == QMPC_CALL_WARM_LOOP_TICK || call == QMPC_CALL_WARM_LOOP;
  if (p.family == QMPC_KERNEL_NONE || p.family == QMPC_KERNEL_LANE) return true;
  if (p.family == QMPC_KERNEL_LANE_HANDOFF) return wform_list_slot(p.handoff_variant) >= 0;
  if (p.fused) return fused_slot(p.variant, ref, convex, joint) >= 0;
  if (warm) return warm_slot(p.variant, convex) >= 0;
  if (call == QMPC_CALL_PROFILE) return p.variant >= 3 ? wform_quat_slot(p.variant, true) >= 0 : dense_solve_slot(s.model, p.variant, true) >= 0;
  if (p.variant >= 3)
    return (s.model == QMPC_MODEL_QUAT && !ref) ? wform_quat_slot(p.variant, false) >= 0
                                                : wform_slot(s.model, ref, p.variant, wform_ref_one_wave(batch, p.lds)) >= 0;
  return ref ? dense_ref_slot(s.model, p.variant) >= 0 : dense_solve_slot(s.model, p.variant, false) >= 0;
}

}  // namespace

int main(int argc, char** argv) {
  FILE* out = stdout;
  const bool kernels = argc == 2 && std::strcmp(argv[1], "--kernels") == 0;
  if (argc == 3 && std::strcmp(argv[1], "--write") == 0) out = std::fopen(argv[2], "w");
  else if (argc != 1 && !kernels) { std::fprintf(stderr, "usage: plan_host [--write FILE | --kernels]\n"); return 2; }
  if (!out) return 1;
  long checked = 0, missing = 0;
  auto check = [&](const qmpc::qmpc_select& sel, const qmpc::qmpc_plan& p, qmpc::qmpc_call call, int b, const char* cfg) {
    for (int joint = 0; joint < (p.fused ? 2 : 1); ++joint) {
      ++checked;
      if (!has_kernel(sel, p, call, b, joint) && ++missing <= 20)
        std::fprintf(stderr, "no kernel: %s, call %d batch %d: family %d variant %d joint %d\n", cfg, (int)call, b, p.family, p.variant, joint);
    }
  };
  if (!kernels)
    std::fprintf(out, "# per configuration and call kind, from the smallest batch of each run with one plan: kind batch | family variant lds gws "
                    "handoff_variant iter_cap handoff_grid upload_params order_prev fused\n");
  const int horizons[] = {1, 2, 4, 10, 12, 13, 16, 20, 21, 22, 23, 32};
  for (int model = 0; model < 3; ++model)
    for (int mode = 0; mode < 2; ++mode)
      for (int N : horizons)
        for (const Knobs& k : kKnobs) {
          qmpc_params params;
          std::memset(&params, 0, sizeof params);
          params.model = model;
          params.mode = mode;
          params.horizon = N;
          // qmpc_default_*_params: 10 AL iterations in the reference mode (ConvexMpc: 5), 120 interior-point iterations otherwise
          params.iterations_max = mode == QMPC_MODE_REFERENCE ? (model == QMPC_MODEL_CONVEX ? 5 : 10) : 120;
          auto env = [&k](const char* name) -> const char* { return (k.var && std::strcmp(name, k.var) == 0) ? k.value : nullptr; };
          qmpc::qmpc_select sel;
          if (!qmpc::qmpc_fill_select(&sel, &params, env, !k.no_slot)) continue;      // qmpc_create refuses the horizon
          std::set<int> batches = {1, 256, 512, 513, 768, 769, 1024, 1025, 2048, 2049, 4096, 4097, 262144};
          for (const auto& table : sel.lds)
            for (size_t lds : table)
              if (lds > 0)
                for (int d = -1; d <= 1; ++d) batches.insert(256 * (int)((160 * 1024) / lds) + d);
          for (int t : {sel.lane_min_batch, sel.lane_min_loop_cold, sel.lane_min_warm, sel.lane_ref_min, qmpc::kLaneRefMinLoop})
            for (int d = -1; d <= 1; ++d) batches.insert(t + d);
          char cfg[128];
          std::snprintf(cfg, sizeof cfg, "%s %s N=%d %s", kModel[model], kMode[mode], N, k.name);
          if (!kernels) std::fprintf(out, "# %s\n", cfg);
          for (int kind = 0; kind <= (int)qmpc::QMPC_CALL_COUNT; ++kind) {      // the last: a plain solve without status records
            const bool has_info = kind != (int)qmpc::QMPC_CALL_COUNT;
            const qmpc::qmpc_call call = has_info ? (qmpc::qmpc_call)kind : qmpc::QMPC_CALL_PLAIN;
            std::string prev;
            for (int b : batches) {
              if (b < 1) continue;
              const qmpc::qmpc_plan p = qmpc::plan(sel, b, call, has_info, k.handoff_failed);
              if (kernels) {
                check(sel, p, call, b, cfg);
                continue;
              }
              const std::string r = row(p);
              if (r == prev) continue;
              std::fprintf(out, "%s%s %d %s\n", kKind[call], has_info ? "" : "-noinfo", b, r.c_str());
              prev = r;
            }
          }
        }
  if (kernels) {
    std::printf("%ld plans checked, %ld without a kernel\n", checked, missing);
    return missing ? 1 : 0;
  }
  return out == stdout ? 0 : (std::fclose(out) == 0 ? 0 : 1);
}
