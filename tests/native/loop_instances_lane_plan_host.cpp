// Host-only check of the policy-aware planner of the closed loop with per-robot records (quaternion-mpc_amd/csrc/qmpc_plan.h:
// plan_loop_instances(s, batch, has_ctrl, warm, policy, handoff_failed)), built like instance_lane_plan_host.cpp (hipcc -x hip
// --offload-host-only) over the same input space -- every model, mode, horizon 1..32, knob set and the batch sizes around every
// switch-over:
//   the overload equals the five-argument function without controller records, under WAVE, where that function refuses the
//         call or takes the persistent kernel, on a handle without a slot of the lane kernel's parameter table and below the
//         switch-over max(lane_min_inst, lane_min_loop_cold) (QMPC_VARIANT=4: no switch-over);
//   from the switch-over on it carries exactly the lane fields of the plain loop's cold tick (the plan of a handle whose own
//         loop switch-over is not above the batch): cap lane_cap_loop, hand-off variant and grid, order_prev, no upload;
//   it is never the persistent form with variant 4, and NONE exactly where the five-argument function is;
//   QMPC_LANE_INST_MIN and QMPC_LANE_MIN move the switch-over as they move its two terms (16384 with the defaults of QuatMpc's problem: 16384 and 14336 / 14848).
// Prints one summary line; exit status 0 when nothing failed.
#define QMPC_FUSED_TU 1      // the templates of the kernel headers only: no kernel is instantiated here
#include "../../quaternion-mpc_amd/csrc/qmpc_kernels.hip"
#include "../../quaternion-mpc_amd/csrc/qmpc_wform.h"
#include "../../quaternion-mpc_amd/csrc/qmpc_plan_fill.h"
#include "../../quaternion-mpc_amd/csrc/qmpc_kernel_slots.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <set>

namespace {

struct Knobs {
  const char* name;
  const char* var;
  const char* value;
  bool no_slot;
};
const Knobs kKnobs[] = {
    {"default", nullptr, nullptr, false},         {"QMPC_VARIANT=1", "QMPC_VARIANT", "1", false},
    {"QMPC_VARIANT=2", "QMPC_VARIANT", "2", false}, {"QMPC_VARIANT=3", "QMPC_VARIANT", "3", false},
    {"QMPC_VARIANT=4", "QMPC_VARIANT", "4", false}, {"QMPC_WFORM=0", "QMPC_WFORM", "0", false},
    {"QMPC_WFORM=3", "QMPC_WFORM", "3", false},     {"no-lane-slot", nullptr, nullptr, true},
    {"QMPC_LANE_MIN=8192", "QMPC_LANE_MIN", "8192", false},
    {"QMPC_LANE_MIN=30000", "QMPC_LANE_MIN", "30000", false},
    {"QMPC_LANE_MIN=1", "QMPC_LANE_MIN", "1", false},
    {"QMPC_LANE_INST_MIN=1", "QMPC_LANE_INST_MIN", "1", false},
    {"QMPC_LANE_INST_MIN=40000", "QMPC_LANE_INST_MIN", "40000", false},
    {"QMPC_LANE_CAP_LOOP=0", "QMPC_LANE_CAP_LOOP", "0", false}, {"QMPC_LANE_CAP_LOOP=9", "QMPC_LANE_CAP_LOOP", "9", false},
    {"QMPC_LOOP_FUSED=1", "QMPC_LOOP_FUSED", "1", false},     {"QMPC_LOOP_FUSED=0", "QMPC_LOOP_FUSED", "0", false},
};

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

bool same(const qmpc::qmpc_plan& a, const qmpc::qmpc_plan& b) {
  return a.family == b.family && a.variant == b.variant && a.lds == b.lds && a.gws == b.gws && a.handoff_variant == b.handoff_variant &&
         a.iter_cap == b.iter_cap && a.handoff_grid == b.handoff_grid && a.upload_params == b.upload_params &&
         a.order_prev == b.order_prev && a.fused == b.fused;
}

}  // namespace

int main() {
  long cases = 0, old = 0, lane = 0, handoff = 0, none = 0, persistent = 0;
  for (int model = 0; model < 3; ++model)
    for (int mode = 0; mode < 2; ++mode)
      for (int N = 1; N <= QMPC_MAX_HORIZON; ++N)
        for (const Knobs& k : kKnobs) {
          qmpc_params params;
          std::memset(&params, 0, sizeof params);
          params.model = model;
          params.mode = mode;
          params.horizon = N;
          params.iterations_max = mode == QMPC_MODE_REFERENCE ? (model == QMPC_MODEL_CONVEX ? 5 : 10) : 120;
          auto env = [&k](const char* name) -> const char* { return (k.var && std::strcmp(name, k.var) == 0) ? k.value : nullptr; };
          qmpc::qmpc_select sel;
          if (!qmpc::qmpc_fill_select(&sel, &params, env, !k.no_slot)) continue;
          const int sw = std::max(sel.lane_min_inst, sel.lane_min_loop_cold);
          // the switch-over is derived from the two it combines: 16384 with the defaults of QuatMpc's problem, moved by the knobs
          if (model == QMPC_MODEL_QUAT && !k.var) CHECK(sw == 16384, "N=%d %s: switch-over %d", N, k.name, sw);
          if (k.var && std::strcmp(k.name, "QMPC_LANE_INST_MIN=40000") == 0) CHECK(sw == 40000, "N=%d: switch-over %d", N, sw);
          if (k.var && std::strcmp(k.name, "QMPC_LANE_MIN=30000") == 0) CHECK(sw == 30000, "N=%d: switch-over %d", N, sw);
          if (k.var && std::strcmp(k.name, "QMPC_LANE_MIN=1") == 0) CHECK(sw == sel.lane_min_inst, "N=%d: switch-over %d", N, sw);
          if (k.var && std::strcmp(k.name, "QMPC_LANE_INST_MIN=1") == 0) CHECK(sw == sel.lane_min_loop_cold, "N=%d: switch-over %d", N, sw);
          std::set<int> batches = {1, 2, 65, 255, 256, 257, 512, 513, 1023, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 14335, 14336,
                                   16384, 18431, 18432, 18433, 20480, 29999, 30000, 32768, 39999, 40000, 40960, 65536, 262144};
          for (const auto& table : sel.lds)
            for (size_t lds : table)
              if (lds > 0)
                for (int d = -1; d <= 1; ++d) batches.insert(256 * (int)((160 * 1024) / lds) + d);
          for (int t : {sel.lane_min_batch, sel.lane_min_inst, sel.lane_min_loop_cold, sel.lane_min_warm, sel.lane_ref_min})
            for (int d = -1; d <= 1; ++d) batches.insert(t + d);
          for (int b : batches) {
            if (b < 1) continue;
            for (int has_ctrl = 0; has_ctrl < 2; ++has_ctrl)
              for (int warm = 0; warm < 2; ++warm)
                for (int hf = 0; hf < 2; ++hf) {
                  ++cases;
                  const qmpc::qmpc_plan w = qmpc::plan_loop_instances(sel, b, has_ctrl, warm, hf);
                  CHECK(same(qmpc::plan_loop_instances(sel, b, has_ctrl, warm, QMPC_INSTANCES_WAVE, hf), w),
                        "model %d mode %d N=%d %s B=%d ctrl %d warm %d: WAVE differs", model, mode, N, k.name, b, has_ctrl, warm);
                  const qmpc::qmpc_plan a = qmpc::plan_loop_instances(sel, b, has_ctrl, warm, QMPC_INSTANCES_AUTO, hf);
                  CHECK((a.family == QMPC_KERNEL_NONE) == (w.family == QMPC_KERNEL_NONE), "model %d mode %d N=%d %s B=%d ctrl %d warm %d: NONE",
                        model, mode, N, k.name, b, has_ctrl, warm);
                  CHECK(!(a.fused && a.variant == 4), "N=%d %s B=%d: persistent with variant 4", N, k.name, b);
                  const bool forced = sel.variant == 4;
                  if (!has_ctrl || w.family == QMPC_KERNEL_NONE || w.fused || !sel.lane_slot || (!forced && b < sw) ||
                      (sel.variant != 0 && !forced)) {
                    CHECK(same(a, w), "model %d mode %d N=%d %s B=%d ctrl %d warm %d hf %d: AUTO family %d, want %d", model, mode, N, k.name,
                          b, has_ctrl, warm, hf, a.family, w.family);
                    if (w.family == QMPC_KERNEL_NONE) ++none; else if (w.fused) ++persistent; else ++old;
                    if (has_ctrl && w.family != QMPC_KERNEL_NONE)
                      CHECK(qmpc::wform_index(a.variant) >= 0, "N=%d %s B=%d: variant %d", N, k.name, b, a.variant);
                    continue;
                  }
                  // the plain loop's cold tick for this batch on a handle whose loop switch-over is not above it
                  qmpc::qmpc_select pl = sel;
                  if (pl.lane_min_loop_cold > b) pl.lane_min_loop_cold = b;
                  const qmpc::qmpc_plan pp = qmpc::plan(pl, b, qmpc::QMPC_CALL_LOOP_TICK, true, hf);
                  CHECK(pp.variant == 4, "N=%d %s B=%d: the plain tick is not a lane plan", N, k.name, b);
                  CHECK(same(a, pp), "N=%d %s B=%d hf %d: AUTO family %d cap %d, plain tick family %d cap %d", N, k.name, b, hf, a.family,
                        a.iter_cap, pp.family, pp.iter_cap);
                  CHECK(a.variant == 4 && !a.upload_params && a.order_prev && !a.fused && !warm, "N=%d %s B=%d", N, k.name, b);
                  if (a.family == QMPC_KERNEL_LANE_HANDOFF) {
                    ++handoff;
                    CHECK(!hf && !forced, "N=%d %s B=%d hf %d: hand-off", N, k.name, b, hf);
                    CHECK(qmpc::wform_list_inst_slot(a.handoff_variant) >= 0 && a.iter_cap == sel.lane_cap_loop && a.iter_cap > 0 &&
                              a.iter_cap < sel.iterations_max && (a.handoff_grid == 512 || a.handoff_grid == 1024) &&
                              a.lds == sel.lds[0][a.handoff_variant] && a.gws == (a.handoff_variant == 5),
                          "N=%d %s B=%d: hand-off variant %d cap %d grid %d", N, k.name, b, a.handoff_variant, a.iter_cap, a.handoff_grid);
                  } else {
                    ++lane;
                    CHECK(a.family == QMPC_KERNEL_LANE && a.iter_cap == 0 && a.handoff_variant == 0, "N=%d %s B=%d: family %d", N, k.name, b,
                          a.family);
                  }
                  if (forced) CHECK(a.family == QMPC_KERNEL_LANE, "N=%d %s B=%d: QMPC_VARIANT=4 gives family %d", N, k.name, b, a.family);
                }
          }
        }
  std::printf("loop instance lane planner: %ld cases, %ld as before, %ld persistent, %ld lane, %ld lane with hand-off, %ld none\n", cases, old,
              persistent, lane, handoff, none);
  CHECK(old > 0 && persistent > 0 && lane > 0 && handoff > 0 && none > 0, "every branch visited");
  std::printf("%s: %d failures\n", failures ? "FAILED" : "passed", failures);
  return failures ? 1 : 0;
}
