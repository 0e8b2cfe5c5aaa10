// Host-only check of the planner of warm-started closed loops with controller records (quaternion-mpc_amd/csrc/qmpc_plan.h:
// plan_loop_instances(s, batch, has_ctrl, warm, policy, handoff_failed, warm_records, first)), built like
// loop_instances_lane_plan_host.cpp (hipcc -x hip --offload-host-only) over the same input space -- every model, mode, horizon
// 1..32, knob set and the batch sizes around every switch-over, x ctrl x warm x policy x handoff_failed:
//   flag off: the overload equals the policy-aware overload field for field, for the tick and for the first tick;
//   flag on, without controller records or without the warm start: the same;
//   flag on, with both:
//     NONE exactly for another model or mode and for a handle without wrench-form kernels, or where qmpc_solve_instances* has none;
//     persistent: where plan(QMPC_CALL_WARM_LOOP) is fused on variant 3 / 5 / 6, that plan (the rule of plant records only);
//     per tick, wave: otherwise plan_instances(s, batch) with fused = false;
//     per tick, lane: under AUTO with a lane slot from max(lane_min_inst, lane_min_warm) on (QMPC_VARIANT=4: everywhere), the
//                     lane fields of the plain warm tick on a handle whose own switch-over is not above the batch: cap
//                     lane_cap_warm, hand-off variant and grid, order_prev, no upload;
//     the first tick: the same wave plan, or the plain QMPC_CALL_WARM_LOOP_FIRST lane plan (no cap, no hand-off);
//   the plan is never fused on variant 4, and every planned variant has a slot in the launch tables it is launched from
//   (wform_inst_warm_slot, wform_index for the first tick and the persistent kernel, wform_list_inst_slot for the hand-off).
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
    {"QMPC_LANE_CAP_WARM=0", "QMPC_LANE_CAP_WARM", "0", false}, {"QMPC_LANE_CAP_WARM=5", "QMPC_LANE_CAP_WARM", "5", false},
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
  long cases = 0, off = 0, persistent = 0, wave = 0, lane = 0, handoff = 0, none = 0;
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
          const int sw = std::max(sel.lane_min_inst, sel.lane_min_warm);
          // the switch-over with the defaults of QuatMpc's problem: 18432, 20480 at N = 13 ... 22
          if (model == QMPC_MODEL_QUAT && mode == QMPC_MODE_CONVERGED && !k.var && !k.no_slot)
            CHECK(sw == ((N >= 13 && N <= 22) ? 20480 : 18432), "N=%d %s: switch-over %d", N, k.name, sw);
          std::set<int> batches = {1, 2, 65, 255, 256, 257, 512, 513, 1023, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 14335, 14336,
                                   16384, 18431, 18432, 18433, 20479, 20480, 20481, 29999, 30000, 32768, 39999, 40000, 40960, 65536, 262144};
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
                for (int policy : {QMPC_INSTANCES_WAVE, QMPC_INSTANCES_AUTO})
                  for (int hf = 0; hf < 2; ++hf)
                    for (int first = 0; first < 2; ++first) {
                      ++cases;
                      const qmpc::qmpc_plan before = qmpc::plan_loop_instances(sel, b, has_ctrl, warm, policy, hf);
                      // flag off: the policy-aware overload, field for field
                      CHECK(same(qmpc::plan_loop_instances(sel, b, has_ctrl, warm, policy, hf, false, first), before),
                            "model %d mode %d N=%d %s B=%d ctrl %d warm %d policy %d hf %d first %d: flag off differs", model, mode, N, k.name, b,
                            has_ctrl, warm, policy, hf, first);
                      const qmpc::qmpc_plan a = qmpc::plan_loop_instances(sel, b, has_ctrl, warm, policy, hf, true, first);
                      CHECK(!(a.fused && a.variant == 4), "N=%d %s B=%d: persistent with variant 4", N, k.name, b);
                      if (!has_ctrl || !warm) {
                        CHECK(same(a, before), "model %d mode %d N=%d %s B=%d ctrl %d warm %d policy %d: flag on differs without ctrl and warm",
                              model, mode, N, k.name, b, has_ctrl, warm, policy);
                        ++off;
                        continue;
                      }
                      CHECK(before.family == QMPC_KERNEL_NONE, "N=%d %s B=%d: the existing overload accepts ctrl with warm", N, k.name, b);
                      const qmpc::qmpc_plan inst = qmpc::plan_instances(sel, b);
                      const qmpc::qmpc_plan f = qmpc::plan(sel, b, qmpc::QMPC_CALL_WARM_LOOP, true, hf);
                      const bool pers = f.fused && qmpc::wform_index(f.variant) >= 0;
                      if (model != QMPC_MODEL_QUAT || mode != QMPC_MODE_CONVERGED || !sel.wform || (!pers && inst.family == QMPC_KERNEL_NONE)) {
                        CHECK(a.family == QMPC_KERNEL_NONE, "model %d mode %d N=%d %s B=%d: family %d, want NONE", model, mode, N, k.name, b, a.family);
                        ++none;
                        continue;
                      }
                      if (pers) {      // the rule of a call with plant records only
                        CHECK(same(a, f) && same(a, qmpc::plan_loop_instances(sel, b, false, true, policy, hf)),
                              "N=%d %s B=%d: persistent plan differs from the plant-only call's", N, k.name, b);
                        CHECK(b <= 4096 || sel.loop_fused == 1, "N=%d %s B=%d: persistent beyond 4096 robots", N, k.name, b);
                        ++persistent;
                        continue;
                      }
                      const bool forced = sel.variant == 4;
                      const bool lane_form = policy == QMPC_INSTANCES_AUTO && sel.lane_slot && (forced || (sel.variant == 0 && b >= sw));
                      if (!lane_form) {
                        qmpc::qmpc_plan w = inst;
                        w.fused = false;
                        CHECK(same(a, w), "N=%d %s B=%d policy %d: family %d variant %d, want the plan of qmpc_solve_instances*", N, k.name, b,
                              policy, a.family, a.variant);
                        CHECK(qmpc::wform_inst_warm_slot(a.variant) >= 0 && qmpc::wform_index(a.variant) >= 0 && !a.fused && a.iter_cap == 0,
                              "N=%d %s B=%d: variant %d without a slot", N, k.name, b, a.variant);
                        ++wave;
                        continue;
                      }
                      // the plain loop's warm tick (first tick) for this batch on a handle whose switch-over is not above it
                      qmpc::qmpc_select pl = sel;
                      if (pl.lane_min_warm > b) pl.lane_min_warm = b;
                      const qmpc::qmpc_plan pp =
                          qmpc::plan(pl, b, first ? qmpc::QMPC_CALL_WARM_LOOP_FIRST : qmpc::QMPC_CALL_WARM_LOOP_TICK, true, hf);
                      CHECK(pp.variant == 4, "N=%d %s B=%d: the plain warm tick is not a lane plan", N, k.name, b);
                      CHECK(same(a, pp), "N=%d %s B=%d hf %d first %d: family %d cap %d, plain warm tick family %d cap %d", N, k.name, b, hf, first,
                            a.family, a.iter_cap, pp.family, pp.iter_cap);
                      CHECK(a.variant == 4 && !a.upload_params && a.order_prev && !a.fused, "N=%d %s B=%d", N, k.name, b);
                      if (a.family == QMPC_KERNEL_LANE_HANDOFF) {
                        ++handoff;
                        CHECK(!hf && !forced && !first, "N=%d %s B=%d hf %d first %d: hand-off", N, k.name, b, hf, first);
                        CHECK(qmpc::wform_list_inst_slot(a.handoff_variant) >= 0 && a.iter_cap == sel.lane_cap_warm && a.iter_cap > 0 &&
                                  a.iter_cap < sel.iterations_max && (a.handoff_grid == 512 || a.handoff_grid == 1024) &&
                                  a.lds == sel.lds[0][a.handoff_variant] && a.gws == (a.handoff_variant == 5),
                              "N=%d %s B=%d: hand-off variant %d cap %d grid %d", N, k.name, b, a.handoff_variant, a.iter_cap, a.handoff_grid);
                      } else {
                        ++lane;
                        CHECK(a.family == QMPC_KERNEL_LANE && a.iter_cap == 0 && a.handoff_variant == 0, "N=%d %s B=%d: family %d", N, k.name, b,
                              a.family);
                      }
                      if (forced || first) CHECK(a.family == QMPC_KERNEL_LANE, "N=%d %s B=%d first %d: family %d", N, k.name, b, first, a.family);
                    }
          }
        }
  std::printf("loop warm records planner: %ld cases, %ld without ctrl and warm, %ld persistent, %ld wave, %ld lane, %ld lane with hand-off, %ld none\n",
              cases, off, persistent, wave, lane, handoff, none);
  CHECK(off > 0 && persistent > 0 && wave > 0 && lane > 0 && handoff > 0 && none > 0, "every branch visited");
  std::printf("%s: %d failures\n", failures ? "FAILED" : "passed", failures);
  return failures ? 1 : 0;
}
