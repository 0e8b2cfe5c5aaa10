// Host-only check of the policy-aware planner of qmpc_solve_instances* (quaternion-mpc_amd/csrc/qmpc_plan.h:
// plan_instances(s, batch, policy, has_info, handoff_failed)), built like instance_host.cpp (hipcc -x hip --offload-host-only)
// over the same input space -- every model, mode, horizon 1..32, knob set and the batch sizes around every switch-over:
//   WAVE  equals plan_instances(s, batch) everywhere;
//   AUTO  equals it where it is NONE, on a handle without a slot of the lane kernel's parameter table and below lane_min_inst;
//         from the switch-over on it carries exactly the lane fields of the plain solve's plan (the plain plan of a handle
//         whose own switch-over is not above the batch), for both values of has_info and handoff_failed;
//   QMPC_LANE_INST_MIN moves the switch-over, QMPC_VARIANT=4 selects the pure lane kernel at every batch size;
//   every plan names a kernel that exists (qmpc_kernel_slots.h).
// Prints one summary line; exit status 0 when nothing failed.
#define QMPC_FUSED_TU 1      // the templates of the kernel headers only: no kernel is instantiated here
#include "../../quaternion-mpc_amd/csrc/qmpc_kernels.hip"
#include "../../quaternion-mpc_amd/csrc/qmpc_wform.h"
#include "../../quaternion-mpc_amd/csrc/qmpc_plan_fill.h"
#include "../../quaternion-mpc_amd/csrc/qmpc_kernel_slots.h"

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
    {"QMPC_LANE_INST_MIN=1", "QMPC_LANE_INST_MIN", "1", false},
    {"QMPC_LANE_INST_MIN=40000", "QMPC_LANE_INST_MIN", "40000", false},
    {"QMPC_LANE_CAP=0", "QMPC_LANE_CAP", "0", false}, {"QMPC_LANE_CAP=12", "QMPC_LANE_CAP", "12", false},
    {"QMPC_LOOP_FUSED=1", "QMPC_LOOP_FUSED", "1", false},
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
  long cases = 0, wave = 0, lane = 0, handoff = 0, none = 0;
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
          // the knob and its defaults (one value up to N = 12, one beyond)
          if (k.var && std::strcmp(k.var, "QMPC_LANE_INST_MIN") == 0)
            CHECK(sel.lane_min_inst == std::atoi(k.value), "N=%d %s: lane_min_inst %d", N, k.name, sel.lane_min_inst);
          else
            CHECK(sel.lane_min_inst == (N <= 12 ? qmpc::kLaneMinInst : qmpc::kLaneMinInstLong), "N=%d %s: lane_min_inst %d", N, k.name,
                  sel.lane_min_inst);
          std::set<int> batches = {1, 2, 65, 255, 256, 257, 512, 513, 768, 769, 1023, 1024, 1025, 2048, 2049, 4096, 4097,
                                   8192, 14335, 14336, 16384, 32768, 39999, 40000, 65536, 262144};
          for (const auto& table : sel.lds)
            for (size_t lds : table)
              if (lds > 0)
                for (int d = -1; d <= 1; ++d) batches.insert(256 * (int)((160 * 1024) / lds) + d);
          for (int t : {sel.lane_min_batch, sel.lane_min_inst, sel.lane_min_loop_cold, sel.lane_min_warm, sel.lane_ref_min})
            for (int d = -1; d <= 1; ++d) batches.insert(t + d);
          for (int b : batches) {
            if (b < 1) continue;
            const qmpc::qmpc_plan w = qmpc::plan_instances(sel, b);
            for (int has_info = 0; has_info < 2; ++has_info)
              for (int hf = 0; hf < 2; ++hf) {
                ++cases;
                CHECK(same(qmpc::plan_instances(sel, b, QMPC_INSTANCES_WAVE, has_info, hf), w), "model %d mode %d N=%d %s B=%d: WAVE differs",
                      model, mode, N, k.name, b);
                const qmpc::qmpc_plan a = qmpc::plan_instances(sel, b, QMPC_INSTANCES_AUTO, has_info, hf);
                const bool forced = sel.variant == 4;
                if (w.family == QMPC_KERNEL_NONE || !sel.lane_slot || (!forced && b < sel.lane_min_inst) ||
                    (sel.variant != 0 && !forced)) {
                  CHECK(same(a, w), "model %d mode %d N=%d %s B=%d info %d hf %d: AUTO family %d, want the wave plan's %d", model, mode, N,
                        k.name, b, has_info, hf, a.family, w.family);
                  if (w.family == QMPC_KERNEL_NONE) ++none; else ++wave;
                  // the wave plan's kernel exists
                  if (w.family != QMPC_KERNEL_NONE) CHECK(qmpc::wform_index(a.variant) >= 0, "N=%d %s B=%d: variant %d", N, k.name, b, a.variant);
                  continue;
                }
                // the plain solve's plan for this batch on a handle whose plain switch-over is not above it
                qmpc::qmpc_select pl = sel;
                if (pl.lane_min_batch > b) pl.lane_min_batch = b;
                const qmpc::qmpc_plan pp = qmpc::plan(pl, b, qmpc::QMPC_CALL_PLAIN, has_info, hf);
                CHECK(pp.variant == 4, "N=%d %s B=%d: the plain plan is not a lane plan", N, k.name, b);
                CHECK(same(a, pp), "N=%d %s B=%d info %d hf %d: AUTO family %d cap %d, plain solve family %d cap %d", N, k.name, b, has_info, hf,
                      a.family, a.iter_cap, pp.family, pp.iter_cap);
                CHECK(a.variant == 4 && a.upload_params && !a.order_prev && !a.fused, "N=%d %s B=%d", N, k.name, b);
                if (a.family == QMPC_KERNEL_LANE_HANDOFF) {
                  ++handoff;
                  CHECK(has_info && !hf && !forced, "N=%d %s B=%d info %d hf %d: hand-off", N, k.name, b, has_info, hf);
                  CHECK(qmpc::wform_list_inst_slot(a.handoff_variant) >= 0 && a.iter_cap > 0 && a.iter_cap < sel.iterations_max &&
                            (a.handoff_grid == 512 || a.handoff_grid == 1024) && a.lds == sel.lds[0][a.handoff_variant] &&
                            a.gws == (a.handoff_variant == 5),
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
  std::printf("instance lane planner: %ld cases, %ld wave, %ld lane, %ld lane with hand-off, %ld none\n", cases, wave, lane, handoff, none);
  CHECK(wave > 0 && lane > 0 && handoff > 0 && none > 0, "every branch visited");
  std::printf("%s: %d failures\n", failures ? "FAILED" : "passed", failures);
  return failures ? 1 : 0;
}
