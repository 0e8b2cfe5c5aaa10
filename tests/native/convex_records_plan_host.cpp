// Host-only check of the planner of ConvexMpc's calls with per-instance records (quaternion-mpc_amd/csrc/qmpc_plan.h:
// plan_convex_instances(s, batch) and plan_loop_instances(s, batch, has_ctrl, warm, policy, handoff_failed, warm_records, first,
// convex_records)), built like loop_warm_records_plan_host.cpp (hipcc -x hip --offload-host-only) over the same input space --
// every model, mode, horizon 1..32, knob set and the batch sizes around every switch-over, x ctrl x warm x policy x
// handoff_failed x warm_records x first x the setting:
//   plan_convex_instances: NONE exactly for another model or mode and without wrench-form kernels; never a dense or lane
//     family; the variant of the plain solve's plan on the wave kernels (lane_slot off) wherever that is 3 / 5 / 6; where the
//     plain plan falls to the round-1 family: 6 under plan()'s own condition for it (N >= 4, lds[6] <= 80 KB), else 5 if
//     lds[5] <= 80 KB, else 3 if it fits a CU, else NONE; LDS and workspace flag of the variant; a slot in the launch table;
//   setting off, or another model: the overload equals the existing last overload field for field;
//   setting on, ConvexMpc handle:
//     NONE for the reference mode, for ctrl with the warm start (whatever warm_records says) and for ctrl without wrench-form
//     kernels or where plan_convex_instances has none;
//     persistent: where the plain ConvexMpc loop's plan is fused on variant 3 / 5 / 6, that plan;
//     per tick: otherwise plan_convex_instances with ctrl, the plain loop's tick without; fused = false; the policy changes nothing.
// Prints the smallest batch that selects each variant at N = 10 and N = 20 with the default knobs, one summary line, and exits
// with status 0 when nothing failed.
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
    {"QMPC_LANE_MIN=1", "QMPC_LANE_MIN", "1", false},
    {"QMPC_LANE_INST_MIN=1", "QMPC_LANE_INST_MIN", "1", false},
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
bool wave_wform(const qmpc::qmpc_plan& p) { return p.family == QMPC_KERNEL_WFORM_LDS || p.family == QMPC_KERNEL_WFORM_WS; }

}  // namespace

int main() {
  long cases = 0, off = 0, persistent = 0, tick_ctrl = 0, tick_plant = 0, none = 0, solve_same = 0, solve_fallback = 0, solve_none = 0;
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
          const bool convex_ok = model == QMPC_MODEL_CONVEX && mode == QMPC_MODE_CONVERGED;
          std::set<int> batches = {1, 2, 65, 255, 256, 257, 512, 513, 1023, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 14335, 14336,
                                   16384, 20480, 32768, 65536, 262144};
          for (const auto& table : sel.lds)
            for (size_t lds : table)
              if (lds > 0)
                for (int d = -1; d <= 1; ++d) batches.insert(256 * (int)((160 * 1024) / lds) + d);
          for (int t : {sel.lane_min_batch, sel.lane_min_inst, sel.lane_min_loop_cold, sel.lane_min_warm, sel.lane_ref_min})
            for (int d = -1; d <= 1; ++d) batches.insert(t + d);
          const size_t* lds = sel.lds[0];
          int first_of[7] = {0, 0, 0, 0, 0, 0, 0};
          for (int b : batches) {
            if (b < 1) continue;
            // ---- the solve's plan ----
            const qmpc::qmpc_plan ci = qmpc::plan_convex_instances(sel, b);
            CHECK(ci.family == QMPC_KERNEL_NONE || wave_wform(ci), "model %d mode %d N=%d %s B=%d: family %d", model, mode, N, k.name, b, ci.family);
            CHECK(!ci.fused && ci.iter_cap == 0 && ci.handoff_variant == 0 && !ci.upload_params && !ci.order_prev, "N=%d %s B=%d: lane fields", N,
                  k.name, b);
            if (!convex_ok || !sel.wform) {
              CHECK(ci.family == QMPC_KERNEL_NONE, "model %d mode %d N=%d %s B=%d: family %d, want NONE", model, mode, N, k.name, b, ci.family);
              ++solve_none;
            } else {
              qmpc::qmpc_select w = sel;
              w.lane_slot = false;
              const qmpc::qmpc_plan pp = qmpc::plan(w, b, qmpc::QMPC_CALL_PLAIN, true, false);
              if (wave_wform(pp)) {
                CHECK(same(ci, pp), "N=%d %s B=%d: variant %d, the plain solve's %d", N, k.name, b, ci.variant, pp.variant);
                ++solve_same;
              } else {
                const int want = (N >= 4 && lds[6] <= 80 * 1024) ? 6 : lds[5] <= 80 * 1024 ? 5 : lds[3] <= 160 * 1024 ? 3 : 0;
                CHECK(ci.variant == want && (want != 0) == (ci.family != QMPC_KERNEL_NONE), "N=%d %s B=%d: variant %d, want %d", N, k.name, b,
                      ci.variant, want);
                ++solve_fallback;
              }
              if (ci.family != QMPC_KERNEL_NONE) {
                CHECK(qmpc::wform_convex_inst_slot(ci.variant) >= 0 && ci.lds == lds[ci.variant] && ci.lds <= 160 * 1024 &&
                          ci.gws == (ci.variant != 3) && ci.family == (ci.variant == 3 ? QMPC_KERNEL_WFORM_LDS : QMPC_KERNEL_WFORM_WS),
                      "N=%d %s B=%d: variant %d lds %zu gws %d", N, k.name, b, ci.variant, ci.lds, (int)ci.gws);
                if (!k.var && !k.no_slot && !first_of[ci.variant]) first_of[ci.variant] = b;
              }
            }
            // ---- the loops' plan ----
            for (int has_ctrl = 0; has_ctrl < 2; ++has_ctrl)
              for (int warm = 0; warm < 2; ++warm)
                for (int policy : {QMPC_INSTANCES_WAVE, QMPC_INSTANCES_AUTO})
                  for (int hf = 0; hf < 2; ++hf)
                    for (int wr = 0; wr < 2; ++wr)
                      for (int first = 0; first < 2; ++first) {
                        ++cases;
                        const qmpc::qmpc_plan before = qmpc::plan_loop_instances(sel, b, has_ctrl, warm, policy, hf, wr, first);
                        CHECK(same(qmpc::plan_loop_instances(sel, b, has_ctrl, warm, policy, hf, wr, first, false), before),
                              "model %d mode %d N=%d %s B=%d ctrl %d warm %d policy %d: setting off differs", model, mode, N, k.name, b, has_ctrl,
                              warm, policy);
                        const qmpc::qmpc_plan a = qmpc::plan_loop_instances(sel, b, has_ctrl, warm, policy, hf, wr, first, true);
                        if (model != QMPC_MODEL_CONVEX) {
                          CHECK(same(a, before), "model %d mode %d N=%d %s B=%d: setting on differs on another model", model, mode, N, k.name, b);
                          ++off;
                          continue;
                        }
                        CHECK(before.family == QMPC_KERNEL_NONE, "N=%d %s B=%d: the existing overload accepts a ConvexMpc handle", N, k.name, b);
                        CHECK(!(a.fused && a.variant == 4), "N=%d %s B=%d: persistent with variant 4", N, k.name, b);
                        if (mode != QMPC_MODE_CONVERGED || (has_ctrl && (warm || !sel.wform))) {
                          CHECK(a.family == QMPC_KERNEL_NONE, "mode %d N=%d %s B=%d ctrl %d warm %d: family %d, want NONE", mode, N, k.name, b,
                                has_ctrl, warm, a.family);
                          ++none;
                          continue;
                        }
                        const qmpc::qmpc_plan f = qmpc::plan(sel, b, warm ? qmpc::QMPC_CALL_WARM_LOOP : qmpc::QMPC_CALL_LOOP, true, hf);
                        if (f.fused && qmpc::wform_index(f.variant) >= 0) {
                          CHECK(same(a, f), "N=%d %s B=%d: persistent plan differs from the plain loop's", N, k.name, b);
                          CHECK(b <= (warm ? 4096 : 2048) || sel.loop_fused == 1, "N=%d %s B=%d: persistent beyond the threshold", N, k.name, b);
                          ++persistent;
                          continue;
                        }
                        qmpc::qmpc_plan want = has_ctrl ? ci
                                                        : qmpc::plan(sel, b, warm ? qmpc::QMPC_CALL_WARM_LOOP_TICK : qmpc::QMPC_CALL_LOOP_TICK, true, hf);
                        want.fused = false;
                        CHECK(same(a, want), "N=%d %s B=%d ctrl %d warm %d policy %d: family %d variant %d, want %d / %d", N, k.name, b, has_ctrl, warm,
                              policy, a.family, a.variant, want.family, want.variant);
                        if (has_ctrl) {
                          CHECK(a.family == QMPC_KERNEL_NONE || (wave_wform(a) && qmpc::wform_convex_inst_slot(a.variant) >= 0),
                                "N=%d %s B=%d: ctrl tick on family %d", N, k.name, b, a.family);
                          ++tick_ctrl;
                        } else {
                          ++tick_plant;
                        }
                      }
          }
          if (convex_ok && !k.var && !k.no_slot && (N == 10 || N == 20))
            std::printf("convex instances N=%d: smallest enumerated batch on variant 3: %d, 5: %d, 6: %d (lds %zu / %zu / %zu B)\n", N, first_of[3],
                        first_of[5], first_of[6], lds[3], lds[5], lds[6]);
        }
  std::printf("convex records planner: %ld loop cases, %ld on another model, %ld persistent, %ld per tick with ctrl, %ld per tick without, %ld none; "
              "solve: %ld the plain variant, %ld beyond it, %ld none\n",
              cases, off, persistent, tick_ctrl, tick_plant, none, solve_same, solve_fallback, solve_none);
  CHECK(off > 0 && persistent > 0 && tick_ctrl > 0 && tick_plant > 0 && none > 0 && solve_same > 0 && solve_fallback > 0 && solve_none > 0,
        "every branch visited");
  std::printf("%s: %d failures\n", failures ? "FAILED" : "passed", failures);
  return failures ? 1 : 0;
}
