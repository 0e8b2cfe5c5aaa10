// Host-only checks of the planner of ConvexMpc's warm-started closed loops with controller records (quaternion-mpc_amd/csrc/
// qmpc_plan.h: plan_loop_instances; qmpc_opts::convex_warm), built like convex_lane_plan_host.cpp (hipcc -x hip
// --offload-host-only; no device code, no device needed).  Every model and mode, the horizons 1..32, the knob sets of
// convex_lane_plan_host.cpp, the batch sizes around every switch-over, ctrl x warm x first, every combination of the handle's settings.
//   setting off   every plan equals the planner before the setting existed, copied here verbatim, and so does every plan of a
//                 QuatMpc or 8-point handle with the setting on, and every plan without ctrl or without the warm start
//   setting on    ConvexMpc with ctrl and the warm start: NONE in the reference mode, without convex_records and without a
//                 wrench-form kernel; persistent where the plain warm-started loop is fused on variant 3 / 5 / 6 (never 4);
//                 otherwise per tick the wave plan of plan_convex_instances(s, batch); the lane form under QMPC_INSTANCES_AUTO with
//                 convex_lane on a handle with a lane slot from max(lane_min_cinst, lane_min_warm) (QMPC_VARIANT=4: every size),
//                 with the lane fields of the plain warm ConvexMpc tick
// Prints a summary and `passed: 0 failures`; exit status 0 when nothing failed.
#define QMPC_FUSED_TU 1      // the templates of the kernel headers only: no kernel is instantiated here
#include "../../quaternion-mpc_amd/csrc/qmpc_kernels.hip"
#include "../../quaternion-mpc_amd/csrc/qmpc_wform.h"
#include "../../quaternion-mpc_amd/csrc/qmpc_plan_fill.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

namespace {

using qmpc::qmpc_opts;
using qmpc::qmpc_plan;
using qmpc::qmpc_select;

struct Knobs {
  const char* name;
  const char* var;
  const char* value;
  bool no_slot;
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
    {"QMPC_LANE_MIN=30000", "QMPC_LANE_MIN", "30000", false},
    {"QMPC_LANE_INST_MIN=1", "QMPC_LANE_INST_MIN", "1", false},
    {"QMPC_LANE_CINST_MIN=1", "QMPC_LANE_CINST_MIN", "1", false},
    {"QMPC_LANE_CINST_MIN=3000", "QMPC_LANE_CINST_MIN", "3000", false},
    {"QMPC_LANE_CINST_MIN=40000", "QMPC_LANE_CINST_MIN", "40000", false},
    {"QMPC_LANE_CAP=12", "QMPC_LANE_CAP", "12", false},
    {"QMPC_LANE_CAP_LOOP=9", "QMPC_LANE_CAP_LOOP", "9", false},
    {"QMPC_LOOP_FUSED=0", "QMPC_LOOP_FUSED", "0", false},
    {"QMPC_LOOP_FUSED=1", "QMPC_LOOP_FUSED", "1", false},
};

bool same(const qmpc_plan& a, const qmpc_plan& b) {
  return a.family == b.family && a.variant == b.variant && a.lds == b.lds && a.gws == b.gws && a.handoff_variant == b.handoff_variant &&
         a.iter_cap == b.iter_cap && a.handoff_grid == b.handoff_grid && a.upload_params == b.upload_params && a.order_prev == b.order_prev &&
         a.fused == b.fused;
}

// plan_loop_instances as it was before qmpc_opts::convex_warm existed, verbatim
qmpc_plan loop_before(const qmpc_select& s, const qmpc_opts& o, int batch, bool has_ctrl, bool warm, bool first = false) {
  using namespace qmpc;
  const bool convex = s.model == QMPC_MODEL_CONVEX && o.convex_records;
  if ((s.model != QMPC_MODEL_QUAT && !convex) || s.mode != QMPC_MODE_CONVERGED) return qmpc_plan();
  if (has_ctrl && (!s.wform || (warm && (convex || !o.loop_warm_records)))) return qmpc_plan();
  const qmpc_plan f = plan(s, batch, warm ? QMPC_CALL_WARM_LOOP : QMPC_CALL_LOOP, true, o.handoff_failed);
  if (f.fused && (f.variant == 3 || f.variant == 5 || f.variant == 6)) return f;
  const qmpc_call tick = !warm ? QMPC_CALL_LOOP_TICK : (has_ctrl && first ? QMPC_CALL_WARM_LOOP_FIRST : QMPC_CALL_WARM_LOOP_TICK);
  qmpc_plan w = !has_ctrl ? plan(s, batch, tick, true, o.handoff_failed)
                : convex  ? plan_convex_instances(s, batch)
                          : plan_instances(s, qmpc_opts(), batch, true);
  w.fused = false;
  if (!has_ctrl || (convex && !o.convex_lane) || o.inst_policy != QMPC_INSTANCES_AUTO || w.family == QMPC_KERNEL_NONE || !s.lane_slot)
    return w;
  qmpc_select l = s;
  int& own = warm ? l.lane_min_warm : l.lane_min_loop_cold;
  const int inst_min = convex ? s.lane_min_cinst : s.lane_min_inst;
  if (s.variant != 4 && batch < (inst_min > own ? inst_min : own)) return w;
  own = 0;      // the switch-over is this call's own: the plain tick's plan only names the lane kernel's fields
  qmpc_plan p = plan(l, batch, tick, true, o.handoff_failed);
  if (p.variant != 4) return w;
  p.fused = false;
  return p;
}

long checks = 0, failures = 0, seen_fused = 0, seen_wave = 0, seen_lane = 0, seen_none = 0;
void fail(const char* what, const char* cfg, int batch, const qmpc_opts& o) {
  if (++failures <= 20)
    std::printf("FAIL %s: %s batch %d policy %d hf %d warm_records %d convex_records %d convex_lane %d convex_warm %d\n", what, cfg, batch,
                o.inst_policy, (int)o.handoff_failed, (int)o.loop_warm_records, (int)o.convex_records, (int)o.convex_lane, (int)o.convex_warm);
}
#define EXPECT(cond, what) do { ++checks; if (!(cond)) fail(what, cfg, b, o); } while (0)

}  // namespace

int main() {
  using namespace qmpc;
  for (int model = 0; model < 3; ++model)
    for (int mode = 0; mode < 2; ++mode)
      for (int N = 1; N <= 32; ++N)
        for (const Knobs& k : kKnobs) {
          qmpc_params params;
          std::memset(&params, 0, sizeof params);
          params.model = model;
          params.mode = mode;
          params.horizon = N;
          params.iterations_max = mode == QMPC_MODE_REFERENCE ? (model == QMPC_MODEL_CONVEX ? 5 : 10) : 120;
          auto env = [&k](const char* name) -> const char* { return (k.var && std::strcmp(name, k.var) == 0) ? k.value : nullptr; };
          qmpc_select s;
          if (!qmpc_fill_select(&s, &params, env, !k.no_slot)) continue;      // qmpc_create refuses the horizon
          char cfg[128];
          std::snprintf(cfg, sizeof cfg, "model %d mode %d N %d %s", model, mode, N, k.name);
          std::set<int> batches = {1, 2, 65, 1024, 1025, 2047, 2048, 2049, 2999, 3000, 3001, 4095, 4096, 4097, 8192, 16384, 29999, 30000, 30001,
                                   39999, 40000, 40001, 65536, 262144};
          for (const auto& table : s.lds)
            for (size_t lds : table)
              if (lds > 0)
                for (int d = -1; d <= 1; ++d) batches.insert(256 * (int)((160 * 1024) / lds) + d);
          for (int t : {s.lane_min_batch, s.lane_min_inst, s.lane_min_cinst, s.lane_min_loop_cold, s.lane_min_warm})
            for (int d = -1; d <= 1; ++d) batches.insert(t + d);
          batches.erase(batches.begin(), batches.lower_bound(1));
          const bool convex = model == QMPC_MODEL_CONVEX, conv_mode = mode == QMPC_MODE_CONVERGED;
          for (int bits = 0; bits < 64; ++bits) {
            qmpc_opts o;
            o.inst_policy = (bits & 1) ? QMPC_INSTANCES_AUTO : QMPC_INSTANCES_WAVE;
            o.handoff_failed = (bits & 2) != 0;
            o.loop_warm_records = (bits & 4) != 0;
            o.convex_records = (bits & 8) != 0;
            o.convex_lane = (bits & 16) != 0;
            o.convex_warm = (bits & 32) != 0;
            for (int b : batches) {
              // (the solves' planners do not read the setting: their signatures take it, their results do not change)
              qmpc_opts off = o;
              off.convex_warm = false;
              EXPECT(same(plan_convex_instances(s, o, b, true), plan_convex_instances(s, off, b, true)), "plan_convex_instances ignores the setting");
              EXPECT(same(plan_instances(s, o, b, true), plan_instances(s, off, b, true)), "plan_instances ignores the setting");
              for (int f = 0; f < 8; ++f) {
                const bool has_ctrl = f & 1, warm = (f & 2) != 0, first = (f & 4) != 0;
                const qmpc_plan p = plan_loop_instances(s, o, b, has_ctrl, warm, first);
                const qmpc_plan before = loop_before(s, o, b, has_ctrl, warm, first);
                EXPECT(!(p.fused && p.variant == 4), "never fused on variant 4");
                if (!o.convex_warm || !convex || !has_ctrl || !warm) {
                  EXPECT(same(p, before), "setting off, another model, no ctrl or no warm start: the plan is unchanged");
                  continue;
                }
                // ---- ConvexMpc, setting on, ctrl with the warm start ----
                if (!conv_mode || !o.convex_records || !s.wform) {
                  EXPECT(p.family == QMPC_KERNEL_NONE, "reference mode / no convex_records / no wrench form: refused");
                  ++seen_none;
                  continue;
                }
                const qmpc_plan plain = plan(s, b, QMPC_CALL_WARM_LOOP, true, o.handoff_failed);
                if (plain.fused && (plain.variant == 3 || plain.variant == 5 || plain.variant == 6)) {
                  EXPECT(same(p, plain), "persistent: the plain warm-started loop's plan");
                  EXPECT(s.loop_fused == 1 || b <= 4096, "persistent: up to 4096 robots unless forced");
                  ++seen_fused;
                  continue;
                }
                qmpc_plan wave = plan_convex_instances(s, b);
                wave.fused = false;
                const int own = s.lane_min_warm;
                const bool lane = o.convex_lane && o.inst_policy == QMPC_INSTANCES_AUTO && s.lane_slot && wave.family != QMPC_KERNEL_NONE &&
                                  (s.variant == 4 || (s.variant == 0 && b >= (s.lane_min_cinst > own ? s.lane_min_cinst : own)));
                if (!lane) {
                  EXPECT(same(p, wave), "per tick, wave: plan_convex_instances(s, batch), first or not");
                  if (p.family == QMPC_KERNEL_NONE) ++seen_none; else ++seen_wave;
                  continue;
                }
                ++seen_lane;
                qmpc_select l = s;
                l.lane_min_warm = 0;
                qmpc_plan tick = plan(l, b, first ? QMPC_CALL_WARM_LOOP_FIRST : QMPC_CALL_WARM_LOOP_TICK, true, o.handoff_failed);
                EXPECT(same(p, tick), "lane tick: the fields of the plain warm ConvexMpc tick");
                EXPECT(p.variant == 4 && p.family == QMPC_KERNEL_LANE && !p.upload_params && p.order_prev && !p.fused && p.iter_cap == 0 &&
                           p.handoff_variant == 0 && p.handoff_grid == 0,
                       "lane tick: variant 4, LANE, order_prev, no upload, no cap, no hand-off, not fused");
              }
            }
          }
        }
  std::printf("convex warm planner: %ld checks\n", checks);
  std::printf("plans seen under the setting: persistent %ld, wave %ld, lane %ld, refused %ld\n", seen_fused, seen_wave, seen_lane, seen_none);
  std::printf("passed: %ld failures\n", failures);
  return failures ? 1 : 0;
}
