// Host-only checks of the per-instance parameter path (qmpc_solve_instances*), built like plan_host.cpp
// (hipcc -x hip --offload-host-only; no device code, no device needed):
//   (a) plan_instances (quaternion-mpc_amd/csrc/qmpc_plan.h) over every model, mode, horizon 1..32, the knob sets of plan_host.cpp
//       and the batch sizes around every switch-over: QuatMpc's problem in the converged mode takes a wave wrench-form kernel
//       (never the lane kernel), the very variant, LDS and workspace of a plain solve wherever that solve is a wave kernel, and
//       NONE where the plain solve would take no wrench-form kernel; every other handle gets NONE.
//   (b) apply_instance_params (qmpc_params_dev.h), the helper the expansion kernel runs, against fill_dev_params on a qmpc_params
//       carrying the same seven fields: byte for byte on 10000 random valid records; every kind of invalid record is rejected.
// Prints one summary line per part; exit status 0 when nothing failed.
#define QMPC_FUSED_TU 1      // the templates of the kernel headers only: no kernel is instantiated here
#include "../../quaternion-mpc_amd/csrc/qmpc_kernels.hip"
#include "../../quaternion-mpc_amd/csrc/qmpc_wform.h"
#include "../../quaternion-mpc_amd/csrc/qmpc_plan_fill.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <set>

namespace {

struct Knobs {
  const char* name;
  const char* var;
  const char* value;
  bool no_slot;
  int handoff_failed;
};
const Knobs kKnobs[] = {
    {"default", nullptr, nullptr, false, 0},       {"QMPC_VARIANT=1", "QMPC_VARIANT", "1", false, 0},
    {"QMPC_VARIANT=2", "QMPC_VARIANT", "2", false, 0}, {"QMPC_VARIANT=3", "QMPC_VARIANT", "3", false, 0},
    {"QMPC_VARIANT=4", "QMPC_VARIANT", "4", false, 0}, {"QMPC_WFORM=0", "QMPC_WFORM", "0", false, 0},
    {"QMPC_WFORM=3", "QMPC_WFORM", "3", false, 0},     {"no-lane-slot", nullptr, nullptr, true, 0},
    {"handoff-failed", nullptr, nullptr, false, 1},
    {"QMPC_VARIANT=4 handoff-failed", "QMPC_VARIANT", "4", false, 1},
    {"QMPC_LANE_MIN=8192", "QMPC_LANE_MIN", "8192", false, 0},
    {"QMPC_LANE_REF_MIN=8192", "QMPC_LANE_REF_MIN", "8192", false, 0},
    {"QMPC_LANE_CAP=0", "QMPC_LANE_CAP", "0", false, 0},     {"QMPC_LANE_CAP=12", "QMPC_LANE_CAP", "12", false, 0},
    {"QMPC_LANE_CAP_LOOP=0", "QMPC_LANE_CAP_LOOP", "0", false, 0}, {"QMPC_LANE_CAP_WARM=0", "QMPC_LANE_CAP_WARM", "0", false, 0},
    {"QMPC_LOOP_FUSED=0", "QMPC_LOOP_FUSED", "0", false, 0}, {"QMPC_LOOP_FUSED=1", "QMPC_LOOP_FUSED", "1", false, 0},
    {"QMPC_REF_WFORM_MAXN=12", "QMPC_REF_WFORM_MAXN", "12", false, 0},
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

bool wform_family(int f) { return f == QMPC_KERNEL_WFORM_LDS || f == QMPC_KERNEL_WFORM_WS; }
bool lane_family(int f) { return f == QMPC_KERNEL_LANE || f == QMPC_KERNEL_LANE_HANDOFF; }

void check_planner() {
  long cases = 0, wave_equal = 0, above_lane = 0, none = 0;
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
          std::set<int> batches = {1, 2, 255, 256, 257, 512, 513, 768, 769, 1023, 1024, 1025, 2048, 2049, 4096, 4097,
                                   8192, 14335, 14336, 16384, 32768, 65536, 262144};
          for (const auto& table : sel.lds)
            for (size_t lds : table)
              if (lds > 0)
                for (int d = -1; d <= 1; ++d) batches.insert(256 * (int)((160 * 1024) / lds) + d);
          for (int t : {sel.lane_min_batch, sel.lane_min_loop_cold, sel.lane_min_warm, sel.lane_ref_min, qmpc::kLaneRefMinLoop})
            for (int d = -1; d <= 1; ++d) batches.insert(t + d);
          const bool supported = model == QMPC_MODEL_QUAT && mode == QMPC_MODE_CONVERGED && sel.wform;
          for (int b : batches) {
            if (b < 1) continue;
            ++cases;
            const qmpc::qmpc_plan r = qmpc::plan_instances(sel, b);
            const qmpc::qmpc_plan pp = qmpc::plan(sel, b, qmpc::QMPC_CALL_PLAIN, true, k.handoff_failed);
            CHECK(!lane_family(r.family) && r.family != QMPC_KERNEL_DENSE_LDS && r.family != QMPC_KERNEL_DENSE_WS,
                  "model %d mode %d N=%d %s B=%d: family %d", model, mode, N, k.name, b, r.family);
            if (!supported) {
              CHECK(r.family == QMPC_KERNEL_NONE, "model %d mode %d N=%d %s B=%d: family %d, want none", model, mode, N, k.name, b,
                    r.family);
              continue;
            }
            if (r.family == QMPC_KERNEL_NONE) {
              ++none;
            } else {
              CHECK(r.variant == 3 || r.variant == 5 || r.variant == 6, "N=%d %s B=%d: variant %d", N, k.name, b, r.variant);
              CHECK(r.family == (r.variant == 3 ? QMPC_KERNEL_WFORM_LDS : QMPC_KERNEL_WFORM_WS), "N=%d %s B=%d", N, k.name, b);
              CHECK(r.lds == sel.lds[0][r.variant] && r.gws == (r.variant != 3), "N=%d %s B=%d: lds %zu gws %d", N, k.name, b, r.lds,
                    (int)r.gws);
              CHECK(r.handoff_variant == 0 && r.iter_cap == 0 && !r.fused, "N=%d %s B=%d", N, k.name, b);
            }
            if (lane_family(pp.family)) {
              ++above_lane;
              // the default knobs leave the wrench form at every batch size: the workspace form beyond the lane switch-over
              if (!k.var) CHECK(wform_family(r.family), "N=%d %s B=%d: none above the lane switch-over", N, k.name, b);
            } else if (wform_family(pp.family)) {
              ++wave_equal;
              CHECK(r.family == pp.family && r.variant == pp.variant && r.lds == pp.lds && r.gws == pp.gws,
                    "N=%d %s B=%d: variant %d, plain solve %d", N, k.name, b, r.variant, pp.variant);
            } else {
              CHECK(r.family == QMPC_KERNEL_NONE, "N=%d %s B=%d: family %d where the plain solve takes family %d", N, k.name, b,
                    r.family, pp.family);
            }
          }
        }
  std::printf("planner: %ld cases, %ld equal to a plain wave-kernel solve, %ld beyond the lane switch-over, %ld none\n", cases,
              wave_equal, above_lane, none);
}

// counter-based uniform draws in [0, 1)
uint64_t mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
struct Rng {
  uint64_t s;
  double u() { s += 0x9E3779B97F4A7C15ull; return (double)(mix(s) >> 11) * (1.0 / 9007199254740992.0); }
  double in(double a, double b) { return a + (b - a) * u(); }
};

void go1_like(qmpc_params* p) {
  std::memset(p, 0, sizeof *p);
  p->horizon = 10;
  p->h = 0.025f;
  p->h_ref = 0.025;
  p->mass = 13.0;
  const double I[9] = {0.0202, 0.0, 0.0, 0.0, 0.0756, 0.0, 0.0, 0.0, 0.0860};
  std::memcpy(p->inertia, I, sizeof I);
  for (int j = 0; j < 13; ++j) p->q_weights[j] = 1.0 + j;
  for (int j = 0; j < 12; ++j) p->r_weights[j] = 1e-5;
  p->w = 10.0;
  p->mu = 0.6;
  p->fz_max = 150.0;
  p->mode = QMPC_MODE_CONVERGED;
  p->iterations_max = 120;
  p->tol_feasibility = 1e-6;
  p->tol_step = 1e-8;
  p->ipm_mu0 = 1.0;
  p->ipm_mu_final = 1e-9;
  p->ipm_sigma = 0.1;
  p->ipm_sigma_fast = 0.01;
  p->ipm_tau = 0.99;
  p->drop_ang_vel = 1;
  p->model = QMPC_MODEL_QUAT;
}

void put(qmpc_params* p, const qmpc_instance_params& r) {
  p->mass = r.mass;
  std::memcpy(p->inertia, r.inertia, sizeof r.inertia);
  p->mu = r.mu;
  p->fz_max = r.fz_max;
  std::memcpy(p->q_weights, r.q_weights, sizeof r.q_weights);
  std::memcpy(p->r_weights, r.r_weights, sizeof r.r_weights);
  p->w = r.w;
}

void check_helper() {
  qmpc_params p0;
  go1_like(&p0);
  qmpc::DevParams base;
  CHECK(qmpc::fill_dev_params(&p0, &base) == QMPC_OK, "base parameters");
  Rng rng{12345};
  int valid = 0;
  auto random_record = [&]() {
    qmpc_instance_params r;
    r.mass = rng.in(5.0, 25.0);
    // a symmetric positive definite inertia with off-diagonal terms (every cofactor product matters)
    double d[3], o[3];
    for (double& x : d) x = rng.in(0.01, 0.2);
    for (double& x : o) x = rng.in(-0.004, 0.004);
    const double I[9] = {d[0], o[0], o[1], o[0], d[1], o[2], o[1], o[2], d[2]};
    std::memcpy(r.inertia, I, sizeof I);
    r.mu = rng.in(0.1, 1.2);
    r.fz_max = rng.in(20.0, 400.0);
    for (double& q : r.q_weights) q = rng.u() < 0.1 ? 0.0 : rng.in(0.0, 500.0);
    for (double& x : r.r_weights) x = rng.in(1e-7, 1e-3);
    r.w = rng.u() < 0.1 ? 0.0 : rng.in(0.0, 100.0);
    return r;
  };
  for (int i = 0; i < 10000; ++i) {
    const qmpc_instance_params r = random_record();
    qmpc::DevParams a, b;
    std::memset(&a, 0x5A, sizeof a);
    const int st = qmpc::apply_instance_params(base, r, &a);
    qmpc_params p = p0;
    put(&p, r);
    CHECK(st == QMPC_OK, "record %d rejected", i);
    CHECK(qmpc::fill_dev_params(&p, &b) == QMPC_OK, "record %d: fill_dev_params", i);
    // byte for byte over the fields (the struct's tail padding is not a value)
    CHECK(std::memcmp(&a, &b, offsetof(qmpc::DevParams, linesearch_max) + sizeof(int)) == 0, "record %d differs", i);
    valid += st == QMPC_OK;
  }
  // every kind of invalid record, planted in an otherwise valid one
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  int kinds = 0;
  auto rejected = [&](const char* what, void (*edit)(qmpc_instance_params*, double), double v) {
    qmpc_instance_params r = random_record();
    edit(&r, v);
    qmpc::DevParams a;
    CHECK(qmpc::apply_instance_params(base, r, &a) == QMPC_BAD_PARAMS, "%s (%g) accepted", what, v);
    ++kinds;
  };
  for (int slot = 0; slot < 38; ++slot)
    for (double v : {nan, inf, -inf}) {
      qmpc_instance_params r = random_record();
      (&r.mass)[slot] = v;
      qmpc::DevParams a;
      CHECK(qmpc::apply_instance_params(base, r, &a) == QMPC_BAD_PARAMS, "non-finite field %d (%g) accepted", slot, v);
      ++kinds;
    }
  for (double v : {0.0, -1.0, -0.0}) rejected("mass", [](qmpc_instance_params* r, double x) { r->mass = x; }, v);
  rejected("zero inertia", [](qmpc_instance_params* r, double) { std::memset(r->inertia, 0, sizeof r->inertia); }, 0.0);
  rejected("rank-1 inertia", [](qmpc_instance_params* r, double) {
    const double I[9] = {1, 2, 3, 2, 4, 6, 3, 6, 9};
    std::memcpy(r->inertia, I, sizeof I);
  }, 0.0);
  rejected("rank-2 inertia", [](qmpc_instance_params* r, double) {
    const double I[9] = {0.1, 0, 0, 0, 0.2, 0, 0, 0, 0};
    std::memcpy(r->inertia, I, sizeof I);
  }, 0.0);
  for (double v : {0.0, -1e-6}) {
    rejected("r_weight 0", [](qmpc_instance_params* r, double x) { r->r_weights[0] = x; }, v);
    rejected("r_weight 11", [](qmpc_instance_params* r, double x) { r->r_weights[11] = x; }, v);
    rejected("mu", [](qmpc_instance_params* r, double x) { r->mu = x; }, v);
    rejected("fz_max", [](qmpc_instance_params* r, double x) { r->fz_max = x; }, v);
  }
  rejected("q_weight 0", [](qmpc_instance_params* r, double x) { r->q_weights[0] = x; }, -1.0);
  rejected("q_weight 12", [](qmpc_instance_params* r, double x) { r->q_weights[12] = x; }, -1e-9);
  rejected("w", [](qmpc_instance_params* r, double x) { r->w = x; }, -0.5);
  std::printf("helper: %d valid records equal to fill_dev_params byte for byte, %d invalid records checked\n", valid, kinds);
}

}  // namespace

int main() {
  check_planner();
  check_helper();
  std::printf("%s: %d failures\n", failures ? "FAILED" : "passed", failures);
  return failures ? 1 : 0;
}
