// Host-only checks of the per-instance parameter path (qmpc_solve_instances*), built like plan_host.cpp
// (hipcc -x hip --offload-host-only; no device code, no device needed):
//   apply_instance_params (qmpc_params_dev.h), the helper the expansion kernel runs, against fill_dev_params on a qmpc_params
//   carrying the same seven fields: byte for byte on 10000 random valid records; every kind of invalid record is rejected.
// (The planner of the call: records_plan_host.cpp --check instances.)
// Prints one summary line; exit status 0 when nothing failed.
#define QMPC_FUSED_TU 1      // the templates of the kernel headers only: no kernel is instantiated here
#include "../../quaternion-mpc_amd/csrc/qmpc_kernels.hip"
#include "../../quaternion-mpc_amd/csrc/qmpc_wform.h"
#include "../../quaternion-mpc_amd/csrc/qmpc_plan_fill.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

namespace {

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
  check_helper();
  std::printf("%s: %d failures\n", failures ? "FAILED" : "passed", failures);
  return failures ? 1 : 0;
}
