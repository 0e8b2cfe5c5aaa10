// Host-only checks of the closed loop with per-robot records (qmpc_loop_run_instances*), built like instance_host.cpp
// (hipcc -x hip --offload-host-only; no device code, no device needed):
//   (a) apply_plant_params (qmpc_params_dev.h): a valid record's inverse inertia equals fill_dev_params' bit for bit; every kind
//       of invalid record (non-finite field, mass <= 0, singular inertia) is rejected.
//   (b) plant_step_ext (qmpc_loop_math.h) with a zero disturbance against plant_step on random states and forces: bit for bit,
//       -0.0 components included; a non-zero component changes the step.
// (The planner of the call: records_plan_host.cpp --check loop.)
// Prints one summary line per part; exit status 0 when nothing failed.
#define QMPC_FUSED_TU 1      // the templates of the kernel headers only: no kernel is instantiated here
#include "../../quaternion-mpc_amd/csrc/qmpc_kernels.hip"
#include "../../quaternion-mpc_amd/csrc/qmpc_wform.h"
#include "../../quaternion-mpc_amd/csrc/qmpc_loop_math.h"
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

void go1_like(qmpc_params* p, Rng& r) {
  std::memset(p, 0, sizeof *p);
  p->horizon = 10;
  p->h = 0.025f;
  p->h_ref = 0.025;
  p->mass = r.in(8.0, 18.0);
  const double d[3] = {r.in(0.01, 0.03), r.in(0.04, 0.09), r.in(0.05, 0.1)};
  for (int i = 0; i < 9; ++i) p->inertia[i] = 0.0;
  for (int i = 0; i < 3; ++i) p->inertia[4 * i] = d[i];
  p->inertia[1] = p->inertia[3] = r.in(-0.002, 0.002);       // symmetric off-diagonals
  p->inertia[5] = p->inertia[7] = r.in(-0.002, 0.002);
  p->mu = 0.6;
  p->fz_max = 150.0;
  for (int i = 0; i < 13; ++i) p->q_weights[i] = 1.0;
  for (int i = 0; i < 12; ++i) p->r_weights[i] = 1e-4;
  p->w = 1e-3;
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

void check_plant_rule() {
  Rng r{11};
  long equal = 0;
  for (int k = 0; k < 10000; ++k) {
    qmpc_params p;
    go1_like(&p, r);
    qmpc::DevParams d;
    if (qmpc::fill_dev_params(&p, &d) != QMPC_OK) { CHECK(false, "fill_dev_params rejected record %d", k); continue; }
    qmpc_plant_params rec;
    std::memset(&rec, 0, sizeof rec);
    rec.mass = p.mass;
    std::memcpy(rec.inertia, p.inertia, sizeof rec.inertia);
    rec.ext_force_world[0] = r.in(-20, 20);
    rec.ext_torque_body[2] = r.in(-2, 2);
    qmpc::PlantDev pl;
    CHECK(qmpc::apply_plant_params(rec, &pl) == QMPC_OK && pl.status == QMPC_OK, "record %d rejected", k);
    const bool same = std::memcmp(pl.Iinv, d.Iinv, sizeof pl.Iinv) == 0 && pl.mass == d.mass &&
                      pl.force[0] == rec.ext_force_world[0] && pl.torque[2] == rec.ext_torque_body[2];
    CHECK(same, "record %d: plant block differs from fill_dev_params", k);
    equal += same;
  }
  // every kind of invalid record
  qmpc_params p;
  go1_like(&p, r);
  qmpc_plant_params good;
  std::memset(&good, 0, sizeof good);
  good.mass = p.mass;
  std::memcpy(good.inertia, p.inertia, sizeof good.inertia);
  int rejected = 0, kinds = 0;
  const double bad_values[3] = {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(),
                                -std::numeric_limits<double>::infinity()};
  for (int f = 0; f < 16; ++f)
    for (double v : bad_values) {
      qmpc_plant_params b = good;
      (&b.mass)[f] = v;
      qmpc::PlantDev pl;
      ++kinds;
      const int st = qmpc::apply_plant_params(b, &pl);
      rejected += st == QMPC_BAD_PARAMS && pl.status == QMPC_BAD_PARAMS;
      CHECK(st == QMPC_BAD_PARAMS, "field %d = %g accepted", f, v);
    }
  for (double m : {0.0, -0.0, -3.0}) {
    qmpc_plant_params b = good;
    b.mass = m;
    qmpc::PlantDev pl;
    ++kinds;
    const int st = qmpc::apply_plant_params(b, &pl);
    rejected += st == QMPC_BAD_PARAMS;
    CHECK(st == QMPC_BAD_PARAMS, "mass %g accepted", m);
  }
  {
    qmpc_plant_params b = good;
    for (int c = 0; c < 3; ++c) b.inertia[6 + c] = b.inertia[3 + c];    // two equal rows: singular
    qmpc::PlantDev pl;
    ++kinds;
    const int st = qmpc::apply_plant_params(b, &pl);
    rejected += st == QMPC_BAD_PARAMS;
    CHECK(st == QMPC_BAD_PARAMS, "singular inertia accepted");
  }
  std::printf("plant rule: 10000 valid records equal fill_dev_params' blocks (%ld), %d of %d invalid records rejected\n", equal,
              rejected, kinds);
}

void check_plant_step() {
  Rng r{23};
  long same = 0, moved = 0;
  const int n = 20000;
  for (int k = 0; k < n; ++k) {
    double x[13], feet[12], u[12], Iinv[9];
    for (int a = 0; a < 3; ++a) x[a] = r.in(-1, 1);
    double q[4], nq = 0.0;
    for (int a = 0; a < 4; ++a) { q[a] = r.in(-1, 1); nq += q[a] * q[a]; }
    for (int a = 0; a < 4; ++a) x[3 + a] = q[a] / std::sqrt(nq);
    for (int a = 7; a < 13; ++a) x[a] = r.in(-2, 2);
    if (k % 3 == 0) { x[7] = -0.0; x[11] = -0.0; }       // signed zeros must survive
    for (int a = 0; a < 12; ++a) { feet[a] = r.in(-0.5, 0.5); u[a] = (k % 5 == 0 && a % 3 != 2) ? -0.0 : r.in(-60, 60); }
    for (int a = 0; a < 9; ++a) Iinv[a] = (a % 4 == 0) ? r.in(10, 60) : r.in(-1, 1);
    const double mass = r.in(8, 18), dt = 0.005;
    const double zf[3] = {0.0, -0.0, 0.0}, zt[3] = {-0.0, 0.0, 0.0};
    double a1[13], a2[13];
    std::memcpy(a1, x, sizeof x);
    std::memcpy(a2, x, sizeof x);
    qmpc_loop::plant_step(a1, u, feet, 4, mass, Iinv, dt);
    qmpc_loop::plant_step_ext(a2, u, feet, 4, mass, Iinv, zf, zt, dt);
    const bool eq = std::memcmp(a1, a2, sizeof a1) == 0;
    CHECK(eq, "state %d: zero disturbance changed the step", k);
    same += eq;
    const double f[3] = {0.0, 0.0, r.in(1, 5)}, t[3] = {0.0, r.in(0.1, 1), 0.0};
    double a3[13];
    std::memcpy(a3, x, sizeof x);
    qmpc_loop::plant_step_ext(a3, u, feet, 4, mass, Iinv, f, t, dt);
    moved += a3[9] > a1[9] && std::memcmp(a3, a1, sizeof a1) != 0;
  }
  CHECK(moved == n, "a disturbance left %ld of %d steps unchanged", n - moved, n);
  std::printf("plant step: %ld of %d zero-disturbance steps equal plant_step bit for bit; %ld disturbed steps moved\n", same, n, moved);
}

}  // namespace

int main() {
  check_plant_rule();
  check_plant_step();
  std::printf("passed: %d failures\n", failures);
  return failures ? 1 : 0;
}
