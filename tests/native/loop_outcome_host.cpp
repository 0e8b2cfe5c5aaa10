// Host-only checks of the outcome step of the closed loop (qmpc_loop_run_outcomes*), built like loop_instances_host.cpp
// (hipcc -x hip --offload-host-only; no device code, no device needed): loop_outcome_one (qmpc_loop_math.h) over hand-made state
// sequences, every field against values worked out here.
//   (a) the first tick on an empty record and two more: selections, the velocity error in the BODY frame (a robot turned by 180
//       degrees about z), the status counters, a tilt beyond the threshold sets down_tick, and the record is frozen afterwards
//   (b) the down rule: a NaN height, a NaN attitude, a height just below / exactly at the threshold
//   (c) accumulation over two segments equals accumulation over one, byte for byte
// The numbers of (a) are dyadic fractions, so every expected value is exact; the one inexact value (the upright value of a
// (0.8, 0.6, 0, 0) attitude) is allowed 4 ulp.
// Prints one summary line per part; exit status 0 when nothing failed.
#include "../../quaternion-mpc_amd/csrc/qmpc_loop_math.h"

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

const double kInf = std::numeric_limits<double>::infinity();
const double kNan = std::numeric_limits<double>::quiet_NaN();

qmpc_loop_outcome empty_record() {      // what qmpc_loop_outcome_init writes (tests/test_loop_outcome_cpu.py compares the two)
  qmpc_loop_outcome o;
  std::memset(&o, 0, sizeof o);
  o.down_tick = o.first_rejected_tick = -1.0;
  o.min_height = o.min_upright = kInf;
  o.max_height_err = o.max_vel_err = o.max_ang_vel = o.max_force_z = o.iterations_max = -kInf;
  return o;
}

qmpc_outcome_params default_op() { return qmpc_outcome_params{0.15, 0.5, 0.0, 0.0}; }

// a state with the fields the outcome step reads; everything else zero
qmpc_loop_state state(double tick, double z, double joy_z, const double (&q)[4], const double (&v)[3], const double (&vd)[2],
                      const double (&w)[3], const double (&fz)[4], int status, int iterations) {
  qmpc_loop_state s;
  std::memset(&s, 0, sizeof s);
  s.pos_world[0] = 3.0; s.pos_world[1] = -2.0; s.pos_world[2] = z;
  s.joy[2] = joy_z;
  for (int a = 0; a < 4; ++a) s.quat[a] = q[a];
  for (int a = 0; a < 3; ++a) { s.lin_vel_world[a] = v[a]; s.ang_vel_body[a] = w[a]; }
  s.lin_vel_d_rel[0] = vd[0]; s.lin_vel_d_rel[1] = vd[1];
  for (int l = 0; l < 4; ++l) { s.forces_body[3 * l] = 1000.0; s.forces_body[3 * l + 1] = -1000.0; s.forces_body[3 * l + 2] = fz[l]; }
  s.status = (double)status;
  s.iterations = (double)iterations;
  s.tick = tick;
  return s;
}

void check_sequence() {
  const qmpc_outcome_params op = default_op();
  qmpc_loop_outcome o = empty_record();
  // tick 1: upright robot; body velocity (0.5, 0.75) against (0.125, 0.25): e = (0.375, 0.5), |e| = 0.625
  qmpc_loop::loop_outcome_one(op, state(1.0, 0.3125, 0.25, {1, 0, 0, 0}, {0.5, 0.75, 0.125}, {0.125, 0.25}, {0.125, -0.75, 0.25},
                                        {10.0, 40.0, -5.0, 20.0}, QMPC_OK, 7), o);
  CHECK(o.ticks == 1.0 && o.down_tick == -1.0, "%g %g", o.ticks, o.down_tick);
  CHECK(o.min_height == 0.3125 && o.min_upright == 1.0, "%g %g", o.min_height, o.min_upright);
  CHECK(o.max_height_err == 0.0625, "%g", o.max_height_err);
  CHECK(o.max_vel_err == 0.625 && o.sum_vel_err_sq == 0.390625, "%g %g", o.max_vel_err, o.sum_vel_err_sq);
  CHECK(o.max_ang_vel == 0.75 && o.max_force_z == 40.0, "%g %g", o.max_ang_vel, o.max_force_z);
  CHECK(o.not_ok_ticks == 0.0 && o.rejected_ticks == 0.0 && o.first_rejected_tick == -1.0, "%g %g %g", o.not_ok_ticks, o.rejected_ticks,
        o.first_rejected_tick);
  CHECK(o.iterations_sum == 7.0 && o.iterations_max == 7.0, "%g %g", o.iterations_sum, o.iterations_max);
  CHECK(o.reserved[0] == 0.0 && o.reserved[1] == 0.0, "reserved");
  // tick 2: turned by 180 degrees about z, R = diag(-1, -1, 1): the body velocity is (-0.5, -0.75), against (0.25, 0.25):
  // e = (-0.75, -1), |e| = 1.25; the solve hit its iteration cap (not OK, but applied)
  qmpc_loop::loop_outcome_one(op, state(2.0, 0.28125, 0.25, {0, 0, 0, 1}, {0.5, 0.75, -4.0}, {0.25, 0.25}, {0.0, 0.0, -0.875},
                                        {5.0, 5.0, 5.0, 5.0}, QMPC_MAX_ITER, 120), o);
  CHECK(o.ticks == 2.0 && o.down_tick == -1.0, "%g %g", o.ticks, o.down_tick);
  CHECK(o.min_height == 0.28125 && o.min_upright == 1.0 && o.max_height_err == 0.0625, "%g %g %g", o.min_height, o.min_upright,
        o.max_height_err);
  CHECK(o.max_vel_err == 1.25 && o.sum_vel_err_sq == 0.390625 + 1.5625, "%g %g", o.max_vel_err, o.sum_vel_err_sq);
  CHECK(o.max_ang_vel == 0.875 && o.max_force_z == 40.0, "%g %g", o.max_ang_vel, o.max_force_z);
  CHECK(o.not_ok_ticks == 1.0 && o.rejected_ticks == 0.0 && o.first_rejected_tick == -1.0, "%g %g %g", o.not_ok_ticks, o.rejected_ticks,
        o.first_rejected_tick);
  CHECK(o.iterations_sum == 127.0 && o.iterations_max == 120.0, "%g %g", o.iterations_sum, o.iterations_max);
  // tick 3: rolled by 2 atan(0.6 / 0.8) = 73.7 degrees: upright = 1 - 2 (0.6^2 + 0) = 0.28 < 0.5 -- down, at full height; the solve was
  // rejected (NaN input), a larger force and fewer iterations
  qmpc_loop::loop_outcome_one(op, state(3.0, 0.375, 0.25, {0.8, 0.6, 0, 0}, {0, 0, 0}, {0, 0}, {0, 0, 0}, {5.0, 5.0, 90.0, 5.0},
                                        QMPC_NAN_INPUT, 0), o);
  CHECK(o.ticks == 3.0 && o.down_tick == 3.0, "%g %g", o.ticks, o.down_tick);
  CHECK(o.min_height == 0.28125 && std::fabs(o.min_upright - 0.28) <= 4 * 0.28 * std::numeric_limits<double>::epsilon(), "%g %.17g",
        o.min_height, o.min_upright);
  CHECK(o.max_height_err == 0.125 && o.max_vel_err == 1.25 && o.sum_vel_err_sq == 1.953125, "%g %g %g", o.max_height_err, o.max_vel_err,
        o.sum_vel_err_sq);
  CHECK(o.max_ang_vel == 0.875 && o.max_force_z == 90.0, "%g %g", o.max_ang_vel, o.max_force_z);
  CHECK(o.not_ok_ticks == 2.0 && o.rejected_ticks == 1.0 && o.first_rejected_tick == 3.0, "%g %g %g", o.not_ok_ticks, o.rejected_ticks,
        o.first_rejected_tick);
  CHECK(o.iterations_sum == 127.0 && o.iterations_max == 120.0, "%g %g", o.iterations_sum, o.iterations_max);
  // tick 4 and 5: the record is frozen, whatever happens to the robot
  const qmpc_loop_outcome at_down = o;
  qmpc_loop::loop_outcome_one(op, state(4.0, 0.01, 0.25, {1, 0, 0, 0}, {9, 9, 9}, {0, 0}, {50, 50, 50}, {500.0, 5.0, 90.0, 5.0},
                                        QMPC_NAN_INPUT, 99), o);
  qmpc_loop::loop_outcome_one(op, state(5.0, kNan, 0.25, {0, kNan, 0, 0}, {9, 9, 9}, {0, 0}, {50, 50, 50}, {500.0, 5.0, 90.0, 5.0}, QMPC_OK, 1), o);
  CHECK(std::memcmp(&o, &at_down, sizeof o) == 0, "the record changed after its down tick");
  std::printf("sequence: 3 ticks accumulated, down at tick %g, frozen afterwards\n", o.down_tick);
}

void check_down_rule() {
  const qmpc_outcome_params op = default_op();
  auto one = [&](double z, const double (&q)[4]) {
    qmpc_loop_outcome o = empty_record();
    qmpc_loop::loop_outcome_one(op, state(17.0, z, 0.25, q, {0, 0, 0}, {0, 0}, {0, 0, 0}, {1.0, 2.0, 3.0, 4.0}, QMPC_OK, 5), o);
    return o;
  };
  qmpc_loop_outcome o = one(kNan, {1, 0, 0, 0});      // a NaN height: down, and no selection took it
  CHECK(o.down_tick == 17.0 && o.ticks == 1.0, "%g %g", o.down_tick, o.ticks);
  CHECK(o.min_height == kInf && o.max_height_err == -kInf && o.min_upright == 1.0, "%g %g %g", o.min_height, o.max_height_err, o.min_upright);
  CHECK(o.max_force_z == 4.0 && o.iterations_sum == 5.0 && o.max_vel_err == 0.0, "%g %g %g", o.max_force_z, o.iterations_sum, o.max_vel_err);
  o = one(kInf, {1, 0, 0, 0});                          // an infinite height is not a height either
  CHECK(o.down_tick == 17.0, "%g", o.down_tick);
  o = one(0.3, {0.5, kNan, 0, 0});                      // a NaN attitude: the upright value is NaN
  CHECK(o.down_tick == 17.0 && o.min_upright == kInf && o.min_height == 0.3, "%g %g %g", o.down_tick, o.min_upright, o.min_height);
  CHECK(o.max_vel_err == -kInf && o.sum_vel_err_sq != o.sum_vel_err_sq, "%g %g", o.max_vel_err, o.sum_vel_err_sq);   // the sum is a sum
  o = one(std::nextafter(0.15, 0.0), {1, 0, 0, 0});     // just below the height threshold
  CHECK(o.down_tick == 17.0, "%g", o.down_tick);
  o = one(0.15, {1, 0, 0, 0});                          // at the threshold: not below
  CHECK(o.down_tick == -1.0, "%g", o.down_tick);
  o = one(0.3, {0.0, 1.0, 0.0, 0.0});                   // upside down: upright = 1 - 2 = -1
  CHECK(o.down_tick == 17.0 && o.min_upright == -1.0, "%g %g", o.down_tick, o.min_upright);
  qmpc_outcome_params lax = op;                         // the thresholds are the caller's
  lax.down_height = 0.05; lax.down_upright = -2.0;
  o = empty_record();
  qmpc_loop::loop_outcome_one(lax, state(17.0, 0.1, 0.25, {0.0, 1.0, 0.0, 0.0}, {0, 0, 0}, {0, 0}, {0, 0, 0}, {1.0, 2.0, 3.0, 4.0}, QMPC_OK, 5), o);
  CHECK(o.down_tick == -1.0, "%g", o.down_tick);
  std::printf("down rule: 8 cases\n");
}

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

void check_segments() {
  const qmpc_outcome_params op = default_op();
  Rng r{5};
  int equal = 0, downs = 0;
  for (int rep = 0; rep < 200; ++rep) {
    qmpc_loop_state seq[60];
    for (int t = 0; t < 60; ++t) {
      double q[4] = {1.0, r.in(-0.35, 0.35), r.in(-0.35, 0.35), r.in(-1, 1)};
      const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
      for (double& c : q) c /= n;
      const double qq[4] = {q[0], q[1], q[2], q[3]};
      seq[t] = state(100.0 + t, r.in(0.145, 0.35), r.in(0.25, 0.32), qq, {r.in(-1, 1), r.in(-1, 1), r.in(-1, 1)}, {r.in(-0.5, 0.5), r.in(-0.5, 0.5)},
                     {r.in(-3, 3), r.in(-3, 3), r.in(-3, 3)}, {r.in(0, 150), r.in(0, 150), r.in(0, 150), r.in(0, 150)},
                     r.u() < 0.8 ? QMPC_OK : (r.u() < 0.5 ? QMPC_MAX_ITER : QMPC_NAN_INPUT), (int)r.in(3, 120));
    }
    qmpc_loop_outcome whole = empty_record(), parts = empty_record();
    for (int t = 0; t < 60; ++t) qmpc_loop::loop_outcome_one(op, seq[t], whole);
    const int cut = 1 + (int)r.in(0, 58);
    for (int t = 0; t < cut; ++t) qmpc_loop::loop_outcome_one(op, seq[t], parts);
    qmpc_loop_outcome carried;
    std::memcpy(&carried, &parts, sizeof carried);      // the record between two calls: 128 bytes, nothing else
    for (int t = cut; t < 60; ++t) qmpc_loop::loop_outcome_one(op, seq[t], carried);
    equal += std::memcmp(&whole, &carried, sizeof whole) == 0;
    downs += whole.down_tick >= 0.0;
    CHECK(whole.ticks == (whole.down_tick >= 0.0 ? whole.down_tick - 99.0 : 60.0), "%g %g", whole.ticks, whole.down_tick);
  }
  CHECK(equal == 200, "%d", equal);
  CHECK(downs > 20 && downs < 200, "%d", downs);      // both kinds of sequence occurred
  std::printf("segments: %d of 200 two-segment accumulations equal the one-segment record (%d sequences went down)\n", equal, downs);
}

}  // namespace

int main() {
  static_assert(sizeof(qmpc_loop_outcome) == 128 && sizeof(qmpc_outcome_params) == 32, "record sizes");
  check_sequence();
  check_down_rule();
  check_segments();
  std::printf("passed: %d failures\n", failures);
  return failures ? 1 : 0;
}
