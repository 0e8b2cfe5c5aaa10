// Host-only checks of the delay line and actuator lag of the closed loop (qmpc_loop_run_actuation*), built like loop_ground_host.cpp
// (hipcc -x hip --offload-host-only; no device code, no device needed): loop_actuation_one / loop_actuation_identity /
// loop_actuation_valid (qmpc_loop_math.h), on a line initialised as qmpc_actuation_line_init does.
//   (a) the identity record returns the command's bytes, a -0.0 and a denormal included, and keeps the line current
//   (b) delay d = 1 .. 8: over 30 pushes the output of push n is command n - d exactly (the ring wraps three times), and before d
//       commands exist the initial force comes out
//   (c) the lag on a constant target y from applied = 0: a_k = y (1 - (1 - alpha)^k) to 4 ulp of y over 40 steps for alpha in
//       {0.1, 0.5, 0.9} (the recurrence a' = a + alpha (y - a) rounds three times per step, each by at most half an ulp of y,
//       and the error of a step is damped by 1 - alpha in the next); one step against the three operations written out; alpha = 1
//       adds no rounding (bytes of y, whatever applied holds)
//   (d) a swing leg gives +0.0 and resets applied; the next stance tick starts from zero
//   (e) validity of records and of count
// Prints one summary line per part; exit status 0 when nothing failed.
#include "../../quaternion-mpc_amd/csrc/qmpc_loop_math.h"

#include <cmath>
#include <cstddef>
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
const double kUlp = std::numeric_limits<double>::epsilon();      // 2^-52
const double kStance[4] = {1.0, 1.0, 1.0, 1.0};

bool same_bytes(const double* a, const double* b, int n) { return std::memcmp(a, b, sizeof(double) * n) == 0; }

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

// qmpc_actuation_line_init for one robot
qmpc_actuation_line line_init(const double* f) {
  qmpc_actuation_line line;
  std::memset(&line, 0, sizeof line);
  for (int k = 0; k < 12; ++k) {
    for (int c = 0; c < QMPC_MAX_DELAY; ++c) line.cmd[c][k] = f ? f[k] : 0.0;
    line.applied[k] = f ? f[k] : 0.0;
  }
  return line;
}
qmpc_actuation_params record(double d, double alpha) { return qmpc_actuation_params{d, alpha, {0.0, 0.0}}; }

void command(Rng& r, double* c) {
  for (int k = 0; k < 12; ++k) c[k] = r.in(-60.0, 120.0);
}

void check_identity() {
  Rng r{11};
  const qmpc_actuation_params p = record(0.0, 1.0);
  CHECK(qmpc_loop::loop_actuation_identity(p), "identity record");
  CHECK(!qmpc_loop::loop_actuation_identity(record(1.0, 1.0)) && !qmpc_loop::loop_actuation_identity(record(0.0, 0.5)), "not identity");
  double init[12];
  command(r, init);
  qmpc_actuation_line line = line_init(init);
  double cmds[20][12];
  for (int n = 0; n < 20; ++n) {
    command(r, cmds[n]);
    cmds[n][n % 12] = -0.0;
    cmds[n][(n + 5) % 12] = 4.9406564584124654e-324;      // the smallest denormal
    double a[12];
    qmpc_loop::loop_actuation_one(p, line, cmds[n], kStance, a);
    CHECK(same_bytes(a, cmds[n], 12), "identity output, push %d", n);
    CHECK(same_bytes(line.applied, cmds[n], 12), "identity applied, push %d", n);
    CHECK(same_bytes(line.cmd[n % QMPC_MAX_DELAY], cmds[n], 12), "identity slot, push %d", n);
    CHECK(line.count == (double)(n + 1), "count after push %d: %g", n, line.count);
  }
  for (int n = 12; n < 20; ++n) CHECK(same_bytes(line.cmd[n % QMPC_MAX_DELAY], cmds[n], 12), "the ring holds the last 8 commands, %d", n);
  std::printf("identity: 20 pushes returned the command's bytes\n");
}

void check_delay() {
  int outputs = 0;
  for (int d = 1; d <= QMPC_MAX_DELAY; ++d) {
    Rng r{100 + (uint64_t)d};
    const qmpc_actuation_params p = record((double)d, 1.0);
    double init[12];
    command(r, init);
    init[3] = -0.0;
    qmpc_actuation_line line = line_init(init);
    double cmds[30][12];
    for (int n = 0; n < 30; ++n) {
      command(r, cmds[n]);
      double a[12];
      qmpc_loop::loop_actuation_one(p, line, cmds[n], kStance, a);
      const double* want = n >= d ? cmds[n - d] : init;      // before d commands exist: the initial force
      CHECK(same_bytes(a, want, 12), "delay %d, push %d", d, n);
      CHECK(same_bytes(line.applied, want, 12), "delay %d, applied after push %d", d, n);
      CHECK(line.count == (double)(n + 1), "delay %d, count %g", d, line.count);
      ++outputs;
    }
    for (int n = 22; n < 30; ++n) CHECK(same_bytes(line.cmd[n % QMPC_MAX_DELAY], cmds[n], 12), "delay %d: slot of command %d", d, n);
  }
  std::printf("delay: %d outputs over d = 1 .. 8 equal command n - d\n", outputs);
}

void check_lag() {
  int steps = 0;
  const double alphas[3] = {0.1, 0.5, 0.9};
  for (int ai = 0; ai < 3; ++ai) {
    const double alpha = alphas[ai];
    Rng r{200 + (uint64_t)ai};
    double y[12];
    command(r, y);
    qmpc_actuation_line line = line_init(nullptr);
    const qmpc_actuation_params p = record(0.0, alpha);
    for (int k = 1; k <= 40; ++k) {
      double a[12];
      qmpc_loop::loop_actuation_one(p, line, y, kStance, a);
      for (int c = 0; c < 12; ++c) {
        const double want = y[c] * (1.0 - std::pow(1.0 - alpha, (double)k));
        CHECK(std::fabs(a[c] - want) <= 4.0 * kUlp * std::fabs(y[c]), "alpha %g step %d: %.17g vs %.17g", alpha, k, a[c], want);
      }
      CHECK(same_bytes(a, line.applied, 12), "applied is the output");
      ++steps;
    }
  }
  {   // the recurrence itself, one step: one subtract, one multiply, one add, in that order
    qmpc_actuation_line line = line_init(nullptr);
    for (int c = 0; c < 12; ++c) line.applied[c] = 10.0 + c;
    double y[12], a[12];
    for (int c = 0; c < 12; ++c) y[c] = 1.0 / (3.0 + c);
    qmpc_loop::loop_actuation_one(record(0.0, 0.3), line, y, kStance, a);
    for (int c = 0; c < 12; ++c) {
      const volatile double diff = y[c] - (10.0 + c);
      const volatile double prod = 0.3 * diff;
      const double want = (10.0 + c) + prod;
      CHECK(a[c] == want, "one step, component %d", c);
    }
  }
  {   // alpha = 1 adds no rounding, whatever applied holds, with and without a delay
    Rng r{300};
    for (int d = 0; d <= 2; ++d) {
      qmpc_actuation_line line = line_init(nullptr);
      for (int c = 0; c < 12; ++c) line.applied[c] = r.in(-1e9, 1e9);
      double y[3][12], a[12];
      for (int n = 0; n < 3; ++n) {
        command(r, y[n]);
        qmpc_loop::loop_actuation_one(record((double)d, 1.0), line, y[n], kStance, a);
        if (n >= d) CHECK(same_bytes(a, y[n - d], 12), "alpha = 1, delay %d, push %d", d, n);
      }
    }
  }
  std::printf("lag: %d steps on a constant target within 4 ulp of the closed form\n", steps);
}

void check_swing() {
  Rng r{400};
  const qmpc_actuation_params p = record(1.0, 0.5);
  double init[12];
  command(r, init);
  qmpc_actuation_line line = line_init(init);
  double c0[12], c1[12], c2[12], a[12];
  command(r, c0); command(r, c1); command(r, c2);
  const double trot[4] = {1.0, 0.0, 0.0, 1.0};
  qmpc_loop::loop_actuation_one(p, line, c0, trot, a);
  for (int l = 1; l <= 2; ++l)
    for (int k = 3 * l; k < 3 * l + 3; ++k) {
      CHECK(a[k] == 0.0 && !std::signbit(a[k]), "swing leg %d delivers +0.0", l);
      CHECK(line.applied[k] == 0.0 && !std::signbit(line.applied[k]), "swing leg %d: applied reset", l);
    }
  for (int k = 0; k < 3; ++k) CHECK(a[k] == init[k] + 0.5 * (init[k] - init[k]), "stance leg lags towards the initial force");
  CHECK(same_bytes(line.cmd[0], c0, 12), "the command of a swing leg still enters the ring");
  // the next tick all legs stand: legs 1 and 2 start from zero towards command 0
  qmpc_loop::loop_actuation_one(p, line, c1, kStance, a);
  for (int l = 1; l <= 2; ++l)
    for (int k = 3 * l; k < 3 * l + 3; ++k) {
      const volatile double diff = c0[k] - 0.0;
      const volatile double prod = 0.5 * diff;
      CHECK(a[k] == 0.0 + prod, "leg %d starts from rest at touchdown", l);
    }
  // a -0.0 in applied or a negative target never leaks into a swing leg
  for (int k = 0; k < 12; ++k) line.applied[k] = -0.0;
  for (int k = 0; k < 12; ++k) c2[k] = -5.0;
  const double none[4] = {0.0, 0.0, 0.0, 0.0};
  qmpc_loop::loop_actuation_one(record(0.0, 1.0), line, c2, none, a);
  for (int k = 0; k < 12; ++k) CHECK(a[k] == 0.0 && !std::signbit(a[k]) && !std::signbit(line.applied[k]), "all swing: +0.0");
  std::printf("swing: unloaded legs deliver +0.0 and restart from rest\n");
}

void check_valid() {
  int rejected = 0, accepted = 0;
  const qmpc_actuation_line fresh = line_init(nullptr);
  for (int d = 0; d <= QMPC_MAX_DELAY; ++d) {
    CHECK(qmpc_loop::loop_actuation_valid(record((double)d, 1.0), fresh), "delay %d is valid", d);
    ++accepted;
  }
  const double good_alpha[4] = {1.0, 0.5, 1e-300, 4.9406564584124654e-324};
  for (double al : good_alpha) { CHECK(qmpc_loop::loop_actuation_valid(record(2.0, al), fresh), "alpha %g is valid", al); ++accepted; }
  const double bad_delay[8] = {-1.0, 9.0, 0.5, 7.999999, kNan, kInf, -kInf, 1e300};
  for (double d : bad_delay) { CHECK(!qmpc_loop::loop_actuation_valid(record(d, 1.0), fresh), "delay %g is invalid", d); ++rejected; }
  const double bad_alpha[7] = {0.0, -0.0, -0.5, 1.0000000000000002, kNan, kInf, -kInf};
  for (double al : bad_alpha) { CHECK(!qmpc_loop::loop_actuation_valid(record(0.0, al), fresh), "alpha %g is invalid", al); ++rejected; }
  for (int k = 0; k < 2; ++k) {
    const double bad[3] = {kNan, kInf, -kInf};
    for (double v : bad) {
      qmpc_actuation_params p = record(0.0, 1.0);
      p.reserved[k] = v;
      CHECK(!qmpc_loop::loop_actuation_valid(p, fresh), "a non-finite reserved field is invalid");
      ++rejected;
    }
  }
  const double bad_count[7] = {-1.0, 0.5, 3.0000000000000004, kNan, kInf, -kInf, 9007199254740992.0};
  for (double n : bad_count) {
    qmpc_actuation_line line = fresh;
    line.count = n;
    CHECK(!qmpc_loop::loop_actuation_valid(record(0.0, 1.0), line), "count %g is invalid", n);
    ++rejected;
  }
  const double good_count[4] = {0.0, 7.0, 123456789.0, 9007199254740991.0};
  for (double n : good_count) {
    qmpc_actuation_line line = fresh;
    line.count = n;
    CHECK(qmpc_loop::loop_actuation_valid(record(3.0, 0.5), line), "count %g is valid", n);
    ++accepted;
  }
  {   // a line that carries on from a large count: the slots are those of count mod 8
    qmpc_actuation_line line = fresh;
    line.count = 1e9 + 5.0;      // 1000000005 mod 8 = 5
    double c[12], a[12];
    for (int k = 0; k < 12; ++k) c[k] = 1.0 + k;
    qmpc_loop::loop_actuation_one(record(2.0, 1.0), line, c, kStance, a);
    CHECK(same_bytes(line.cmd[5], c, 12) && line.count == 1e9 + 6.0, "push at a large count");
  }
  std::printf("validity: %d invalid records rejected, %d valid accepted\n", rejected, accepted);
}

}  // namespace

int main() {
  static_assert(sizeof(qmpc_actuation_params) == 32 && sizeof(qmpc_actuation_line) == 896, "struct sizes");
  static_assert(offsetof(qmpc_actuation_line, applied) == 768 && offsetof(qmpc_actuation_line, count) == 864, "line layout");
  check_identity();
  check_delay();
  check_lag();
  check_swing();
  check_valid();
  std::printf("passed: %d failures\n", failures);
  return failures ? 1 : 0;
}
