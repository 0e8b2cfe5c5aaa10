// Host-only checks of the push windows of the closed loop (qmpc_loop_run_pushes*), built like loop_outcome_host.cpp (hipcc -x hip
// --offload-host-only; no device code, no device needed): loop_push_wrench and loop_push_valid (qmpc_loop_math.h) and one
// plant_step_ext under the effective wrench.
//   (a) the window rule at its edges: t = start - 1, start, start + ticks - 1, start + ticks; ticks <= 0; fractional values
//   (b) the combination rule: replace against add, a zero component leaves the bytes of a -0.0 running value alone, two
//       overlapping windows are summed in index order (against the same sum written out), an inactive window adds nothing
//   (c) the validity rule: each of the eight fields non-finite in turn
//   (d) the impulse identities of one plant step: the plant has no gyroscopic term and the midpoint attitude does not see the
//       wrench, so a pure force F leaves quaternion and body rate byte-identical to the unpushed step and gives dv = dt F / m,
//       dp = dt^2 F / (2 m); a pure torque leaves lin_vel_world byte-identical and gives dw = dt Iinv tau; all to 1e-12 relative
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

qmpc_push_params window(double start, double ticks, double fx, double fy, double fz, double tx, double ty, double tz) {
  return qmpc_push_params{start, ticks, {fx, fy, fz}, {tx, ty, tz}};
}

bool same_bytes(const double* a, const double* b, int n) { return std::memcmp(a, b, sizeof(double) * n) == 0; }

// does the window act at t?  (a force of 1 N in x on a zero running value: replaced when it acts)
bool acts(const qmpc_push_params& w, double t) {
  double f[3] = {0.0, 0.0, 0.0}, q[3] = {0.0, 0.0, 0.0};
  qmpc_loop::loop_push_wrench(&w, 1, t, f, q);
  return f[0] != 0.0;
}

void check_window_rule() {
  int cases = 0;
  const qmpc_push_params w = window(5.0, 3.0, 1.0, 0, 0, 0, 0, 0);      // acts in ticks 5, 6, 7
  CHECK(!acts(w, 4.0), "t = start - 1"); ++cases;
  CHECK(acts(w, 5.0), "t = start"); ++cases;
  CHECK(acts(w, 7.0), "t = start + ticks - 1"); ++cases;
  CHECK(!acts(w, 8.0), "t = start + ticks"); ++cases;
  CHECK(!acts(w, 0.0) && !acts(w, 1e9), "far away"); ++cases;
  for (double n : {0.0, -0.0, -1.0, -3.5}) {      // ticks <= 0: never
    const qmpc_push_params z = window(5.0, n, 1.0, 0, 0, 0, 0, 0);
    CHECK(!acts(z, 4.0) && !acts(z, 5.0) && !acts(z, 6.0) && !acts(z, 2.0), "ticks = %g", n); ++cases;
  }
  const qmpc_push_params neg = window(-4.0, 3.0, 1.0, 0, 0, 0, 0, 0);      // before tick 0: acts at no t >= 0
  CHECK(!acts(neg, 0.0) && acts(neg, -2.0), "a window before tick 0"); ++cases;
  const qmpc_push_params span = window(-4.0, 6.0, 1.0, 0, 0, 0, 0, 0);     // ... one that reaches into the run: ticks 0 and 1
  CHECK(acts(span, 0.0) && acts(span, 1.0) && !acts(span, 2.0), "a window straddling tick 0"); ++cases;
  // fractional values only shift where the comparisons flip: [4.5, 6.75) holds t = 5, 6
  const qmpc_push_params fr = window(4.5, 2.25, 1.0, 0, 0, 0, 0, 0);
  CHECK(!acts(fr, 4.0) && acts(fr, 5.0) && acts(fr, 6.0) && !acts(fr, 7.0), "fractional start and length"); ++cases;
  const qmpc_push_params half = window(5.0, 0.5, 1.0, 0, 0, 0, 0, 0);      // [5, 5.5) holds t = 5
  CHECK(!acts(half, 4.0) && acts(half, 5.0) && !acts(half, 6.0), "half a tick"); ++cases;
  const qmpc_push_params between = window(5.25, 0.5, 1.0, 0, 0, 0, 0, 0);  // [5.25, 5.75) holds no integer
  CHECK(!acts(between, 5.0) && !acts(between, 6.0), "between two ticks"); ++cases;
  std::printf("window rule: %d cases\n", cases);
}

void check_combination_rule() {
  int cases = 0;
  {   // replace: the running value is exactly zero (either sign) -> the window's bits
    const qmpc_push_params w = window(0.0, 1.0, 0.1, -0.0, -7.0, 0.3, 0.0, -0.0);
    double f[3] = {0.0, -0.0, -0.0}, q[3] = {-0.0, -0.0, 0.0};
    const double f0[3] = {0.0, -0.0, -0.0}, q0[3] = {-0.0, -0.0, 0.0};
    qmpc_loop::loop_push_wrench(&w, 1, 0.0, f, q);
    const double fe[3] = {0.1, -0.0, -7.0}, qe[3] = {0.3, -0.0, 0.0};      // zero components of the window: bytes left alone
    CHECK(same_bytes(f, fe, 3) && same_bytes(q, qe, 3), "replace: %g %g %g | %g %g %g", f[0], f[1], f[2], q[0], q[1], q[2]); ++cases;
    CHECK(std::signbit(f[1]) && std::signbit(q[1]) && !std::signbit(q[2]), "a zero component keeps the sign of a zero running value"); ++cases;
    double g[3] = {0.0, -0.0, -0.0}, r[3] = {-0.0, -0.0, 0.0};
    qmpc_loop::loop_push_wrench(&w, 1, 1.0, g, r);      // inactive: every byte as it came
    CHECK(same_bytes(g, f0, 3) && same_bytes(r, q0, 3), "an inactive window touched the wrench"); ++cases;
  }
  {   // add: one IEEE add onto a non-zero running value; 0.1 + 0.2 is not 0.3
    const qmpc_push_params w = window(2.0, 2.0, 0.2, 5.0, 0.0, -1.5, 0.0, 1e-300);
    double f[3] = {0.1, -5.0, 3.0}, q[3] = {1.5, 2.0, 1e300};
    qmpc_loop::loop_push_wrench(&w, 1, 3.0, f, q);
    const double fe[3] = {0.1 + 0.2, -5.0 + 5.0, 3.0}, qe[3] = {1.5 + -1.5, 2.0, 1e300 + 1e-300};
    CHECK(same_bytes(f, fe, 3) && same_bytes(q, qe, 3), "add: %.17g %g %g", f[0], f[1], f[2]); ++cases;
    CHECK(f[0] != 0.3 && f[1] == 0.0 && !std::signbit(f[1]), "the sum is the IEEE sum"); ++cases;
  }
  {   // two overlapping windows and one that does not act: summed in index order
    const qmpc_push_params w[3] = {window(0.0, 10.0, 0.2, 0.0, 1e16, 0.0, 0.7, 0.0), window(100.0, 5.0, 9.0, 9.0, 9.0, 9.0, 9.0, 9.0),
                                   window(3.0, 4.0, 0.3, 4.0, 1.0, 0.0, 0.1, -2.0)};
    double f[3] = {0.1, 0.0, -1e16}, q[3] = {0.0, 0.0, 0.25};
    qmpc_loop::loop_push_wrench(w, 3, 5.0, f, q);
    const double fe[3] = {(0.1 + 0.2) + 0.3, 4.0, (-1e16 + 1e16) == 0.0 ? 1.0 : 0.0}, qe[3] = {0.0, 0.7 + 0.1, 0.25 + -2.0};
    CHECK(same_bytes(f, fe, 3) && same_bytes(q, qe, 3), "index order: %.17g %g %g | %g %.17g %g", f[0], f[1], f[2], q[0], q[1], q[2]); ++cases;
    CHECK((0.1 + 0.2) + 0.3 != 0.1 + (0.2 + 0.3), "the case tells the two orders apart"); ++cases;
    double g[3] = {0.1, 0.0, -1e16}, r[3] = {0.0, 0.0, 0.25};
    qmpc_loop::loop_push_wrench(w, 3, 8.0, g, r);      // t = 8: only the first window is left
    const double ge[3] = {0.1 + 0.2, 0.0, 0.0}, re[3] = {0.0, 0.7, 0.25};
    CHECK(same_bytes(g, ge, 3) && same_bytes(r, re, 3), "after the overlap"); ++cases;
    double z[3] = {0.3, -0.0, -1e16}, y[3] = {-0.0, 0.0, 0.25};
    const double z0[3] = {0.3, -0.0, -1e16}, y0[3] = {-0.0, 0.0, 0.25};
    qmpc_loop::loop_push_wrench(w, 0, 5.0, z, y);      // no windows at all
    qmpc_loop::loop_push_wrench(w, 3, 50.0, z, y);     // none acts
    CHECK(same_bytes(z, z0, 3) && same_bytes(y, y0, 3), "nothing acts: bytes changed"); ++cases;
  }
  std::printf("combination rule: %d cases\n", cases);
}

void check_validity_rule() {
  int bad = 0;
  const qmpc_push_params ok = window(3.5, -2.0, 1e300, -0.0, 5.0, 0.0, -1e-300, 2.0);
  CHECK(qmpc_loop::loop_push_valid(ok), "a finite window");
  CHECK(qmpc_loop::loop_push_valid(window(0, 0, 0, 0, 0, 0, 0, 0)), "the zero window");
  for (int field = 0; field < 8; ++field)
    for (double v : {kNan, kInf, -kInf}) {
      qmpc_push_params w = ok;
      reinterpret_cast<double*>(&w)[field] = v;
      CHECK(!qmpc_loop::loop_push_valid(w), "field %d = %g", field, v);
      ++bad;
    }
  std::printf("validity rule: %d non-finite windows rejected\n", bad);
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

// relative to the largest component of the expected vector (a component may be arbitrarily close to zero)
bool close3(const double* a, const double* b, double tol) {
  const double scale = std::fmax(std::fabs(b[0]), std::fmax(std::fabs(b[1]), std::fabs(b[2])));
  for (int i = 0; i < 3; ++i)
    if (!(std::fabs(a[i] - b[i]) <= tol * scale)) return false;
  return true;
}

void check_impulse_identities() {
  Rng r{9};
  const double dt = 0.005;
  int n = 0;
  auto sgn = [&]() { return r.u() < 0.5 ? -1.0 : 1.0; };
  for (int rep = 0; rep < 200; ++rep) {
    double x[13], u[12], feet[12];
    double q[4] = {1.0, r.in(-0.3, 0.3), r.in(-0.3, 0.3), r.in(-1, 1)};
    const double qn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    x[0] = r.in(-0.4, 0.4); x[1] = r.in(-0.4, 0.4); x[2] = r.in(0.25, 0.35);
    for (int a = 0; a < 4; ++a) x[3 + a] = q[a] / qn;
    for (int a = 0; a < 3; ++a) { x[7 + a] = r.in(-0.5, 0.5); x[10 + a] = r.in(-1, 1); }
    for (int l = 0; l < 4; ++l) {
      feet[3 * l] = x[0] + (l < 2 ? 0.18 : -0.18) + r.in(-0.03, 0.03);
      feet[3 * l + 1] = x[1] + (l % 2 ? -0.13 : 0.13) + r.in(-0.03, 0.03);
      feet[3 * l + 2] = 0.0;
      u[3 * l] = r.in(-10, 10); u[3 * l + 1] = r.in(-10, 10); u[3 * l + 2] = r.in(0, 80);
    }
    const double mass = r.in(10, 16);
    const double Iinv[9] = {r.in(8, 12), r.in(-0.5, 0.5), r.in(-0.5, 0.5), r.in(-0.5, 0.5), r.in(3, 5),
                            r.in(-0.5, 0.5), r.in(-0.5, 0.5), r.in(-0.5, 0.5), r.in(3, 5)};
    const double zero[3] = {0.0, 0.0, 0.0};
    double base[13];
    std::memcpy(base, x, sizeof base);
    qmpc_loop::plant_step_ext(base, u, feet, 4, mass, Iinv, zero, zero, dt);
    {   // a pure force, through a window acting at this tick
      const qmpc_push_params w = window(7.0, 1.0, sgn() * r.in(100, 300), sgn() * r.in(100, 300), sgn() * r.in(100, 300), 0.0, 0.0, 0.0);
      double f[3] = {0.0, 0.0, 0.0}, tq[3] = {0.0, 0.0, 0.0};
      qmpc_loop::loop_push_wrench(&w, 1, 7.0, f, tq);
      double y[13];
      std::memcpy(y, x, sizeof y);
      qmpc_loop::plant_step_ext(y, u, feet, 4, mass, Iinv, f, tq, dt);
      CHECK(same_bytes(y + 3, base + 3, 4) && same_bytes(y + 10, base + 10, 3), "a force changed the attitude or the body rate");
      double dv[3], dp[3], ev[3], ep[3];
      for (int a = 0; a < 3; ++a) {
        dv[a] = y[7 + a] - base[7 + a]; dp[a] = y[a] - base[a];
        ev[a] = dt * w.force_world[a] / mass; ep[a] = 0.5 * dt * dt * w.force_world[a] / mass;
      }
      // Why 1e-12 is attainable here: both steps round p (|p| < 0.5: half an ulp is 2.8e-17) and v (|v| < 1: 5.6e-17) once
      // more than the exact difference, so the differences carry up to 6e-17 and 1.1e-16 of absolute error.  A force of at
      // least 100 N on at most 16 kg gives dp >= 7.8e-5 and dv >= 0.031: 8e-13 and 4e-15 relative.
      CHECK(close3(dv, ev, 1e-12), "dv %g %g %g against %g %g %g", dv[0], dv[1], dv[2], ev[0], ev[1], ev[2]);
      CHECK(close3(dp, ep, 1e-12), "dp %g %g %g against %g %g %g", dp[0], dp[1], dp[2], ep[0], ep[1], ep[2]);
    }
    {   // a pure torque
      const qmpc_push_params w = window(7.0, 1.0, 0.0, 0.0, 0.0, sgn() * r.in(10, 30), sgn() * r.in(10, 30), sgn() * r.in(10, 30));
      double f[3] = {0.0, 0.0, 0.0}, tq[3] = {0.0, 0.0, 0.0};
      qmpc_loop::loop_push_wrench(&w, 1, 7.0, f, tq);
      double y[13];
      std::memcpy(y, x, sizeof y);
      qmpc_loop::plant_step_ext(y, u, feet, 4, mass, Iinv, f, tq, dt);
      CHECK(same_bytes(y + 7, base + 7, 3), "a torque changed lin_vel_world");
      double dw[3], ew[3];
      for (int a = 0; a < 3; ++a) {
        dw[a] = y[10 + a] - base[10 + a];
        ew[a] = dt * (Iinv[3 * a] * w.torque_body[0] + Iinv[3 * a + 1] * w.torque_body[1] + Iinv[3 * a + 2] * w.torque_body[2]);
      }
      // (|w| < 1.1: 2.2e-16 of absolute error in the difference, the torque sum's rounding another 1e-16; the largest component
      // of dw is at least dt (8 * 10 - 2 * 0.5 * 30) = 0.25)
      CHECK(close3(dw, ew, 1e-12), "dw %g %g %g against %g %g %g", dw[0], dw[1], dw[2], ew[0], ew[1], ew[2]);
    }
    ++n;
  }
  std::printf("impulse identities: %d random steps, force and torque\n", n);
}

}  // namespace

int main() {
  static_assert(sizeof(qmpc_push_params) == 64 && QMPC_MAX_PUSHES == 8, "record size");
  check_window_rule();
  check_combination_rule();
  check_validity_rule();
  check_impulse_identities();
  std::printf("passed: %d failures\n", failures);
  return failures ? 1 : 0;
}
