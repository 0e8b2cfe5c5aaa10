// Host-only checks of the true ground of the closed loop's plant (qmpc_loop_run_ground*), built like loop_push_host.cpp (hipcc -x hip
// --offload-host-only; no device code, no device needed): loop_ground_leg / loop_ground_clamp / loop_ground_valid /
// loop_ground_tally_one / loop_ground_to_body (qmpc_loop_math.h) and one plant_step_ext under the delivered forces.
//   (a) the clamp on hand-made legs: each rule alone and the three in order; fz exactly at fz_max and t exactly at mu fz do not
//       bind; an unchanged leg keeps its bytes, a -0.0 included; mu = 0 gives zero tangential components; after scaling
//       t' <= mu fz (1 + 4 ulp) with the direction preserved (random legs); +inf limits never bind; swing legs are ignored and
//       an all-+inf record looks at no leg (a negative fz stays)
//   (b) the validity rule: NaN in each field, mu < 0, fz_max <= 0; +inf, mu = 0 pass
//   (c) the tally: ticks, first tick, leg-tick pairs of both kinds, a leg with both verdicts counts in both
//   (d) one plant step of a body at rest in rotation under clamped legs: dv = dt (sum f_delivered / m + g) to 1e-12 relative, with
//       the unchanged legs handed on as their commanded body-frame bytes
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
const double kUlp = std::numeric_limits<double>::epsilon();      // 2^-52
using qmpc_loop::LOOP_GROUND_FRICTION;
using qmpc_loop::LOOP_GROUND_NORMAL;

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

qmpc_ground_params ground(double mu, double fz_max) { return qmpc_ground_params{{mu, mu, mu, mu}, {fz_max, fz_max, fz_max, fz_max}}; }

void check_clamp() {
  int cases = 0;
  {   // rule 1 alone: the ground does not pull
    double f[3] = {3.0, -4.0, -1e-9};
    const int v = qmpc_loop::loop_ground_leg(kInf, kInf, f);
    const double e[3] = {0.0, 0.0, 0.0};
    CHECK(v == LOOP_GROUND_NORMAL && same_bytes(f, e, 3), "fz < 0: %d %g %g %g", v, f[0], f[1], f[2]); ++cases;
  }
  {   // rule 2 alone
    double f[3] = {3.0, -4.0, 80.0};
    const int v = qmpc_loop::loop_ground_leg(kInf, 30.0, f);
    const double e[3] = {3.0, -4.0, 30.0};
    CHECK(v == LOOP_GROUND_NORMAL && same_bytes(f, e, 3), "fz > fz_max: %d %g %g %g", v, f[0], f[1], f[2]); ++cases;
  }
  {   // rule 3 alone: |f_xy| = 5 against 0.25 * 8 = 2 -> s = 0.4
    double f[3] = {3.0, -4.0, 8.0};
    const int v = qmpc_loop::loop_ground_leg(0.25, kInf, f);
    const double s = (0.25 * 8.0) / 5.0, e[3] = {3.0 * s, -4.0 * s, 8.0};
    CHECK(v == LOOP_GROUND_FRICTION && same_bytes(f, e, 3), "friction: %d %.17g %.17g %g", v, f[0], f[1], f[2]); ++cases;
  }
  {   // the order: the normal cut comes first and the cone is that of the cut force: 0.5 * 10 = 5 against |f_xy| = 10
    double f[3] = {6.0, 8.0, 100.0};
    const int v = qmpc_loop::loop_ground_leg(0.5, 10.0, f);
    const double s = (0.5 * 10.0) / 10.0, e[3] = {6.0 * s, 8.0 * s, 10.0};
    CHECK(v == (LOOP_GROUND_NORMAL | LOOP_GROUND_FRICTION) && same_bytes(f, e, 3), "order: %d %g %g %g", v, f[0], f[1], f[2]); ++cases;
    // (on the uncut force, 0.5 * 100 = 50 > 10, friction would not have bound)
    double g[3] = {6.0, 8.0, 100.0};
    CHECK(qmpc_loop::loop_ground_leg(0.5, kInf, g) == 0, "the case tells the two orders apart"); ++cases;
  }
  {   // a pulled leg is zeroed and then binds nothing else, whatever the limits
    double f[3] = {6.0, 8.0, -5.0};
    const int v = qmpc_loop::loop_ground_leg(0.0, 1.0, f);
    const double e[3] = {0.0, 0.0, 0.0};
    CHECK(v == LOOP_GROUND_NORMAL && same_bytes(f, e, 3), "pulled, mu = 0: %d", v); ++cases;
  }
  {   // exactly at the limits: nothing binds, every byte stays (3-4-5: t is exactly 5 = 0.5 * 10)
    double f[3] = {3.0, -4.0, 10.0};
    const double f0[3] = {3.0, -4.0, 10.0};
    CHECK(qmpc_loop::loop_ground_leg(0.5, 10.0, f) == 0 && same_bytes(f, f0, 3), "at both limits"); ++cases;
  }
  {   // the bytes of an unchanged leg, a -0.0 included; fz = 0 with t = 0 does not bind either (0 > 0 is false; mu = inf: NaN)
    double f[3] = {-0.0, 0.0, 20.0};
    const double f0[3] = {-0.0, 0.0, 20.0};
    CHECK(qmpc_loop::loop_ground_leg(0.6, 200.0, f) == 0 && same_bytes(f, f0, 3) && std::signbit(f[0]), "-0.0 lost"); ++cases;
    double z[3] = {-0.0, -0.0, -0.0};
    const double z0[3] = {-0.0, -0.0, -0.0};
    CHECK(qmpc_loop::loop_ground_leg(0.6, 200.0, z) == 0 && same_bytes(z, z0, 3), "a -0.0 force"); ++cases;
    CHECK(qmpc_loop::loop_ground_leg(kInf, kInf, z) == 0 && same_bytes(z, z0, 3), "a -0.0 force, no limits"); ++cases;
    double big[3] = {1e300, -1e300, 1e-300};      // t overflows to +inf: still not above +inf * fz
    const double big0[3] = {1e300, -1e300, 1e-300};
    CHECK(qmpc_loop::loop_ground_leg(kInf, kInf, big) == 0 && same_bytes(big, big0, 3), "+inf limits bound"); ++cases;
  }
  {   // mu = 0: zero tangential components (of either sign), fz kept
    double f[3] = {3.0, -4.0, 10.0};
    const int v = qmpc_loop::loop_ground_leg(0.0, kInf, f);
    CHECK(v == LOOP_GROUND_FRICTION && f[0] == 0.0 && f[1] == 0.0 && f[2] == 10.0, "ice: %g %g %g", f[0], f[1], f[2]); ++cases;
    double g[3] = {0.0, -0.0, 10.0};      // nothing to take away: not bound
    const double g0[3] = {0.0, -0.0, 10.0};
    CHECK(qmpc_loop::loop_ground_leg(0.0, kInf, g) == 0 && same_bytes(g, g0, 3), "ice under a vertical force"); ++cases;
  }
  {   // random legs whose friction binds: t' <= mu fz (1 + 4 ulp), the direction kept to 4 ulp
    Rng r{5};
    int n = 0;
    for (int rep = 0; rep < 2000; ++rep) {
      const double mu = r.in(0.01, 1.0), fz = r.in(1.0, 150.0);
      const double t0 = mu * fz * r.in(1.0, 20.0), a = r.in(-3.14159, 3.14159);
      double f[3] = {t0 * std::cos(a), t0 * std::sin(a), fz};
      const double c[3] = {f[0], f[1], f[2]};
      const int v = qmpc_loop::loop_ground_leg(mu, kInf, f);
      if (!v) continue;      // (a factor that rounded to 1)
      ++n;
      const double t1 = std::sqrt(f[0] * f[0] + f[1] * f[1]);
      CHECK(v == LOOP_GROUND_FRICTION && f[2] == c[2], "verdict %d", v);
      CHECK(t1 <= mu * fz * (1.0 + 4.0 * kUlp) && t1 >= mu * fz * (1.0 - 4.0 * kUlp), "t' = %.17g against %.17g", t1, mu * fz);
      // both components were multiplied by one s: the cross product of (f, c) is zero to the roundings of two products
      const double cross = f[0] * c[1] - f[1] * c[0];
      CHECK(std::fabs(cross) <= 4.0 * kUlp * t1 * t0 && f[0] * c[0] + f[1] * c[1] > 0.0, "direction: cross %g", cross);
    }
    CHECK(n > 1900, "only %d legs bound", n);
    ++cases;
  }
  {   // the record: swing legs are not looked at, an all-+inf record looks at no leg
    const qmpc_ground_params g = ground(0.5, 10.0);
    double f[12] = {6.0, 8.0, 100.0, 6.0, 8.0, 100.0, 1.0, 0.0, 4.0, 1.0, 2.0, -3.0};
    const double f0[12] = {6.0, 8.0, 100.0, 6.0, 8.0, 100.0, 1.0, 0.0, 4.0, 1.0, 2.0, -3.0};
    const double con[4] = {1.0, 0.0, 1.0, 0.0};
    int v[4];
    const int any = qmpc_loop::loop_ground_clamp(g, con, f, v);
    CHECK(any == 3 && v[0] == 3 && v[1] == 0 && v[2] == 0 && v[3] == 0, "verdicts %d %d %d %d", v[0], v[1], v[2], v[3]); ++cases;
    CHECK(f[2] == 10.0 && same_bytes(f + 3, f0 + 3, 9), "a swing or an unbound leg changed"); ++cases;
    qmpc_ground_params none;
    for (int l = 0; l < 4; ++l) none.mu[l] = none.fz_max[l] = kInf;
    double h[12];
    std::memcpy(h, f0, sizeof h);
    const double all[4] = {1.0, 1.0, 1.0, 1.0};
    CHECK(!qmpc_loop::loop_ground_active(none) && qmpc_loop::loop_ground_clamp(none, all, h, v) == 0 && same_bytes(h, f0, 12),
          "an all-+inf record touched a leg"); ++cases;
    none.fz_max[2] = 1e4;      // one finite field: the record is active and leg 3's pull is cut, nothing else
    CHECK(qmpc_loop::loop_ground_active(none) && qmpc_loop::loop_ground_clamp(none, all, h, v) == LOOP_GROUND_NORMAL && v[3] == LOOP_GROUND_NORMAL &&
              v[0] == 0 && v[1] == 0 && v[2] == 0 && h[9] == 0.0 && h[10] == 0.0 && h[11] == 0.0 && same_bytes(h, f0, 9),
          "one finite field"); ++cases;
  }
  std::printf("clamp: %d cases\n", cases);
}

void check_validity() {
  int bad = 0;
  CHECK(qmpc_loop::loop_ground_valid(ground(kInf, kInf)) && qmpc_loop::loop_ground_valid(ground(0.0, 1e-300)) &&
            qmpc_loop::loop_ground_valid(ground(0.7, kInf)) && qmpc_loop::loop_ground_valid(ground(kInf, 55.0)), "valid records");
  for (int field = 0; field < 8; ++field) {
    const double vals_mu[] = {kNan, -1e-300, -1.0, -kInf}, vals_fz[] = {kNan, 0.0, -0.0, -5.0, -kInf};
    const double* vals = field < 4 ? vals_mu : vals_fz;
    const int nv = field < 4 ? 4 : 5;
    for (int k = 0; k < nv; ++k) {
      qmpc_ground_params g = ground(0.6, 200.0);
      reinterpret_cast<double*>(&g)[field] = vals[k];
      CHECK(!qmpc_loop::loop_ground_valid(g), "field %d = %g", field, vals[k]);
      ++bad;
    }
  }
  std::printf("validity: %d invalid records rejected\n", bad);
}

void check_tally() {
  qmpc_ground_tally t = {0.0, -1.0, 0.0, 0.0};
  const qmpc_ground_tally t0 = t;
  const int none[4] = {0, 0, 0, 0};
  qmpc_loop::loop_ground_tally_one(none, 4.0, t);
  CHECK(std::memcmp(&t, &t0, sizeof t) == 0, "a tick without a verdict changed the tally");
  const int a[4] = {LOOP_GROUND_NORMAL, 0, LOOP_GROUND_FRICTION, LOOP_GROUND_NORMAL | LOOP_GROUND_FRICTION};
  qmpc_loop::loop_ground_tally_one(a, 7.0, t);
  CHECK(t.clipped_ticks == 1.0 && t.first_clipped_tick == 7.0 && t.friction_leg_ticks == 2.0 && t.normal_leg_ticks == 2.0, "first tick");
  const int b[4] = {0, LOOP_GROUND_FRICTION, 0, 0};
  qmpc_loop::loop_ground_tally_one(b, 9.0, t);
  qmpc_loop::loop_ground_tally_one(none, 10.0, t);
  CHECK(t.clipped_ticks == 2.0 && t.first_clipped_tick == 7.0 && t.friction_leg_ticks == 3.0 && t.normal_leg_ticks == 2.0, "second tick");
  std::printf("tally: 4 ticks counted\n");
}

void check_momentum() {
  Rng r{11};
  const double dt = 0.005;
  int n = 0, clipped = 0;
  for (int rep = 0; rep < 200; ++rep) {
    double x[13], u[12], feet[12];
    double q[4] = {1.0, r.in(-0.1, 0.1), r.in(-0.1, 0.1), r.in(-1, 1)};
    const double qn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    x[0] = r.in(-0.4, 0.4); x[1] = r.in(-0.4, 0.4); x[2] = r.in(0.25, 0.35);
    for (int a = 0; a < 4; ++a) x[3 + a] = q[a] / qn;
    // no body rate: the midpoint attitude is the attitude, so R(q_mid) R(q)' f is f to rounding
    for (int a = 0; a < 3; ++a) { x[7 + a] = r.in(-0.5, 0.5); x[10 + a] = 0.0; }
    double R[9];
    qmpc_loop::quat_to_rot(&x[3], R);
    double grf[12];
    for (int l = 0; l < 4; ++l) {
      feet[3 * l] = x[0] + (l < 2 ? 0.18 : -0.18); feet[3 * l + 1] = x[1] + (l % 2 ? -0.13 : 0.13); feet[3 * l + 2] = 0.0;
      u[3 * l] = r.in(-5, 5); u[3 * l + 1] = r.in(-5, 5); u[3 * l + 2] = r.in(20, 28);
      for (int a = 0; a < 3; ++a) grf[3 * l + a] = R[3 * a] * u[3 * l] + R[3 * a + 1] * u[3 * l + 1] + R[3 * a + 2] * u[3 * l + 2];
    }
    const double mass = r.in(10, 16);
    const double Iinv[9] = {r.in(8, 12), 0, 0, 0, r.in(3, 5), 0, 0, 0, r.in(3, 5)};
    const double zero[3] = {0.0, 0.0, 0.0};
    // legs 0 and 1 stand on a ground that binds (fz_max 5 .. 10 N, mu 0.05), leg 2 on one that does not, leg 3 swings
    qmpc_ground_params g = ground(0.05, r.in(5.0, 10.0));
    g.mu[2] = 10.0; g.fz_max[2] = 1e4;
    const double con[4] = {1.0, 1.0, 1.0, 0.0};
    int v[4];
    qmpc_loop::loop_ground_clamp(g, con, grf, v);
    CHECK(v[0] != 0 && v[1] != 0 && v[2] == 0 && v[3] == 0, "verdicts %d %d %d %d", v[0], v[1], v[2], v[3]);
    double del[12];
    for (int l = 0; l < 4; ++l) {
      if (v[l]) { qmpc_loop::loop_ground_to_body(R, grf + 3 * l, del + 3 * l); ++clipped; }
      else std::memcpy(del + 3 * l, u + 3 * l, 3 * sizeof(double));
    }
    double y[13];
    std::memcpy(y, x, sizeof y);
    qmpc_loop::plant_step_ext(y, del, feet, 4, mass, Iinv, zero, zero, dt);
    double dv[3], ev[3], scale = 0.0;
    for (int a = 0; a < 3; ++a) {
      dv[a] = y[7 + a] - x[7 + a];
      ev[a] = dt * ((grf[a] + grf[3 + a] + grf[6 + a] + grf[9 + a]) / mass + (a == 2 ? -9.81 : 0.0));
      scale = std::fmax(scale, std::fabs(ev[a]));
    }
    // Why 1e-12: |v| < 1 rounds to 1.1e-16 twice in the difference; R R' f carries a few ulp of |f| < 40 N, over m >= 10 kg and
    // times dt that is 1e-17.  The legs carry at most 10 + 10 + 31 + 31 N in world z (tilt below 17 degrees), under m g >= 98 N:
    // |dv_z| >= dt 1.6 = 8e-3, so the scale -- the largest expected component -- stays above 1e-3 (checked).
    CHECK(scale > 1e-3, "scale %g", scale);
    for (int a = 0; a < 3; ++a) CHECK(std::fabs(dv[a] - ev[a]) <= 1e-12 * scale, "dv[%d] %.17g against %.17g", a, dv[a], ev[a]);
    ++n;
  }
  std::printf("momentum identity: %d random steps, %d clamped legs\n", n, clipped);
}

}  // namespace

int main() {
  static_assert(sizeof(qmpc_ground_params) == 64 && sizeof(qmpc_ground_tally) == 32, "record sizes");
  check_clamp();
  check_validity();
  check_tally();
  check_momentum();
  std::printf("passed: %d failures\n", failures);
  return failures ? 1 : 0;
}
