// Host-only checks of the measured state of the closed loop (qmpc_loop_run_sensing*), built like loop_actuation_host.cpp
// (hipcc -x hip --offload-host-only; no device code, no device needed): loop_sense_sum / loop_sense_noise / loop_sense_one /
// loop_sense_identity / loop_sense_valid (qmpc_loop_math.h), the one source of the rule.
//   (a) the six known answers of include/qmpc.h's hash, computed independently of this repository
//   (b) the identity record returns the input's bytes, a -0.0 and a denormal included
//   (c) an inactive channel is copied as bytes while its neighbours change; a bias-only channel adds exactly its bias; a channel
//       with sigma adds bias + sigma * n with the n of its (seed, tick, channel)
//   (d) attitude: |q_m| = 1 within 2 ulp, and the angle from q to q_m is 2 atan(|phi| / 2) within 1e-15 rad for |phi| in
//       {1e-3, 0.1, 1}, about phi (long double arithmetic on the doubles the rule returned)
//   (e) moments of n over 20000 ticks x 12 channels at seed 7: |mean| < 0.01, |var - 1| < 0.01 overall, each channel's variance
//       in [0.97, 1.03], every |n| <= 3.4641, largest off-diagonal channel correlation < 0.03, lag-1 autocorrelation < 0.03
//   (f) validity of records
// Prints one summary line per part; exit status 0 when nothing failed.
#include "../../quaternion-mpc_amd/csrc/qmpc_loop_math.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

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

bool same_bytes(const double* a, const double* b, int n) { return std::memcmp(a, b, sizeof(double) * n) == 0; }

qmpc_sense_params identity() {
  qmpc_sense_params p;
  std::memset(&p, 0, sizeof p);
  return p;
}

// a state away from every special value: position, a unit quaternion, velocity, body rate
void a_state(double* x, double yaw, double roll) {
  const double s[13] = {0.31, -1.7, 0.29, 0.0, 0.0, 0.0, 0.0, 0.4, -0.05, 0.02, 0.3, -0.2, 0.7};
  for (int a = 0; a < 13; ++a) x[a] = s[a];
  const double cy = std::cos(yaw / 2), sy = std::sin(yaw / 2), cr = std::cos(roll / 2), sr = std::sin(roll / 2);
  const double q[4] = {cy * cr, cy * sr, sy * sr, sy * cr};      // yaw about z after roll about x
  const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int a = 0; a < 4; ++a) x[3 + a] = q[a] / n;
}

void check_known_answers() {
  const struct { unsigned long long seed, tick; int c; unsigned S; } k[6] = {
      {0ull, 0ull, 0, 185125u},          {1ull, 0ull, 0, 107705u},           {1ull, 0ull, 11, 135190u}, {1ull, 1ull, 0, 126314u},
      {12345ull, 1000ull, 5, 107246u},   {9007199254740991ull, 2147483648ull, 11, 181815u}};
  int ok = 0;
  for (const auto& e : k) {
    const unsigned S = qmpc_loop::loop_sense_sum(e.seed, e.tick, e.c);
    CHECK(S == e.S, "S(%llu, %llu, %d) = %u, expected %u", e.seed, e.tick, e.c, S, e.S);
    const double n = qmpc_loop::loop_sense_noise(e.seed, e.tick, e.c);
    CHECK(n == ((double)e.S - 131070.0) * 2.6428997921303014e-05, "n of S = %u", e.S);
    ok += S == e.S;
  }
  CHECK(0x1.bb67ae86627e7p-16 == 2.6428997921303014e-05, "the scale's two spellings");
  CHECK(std::fabs(0x1.bb67ae86627e7p-16 * std::sqrt(4294967295.0 / 3.0) - 1.0) <= 2 * kUlp, "the scale is 1 / sqrt((2^32 - 1) / 3)");
  std::printf("hash: %d of 6 known answers\n", ok);
}

void check_identity() {
  qmpc_sense_params p = identity();
  p.seed = 99.0;      // ignored
  CHECK(qmpc_loop::loop_sense_identity(p), "identity");
  p.bias[4] = -0.0;
  CHECK(qmpc_loop::loop_sense_identity(p), "a -0.0 bias is zero");
  double x[13], m[13];
  a_state(x, 0.7, 0.1);
  x[1] = -0.0;
  x[8] = 4.9406564584124654e-324;      // the smallest denormal
  x[11] = -2.2250738585072014e-308 / 4;
  for (int a = 0; a < 13; ++a) m[a] = kNan;
  qmpc_loop::loop_sense_one(p, 17.0, x, m);
  CHECK(same_bytes(x, m, 13), "identity returns the input's bytes");
  for (int c = 0; c < 12; ++c) {
    qmpc_sense_params q = identity();
    q.bias[c] = 1e-300;
    CHECK(!qmpc_loop::loop_sense_identity(q), "bias[%d]", c);
    q = identity();
    q.sigma[c] = 1e-300;
    CHECK(!qmpc_loop::loop_sense_identity(q), "sigma[%d]", c);
  }
  if (!failures) std::printf("identity: the input's bytes, 24 single-field records are not the identity\n");
}

// the field of the 13 a non-attitude channel acts on
int field_of(int c) { return c < 3 ? c : c < 9 ? c + 1 : c + 1; }

void check_channels() {
  double x[13], m[13];
  a_state(x, -1.1, 0.2);
  x[0] = -0.0;
  int copies = 0, sums = 0;
  for (int c = 0; c < 12; ++c) {
    if (c >= 3 && c < 6) continue;
    // bias only on c: its field is x + bias exactly, every other field the input's bytes (the quaternion included)
    qmpc_sense_params p = identity();
    p.bias[c] = 0.0123 * (c + 1);
    p.seed = 5.0;
    qmpc_loop::loop_sense_one(p, 40.0, x, m);
    const int f = field_of(c);
    for (int a = 0; a < 13; ++a) {
      if (a == f) {
        CHECK(m[a] == x[a] + p.bias[c], "bias-only channel %d", c);
        ++sums;
      } else {
        CHECK(same_bytes(x + a, m + a, 1), "channel %d moved field %d", c, a);
        ++copies;
      }
    }
    // sigma on c and on its neighbours but one: the channel between them is copied as bytes while they change
    p = identity();
    const int lo = c < 3 ? 0 : c < 9 ? 6 : 9;
    for (int k = lo; k < lo + 3; ++k)
      if (k != c) { p.sigma[k] = 0.05; p.bias[k] = -0.01; }
    p.seed = 123456789.0;
    qmpc_loop::loop_sense_one(p, 1000.0, x, m);
    CHECK(same_bytes(x + f, m + f, 1), "inactive channel %d between active neighbours", c);
    for (int k = lo; k < lo + 3; ++k)
      if (k != c) {
        const double n = qmpc_loop::loop_sense_noise(123456789ull, 1000ull, k);
        CHECK(m[field_of(k)] == x[field_of(k)] + (p.bias[k] + p.sigma[k] * n) && m[field_of(k)] != x[field_of(k)], "active neighbour %d", k);
        ++sums;
      }
  }
  // one attitude channel: the other two enter as 0, every non-attitude field is copied
  qmpc_sense_params p = identity();
  p.bias[4] = 0.2;
  qmpc_loop::loop_sense_one(p, 0.0, x, m);
  CHECK(same_bytes(x, m, 3) && same_bytes(x + 7, m + 7, 6) && !same_bytes(x + 3, m + 3, 4), "attitude channel 4 alone");
  {
    const double w = x[3], qx = x[4], qy = x[5], qz = x[6], b = 0.1;
    const double q[4] = {w - qx * 0.0 - qy * b - qz * 0.0, w * 0.0 + qx + qy * 0.0 - qz * b, w * b - qx * 0.0 + qy + qz * 0.0,
                         w * 0.0 + qx * b - qy * 0.0 + qz};
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int a = 0; a < 4; ++a) CHECK(m[3 + a] == q[a] / n, "the product written out, component %d", a);
  }
  // the noise is a function of (seed, tick, channel) only
  p = identity();
  for (int c = 0; c < 12; ++c) p.sigma[c] = 0.01;
  p.seed = 77.0;
  double m2[13], m3[13];
  qmpc_loop::loop_sense_one(p, 9.0, x, m);
  qmpc_loop::loop_sense_one(p, 9.0, x, m2);
  qmpc_loop::loop_sense_one(p, 10.0, x, m3);
  CHECK(same_bytes(m, m2, 13), "reproducible");
  int moved = 0;
  for (int a = 0; a < 13; ++a) moved += m[a] != m3[a];
  CHECK(moved == 13, "another tick, another draw (%d of 13 fields)", moved);
  if (!failures) std::printf("channels: %d fields copied as bytes, %d sums exact, one attitude channel alone, reproducible\n", copies, sums);
}

void check_attitude() {
  const double mags[3] = {1e-3, 0.1, 1.0};
  const double dirs[5][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0.6, -0.48, 0.64}, {-0.36, 0.8, 0.48}};
  const double poses[4][2] = {{0.0, 0.0}, {0.7, 0.1}, {-2.9, -0.4}, {3.1, 1.2}};
  int n = 0;
  double worst_norm = 0.0;
  long double worst_angle = 0.0L;
  for (double mag : mags)
    for (const auto& d : dirs)
      for (const auto& pose : poses) {
        double x[13], m[13];
        a_state(x, pose[0], pose[1]);
        qmpc_sense_params p = identity();
        for (int a = 0; a < 3; ++a) p.bias[3 + a] = mag * d[a];
        qmpc_loop::loop_sense_one(p, 3.0, x, m);
        const double nn = std::sqrt(m[3] * m[3] + m[4] * m[4] + m[5] * m[5] + m[6] * m[6]);
        worst_norm = std::fmax(worst_norm, std::fabs(nn - 1.0));
        CHECK(std::fabs(nn - 1.0) <= 2 * kUlp, "|q_m| - 1 = %.3e", nn - 1.0);
        // r = conj(q) (x) q_m in long double: the rotation from q to q_m, expressed in the body frame
        const long double w = x[3], a = -x[4], b = -x[5], c = -x[6], W = m[3], A = m[4], B = m[5], C = m[6];
        const long double r[4] = {w * W - a * A - b * B - c * C, w * A + a * W + b * C - c * B, w * B - a * C + b * W + c * A,
                                  w * C + a * B - b * A + c * W};
        const long double v = sqrtl(r[1] * r[1] + r[2] * r[2] + r[3] * r[3]);
        const long double angle = 2.0L * atan2l(v, r[0]);
        const long double phi[3] = {(long double)p.bias[3], (long double)p.bias[4], (long double)p.bias[5]};
        const long double pn = sqrtl(phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]);
        const long double want = 2.0L * atanl(pn / 2.0L);
        worst_angle = fmaxl(worst_angle, fabsl(angle - want));
        CHECK(fabsl(angle - want) <= 1e-15L, "|phi| = %g: angle off by %.3Le", mag, angle - want);
        for (int k = 0; k < 3; ++k) CHECK(fabsl(r[1 + k] / v - phi[k] / pn) <= 1e-12L, "axis component %d at |phi| = %g", k, mag);
        ++n;
      }
  std::printf("attitude: %d rotations, | |q_m| - 1 | <= %.2f ulp, angle within %.2Le rad of 2 atan(|phi| / 2)\n", n, worst_norm / kUlp,
              worst_angle);
}

void check_moments() {
  const int T = 20000;
  std::vector<double> z((size_t)T * 12);
  double sum = 0.0, sq = 0.0, big = 0.0;
  for (int t = 0; t < T; ++t)
    for (int c = 0; c < 12; ++c) {
      const double n = qmpc_loop::loop_sense_noise(7ull, (unsigned long long)t, c);
      z[(size_t)t * 12 + c] = n;
      sum += n;
      sq += n * n;
      big = std::fmax(big, std::fabs(n));
    }
  const double N = (double)T * 12.0, mean = sum / N, var = sq / N - mean * mean;
  CHECK(std::fabs(mean) < 0.01, "mean %.5f", mean);
  CHECK(std::fabs(var - 1.0) < 0.01, "variance %.5f", var);
  CHECK(big <= 3.4641, "largest |n| %.6f", big);
  double mu[12], sd[12], vmin = 1e9, vmax = -1e9;
  for (int c = 0; c < 12; ++c) {
    double s = 0.0, s2 = 0.0;
    for (int t = 0; t < T; ++t) { s += z[(size_t)t * 12 + c]; s2 += z[(size_t)t * 12 + c] * z[(size_t)t * 12 + c]; }
    mu[c] = s / T;
    const double v = s2 / T - mu[c] * mu[c];
    sd[c] = std::sqrt(v);
    vmin = std::fmin(vmin, v);
    vmax = std::fmax(vmax, v);
    CHECK(v >= 0.97 && v <= 1.03, "variance of channel %d: %.5f", c, v);
  }
  double cross = 0.0, lag = 0.0;
  for (int a = 0; a < 12; ++a) {
    for (int b = a + 1; b < 12; ++b) {
      double s = 0.0;
      for (int t = 0; t < T; ++t) s += (z[(size_t)t * 12 + a] - mu[a]) * (z[(size_t)t * 12 + b] - mu[b]);
      cross = std::fmax(cross, std::fabs(s / T / (sd[a] * sd[b])));
    }
    double s = 0.0;
    for (int t = 0; t + 1 < T; ++t) s += (z[(size_t)t * 12 + a] - mu[a]) * (z[(size_t)(t + 1) * 12 + a] - mu[a]);
    lag = std::fmax(lag, std::fabs(s / (T - 1) / (sd[a] * sd[a])));
  }
  CHECK(cross < 0.03, "largest off-diagonal channel correlation %.5f", cross);
  CHECK(lag < 0.03, "largest lag-1 autocorrelation of a channel %.5f", lag);
  std::printf("moments: mean %.5f variance %.5f (channels %.4f .. %.4f) max |n| %.5f cross %.5f lag-1 %.5f\n", mean, var, vmin, vmax, big,
              cross, lag);
}

void check_validity() {
  int bad = 0, good = 0;
  auto invalid = [&](qmpc_sense_params p, const char* what) {
    CHECK(!qmpc_loop::loop_sense_valid(p), "accepted: %s", what);
    ++bad;
  };
  auto valid = [&](qmpc_sense_params p, const char* what) {
    CHECK(qmpc_loop::loop_sense_valid(p), "rejected: %s", what);
    ++good;
  };
  qmpc_sense_params p;
  for (double v : {kNan, kInf, -kInf}) {
    for (int c : {0, 5, 11}) {
      p = identity(); p.bias[c] = v; invalid(p, "non-finite bias");
      p = identity(); p.sigma[c] = v; invalid(p, "non-finite sigma");
    }
    p = identity(); p.seed = v; invalid(p, "non-finite seed");
    p = identity(); p.reserved[0] = v; invalid(p, "non-finite reserved");
    p = identity(); p.reserved[6] = v; invalid(p, "non-finite reserved");
  }
  for (int c : {0, 4, 11}) { p = identity(); p.sigma[c] = -1e-300; invalid(p, "negative sigma"); }
  for (double s : {-1.0, 0.5, 1.5, 9007199254740992.0, 1e300, -0.25}) { p = identity(); p.seed = s; invalid(p, "seed"); }
  valid(identity(), "identity");
  for (double s : {0.0, -0.0, 1.0, 4294967296.0, 9007199254740991.0}) { p = identity(); p.seed = s; valid(p, "seed"); }
  for (int c = 0; c < 12; ++c) { p = identity(); p.bias[c] = -3.0; p.sigma[c] = 2.0; valid(p, "bias and sigma"); }
  p = identity(); p.sigma[3] = -0.0; valid(p, "sigma -0.0");
  p = identity(); p.reserved[2] = 5.0; valid(p, "a finite reserved word");
  std::printf("validity: %d invalid records rejected, %d valid accepted\n", bad, good);
}

}  // namespace

int main() {
  check_known_answers();
  check_identity();
  check_channels();
  check_attitude();
  check_moments();
  check_validity();
  std::printf("%s: %d failures\n", failures ? "FAILED" : "passed", failures);
  return failures ? 1 : 0;
}
