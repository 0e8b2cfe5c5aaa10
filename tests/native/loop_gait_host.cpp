// Host-only checks of a robot's own gait in the closed loop (qmpc_loop_run_gaits*), built like loop_sensing_host.cpp
// (hipcc -x hip --offload-host-only; no device code, no device needed): loop_gait_* of qmpc_loop_math.h, the one source of the
// rule, and the host classes that use it (host/LeggedContactFSMHip.h, host/SwingTrajectoryHip.h).
//   (a) validity: the six named gaits are valid at 5 ms up to 12.5 Hz; pronk, a gait with a flight phase, a non-dyadic split, a
//       split of 1/16, a frequency above 1 / (16 dt), a non-zero reserved word, non-finite fields and a first_stance of 2 are not
//   (b) identity: the trot at the call's frequency and nothing else
//   (c) the reset rule with phase0 on both sides of split, both patterns
//   (d) the GENERAL path on the trot record against the FIXED path, 400 ticks on scripted feet with early contacts: the legs
//       qmpc_loop::loop_gait_update advances equal, byte for byte after every tick, those of LeggedContactFSMHip with its trot
//       table; and the per-leg Raibert targets equal raibert_foot_targets' on 2000 random feedbacks (the only place the general
//       path meets the trot: an identity record never reaches it in the library)
//   (e) the class after set_gait walks the legs of loop_gait_update for the other five gaits, byte for byte
// Prints one summary line per part; exit status 0 when nothing failed.
#include "../../quaternion-mpc_amd/csrc/qmpc_loop_math.h"
#include "../../quaternion-mpc_amd/host/LeggedContactFSMHip.h"
#include "../../quaternion-mpc_amd/host/LeggedStateLite.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

namespace {

using legged::LeggedStateLite;

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

struct Named { const char* name; double fs[4], split[4], phase0[4]; };
const Named kGaits[6] = {{"trot", {1, 0, 0, 1}, {.5, .5, .5, .5}, {0, 0, 0, 0}},
                         {"pace", {1, 0, 1, 0}, {.5, .5, .5, .5}, {0, 0, 0, 0}},
                         {"bound", {1, 1, 0, 0}, {.5, .5, .5, .5}, {0, 0, 0, 0}},
                         {"trot_overlap", {1, 0, 0, 1}, {.625, .375, .375, .625}, {0, .875, .875, 0}},
                         {"crawl", {0, 0, 0, 0}, {.25, .25, .25, .25}, {0, .75, .5, .25}},
                         {"amble", {0, 0, 0, 0}, {.375, .375, .375, .375}, {0, .5, .75, .25}}};

qmpc_gait_params record(const Named& n, double f) {
  qmpc_gait_params g;
  std::memset(&g, 0, sizeof g);
  g.gait_freq = f;
  for (int l = 0; l < 4; ++l) { g.first_stance[l] = n.fs[l]; g.split[l] = n.split[l]; g.phase0[l] = n.phase0[l]; }
  return g;
}

std::uint64_t rng_state = 0x243F6A8885A308D3ull;
double uniform() {      // splitmix64 -> [0, 1)
  std::uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (double)(z >> 11) * 0x1.0p-53;
}

qmpc_loop_leg export_leg(const legged::LeggedContactFSMHip& F) {
  qmpc_loop_leg L;
  std::memset(&L, 0, sizeof L);
  L.gait_phase = F.phase();
  L.state = (double)F.get_contact_state();
  L.pattern_index = F.pattern_index();
  L.prev_pattern_index = F.prev_pattern_index();
  L.start_time = F.state_start_time();
  L.end_time = F.state_end_time();
  L.not_first_call = F.first_call_done() ? 1.0 : 0.0;
  L.terrain_height = F.terrain_height;
  for (int a = 0; a < 3; ++a) {
    L.swing_start[a] = F.swing_start()[a];
    L.swing_end[a] = F.swing_end()[a];
    L.fsm_pos[a] = F.FSM_foot_pos_target_world[a];
    L.fsm_vel[a] = F.FSM_foot_vel_target_world[a];
    L.fsm_acc[a] = F.FSM_foot_acc_target_world[a];
  }
  return L;
}

// `ticks` ticks of the four legs on scripted feet: the rule on record legs against the class (with its trot table when
// `fixed`, after set_gait otherwise); returns the number of (tick, leg) pairs whose bytes differ
int walk(const qmpc_gait_params& g, bool fixed, int ticks, int* transitions, int* early) {
  legged::LeggedContactFSMHip fsm[4];
  qmpc_loop_leg leg[4];
  std::memset(leg, 0, sizeof leg);
  for (int l = 0; l < 4; ++l) {
    leg[l].state = 1.0;
    qmpc_loop::loop_gait_reset(g, l, leg[l]);
    fsm[l].reset_params(g.gait_freq, l);
    if (fixed) fsm[l].reset();
    else fsm[l].set_gait(g.first_stance[l], g.split[l], g.phase0[l]);
  }
  legged::QuinticCurveHip curve;
  auto swing = [&](float t, float T, const double* a, const double* b, double* out) { curve.get_foot_swing_target(t, T, a, b, out); };
  int bad = 0;
  for (int t = 0; t < ticks; ++t)
    for (int l = 0; l < 4; ++l) {
      const double cur[3] = {0.2 * l + 0.001 * t + 0.01 * uniform(), -0.1 * l + 0.02 * uniform(), 0.03 * uniform()};
      const double tgt[3] = {cur[0] + 0.1 * uniform(), cur[1] + 0.05 * (uniform() - 0.5), 0.0};
      const bool flag = uniform() < 0.3;      // early contacts: the percent > 0.9 branch is taken now and then
      const double before = leg[l].state;      // raw: the fraction of its slot the leg will have spent after this tick's add
      const double raw = (leg[l].gait_phase + g.gait_freq * 0.005 - leg[l].start_time) / (leg[l].end_time - leg[l].start_time);
      qmpc_loop::loop_gait_update(g, l, leg[l], 5.0 / 1000.0, cur, tgt, flag, swing);
      fsm[l].update(5.0 / 1000.0, g.gait_freq, cur, tgt, flag);
      if (leg[l].state != before) {
        ++*transitions;
        if (before == 0.0 && raw < 0.999) ++*early;
      }
      const qmpc_loop_leg want = export_leg(fsm[l]);
      qmpc_loop_leg got = leg[l];
      for (int a = 0; a < 3; ++a) got.swing_extend[a] = 0.0;      // (private to the class: not exported; it is only ever 0)
      if (std::memcmp(&want, &got, sizeof want) != 0) ++bad;
    }
  return bad;
}

}  // namespace

int main() {
  const double dt = 0.005;
  {   // (a)
    int valid = 0, invalid = 0;
    for (const Named& n : kGaits)
      for (double f : {0.5, 1.7, 2.0, 2.2, 3.0, 12.5}) {
        const bool ok = qmpc_loop::loop_gait_valid(record(n, f), dt);
        CHECK(ok, "%s at %g Hz", n.name, f);
        valid += ok;
      }
    std::vector<qmpc_gait_params> bad;
    const Named pronk = {"pronk", {1, 1, 1, 1}, {.5, .5, .5, .5}, {0, 0, 0, 0}};
    bad.push_back(record(pronk, 2.2));
    const Named gallop = {"flight", {1, 1, 1, 1}, {.25, .25, .25, .25}, {0, .75, .5, .375}};      // a gap after the last arc
    bad.push_back(record(gallop, 2.2));
    qmpc_gait_params g = record(kGaits[0], 2.2);
    g.split[2] = 0.3; bad.push_back(g);
    g = record(kGaits[0], 2.2); g.split[0] = 0.0625; bad.push_back(g);
    g = record(kGaits[0], 2.2); g.split[3] = 0.9375; bad.push_back(g);
    g = record(kGaits[0], 12.5 + 1e-9); bad.push_back(g);
    g = record(kGaits[0], 0.0); bad.push_back(g);
    g = record(kGaits[0], -2.2); bad.push_back(g);
    g = record(kGaits[0], kNan); bad.push_back(g);
    g = record(kGaits[0], kInf); bad.push_back(g);
    for (int c = 0; c < 3; ++c) { g = record(kGaits[4], 2.2); g.reserved[c] = 1e-300; bad.push_back(g); }
    g = record(kGaits[4], 2.2); g.reserved[1] = kNan; bad.push_back(g);
    g = record(kGaits[0], 2.2); g.first_stance[1] = 2.0; bad.push_back(g);
    g = record(kGaits[0], 2.2); g.first_stance[1] = kNan; bad.push_back(g);
    g = record(kGaits[0], 2.2); g.phase0[1] = 1.0; bad.push_back(g);
    g = record(kGaits[0], 2.2); g.phase0[1] = -0.125; bad.push_back(g);
    g = record(kGaits[0], 2.2); g.phase0[1] = 0.1; bad.push_back(g);
    g = record(kGaits[0], 2.2); g.phase0[1] = kNan; bad.push_back(g);
    g = record(kGaits[0], 2.2); g.split[1] = kNan; bad.push_back(g);
    g = record(kGaits[0], 2.2); g.split[1] = kInf; bad.push_back(g);
    for (size_t i = 0; i < bad.size(); ++i) {
      const bool ok = qmpc_loop::loop_gait_valid(bad[i], dt);
      CHECK(!ok, "invalid record %zu accepted", i);
      invalid += !ok;
    }
    CHECK(!qmpc_loop::loop_gait_valid(record(kGaits[0], 6.5), 0.01), "6.5 Hz at 10 ms");
    CHECK(qmpc_loop::loop_gait_valid(record(kGaits[0], 6.25), 0.01), "6.25 Hz at 10 ms");
    std::printf("validity: %d valid records accepted, %d invalid rejected\n", valid, invalid);
  }
  {   // (b)
    int others = 0;
    CHECK(qmpc_loop::loop_gait_identity(record(kGaits[0], 2.2), 2.2), "trot at 2.2");
    CHECK(!qmpc_loop::loop_gait_identity(record(kGaits[0], 2.2), 2.0), "trot at another frequency");
    for (int k = 1; k < 6; ++k) { const bool id = qmpc_loop::loop_gait_identity(record(kGaits[k], 2.2), 2.2); CHECK(!id, "%s", kGaits[k].name); others += !id; }
    qmpc_gait_params g = record(kGaits[0], 2.2);
    g.phase0[3] = 0.25;
    CHECK(!qmpc_loop::loop_gait_identity(g, 2.2), "a phase offset");
    std::printf("identity: the trot at the call's frequency, %d other gaits are not\n", others);
  }
  {   // (c)
    int n = 0;
    for (double fs : {0.0, 1.0})
      for (double split : {0.25, 0.5, 0.625})
        for (double ph : {0.0, 0.125, 0.25, 0.5, 0.625, 0.875}) {
          qmpc_gait_params g = record(kGaits[0], 2.2);
          g.first_stance[2] = fs; g.split[2] = split; g.phase0[2] = ph;
          qmpc_loop_leg L;
          std::memset(&L, 0, sizeof L);
          L.state = 0.0; L.not_first_call = 1.0;
          L.swing_end[0] = 1.5; L.swing_end[1] = -2.5; L.swing_end[2] = 0.5; L.fsm_vel[1] = 3.0;
          qmpc_loop::loop_gait_reset(g, 2, L);
          const int idx = ph < split ? 0 : 1;
          CHECK(L.gait_phase == ph && L.pattern_index == idx && L.prev_pattern_index == 1 - idx, "indices at %g / %g", ph, split);
          CHECK(L.start_time == (idx ? split : 0.0) && L.end_time == (idx ? 1.0 : split), "times at %g / %g", ph, split);
          CHECK(L.state == ((idx == 0) == (fs != 0.0) ? 1.0 : 0.0), "state at %g / %g", ph, split);
          CHECK(L.not_first_call == 0.0 && L.fsm_pos[0] == 1.5 && L.fsm_pos[1] == -2.5 && L.fsm_pos[2] == 0.5 && L.fsm_vel[1] == 0.0, "the rest of reset()");
          CHECK(L.start_time <= L.gait_phase && L.gait_phase < L.end_time, "the phase lies in its slot");
          ++n;
        }
    std::printf("reset: %d cases\n", n);
  }
  {   // (d)
    int transitions = 0, early = 0, bad = 0;
    for (double f : {1.7, 2.2, 3.0}) bad += walk(record(kGaits[0], f), true, 400, &transitions, &early);
    CHECK(bad == 0, "%d (tick, leg) pairs differ", bad);
    CHECK(transitions > 40 && early > 0, "%d transitions, %d early", transitions, early);
    std::printf("general against fixed: 3 x 400 ticks, %d transitions (%d early), %d legs differ\n", transitions, early, bad);
    int rb = 0;
    for (int k = 0; k < 2000; ++k) {
      LeggedStateLite a, b;
      const double f = 0.5 + 4.5 * uniform(), yaw = 6.0 * (uniform() - 0.5);
      const double c = std::cos(yaw), s = std::sin(yaw);
      const double Rz[9] = {c, -s, 0, s, c, 0, 0, 0, 1};
      for (LeggedStateLite* S : {&a, &b}) {
        S->param.gait_freq = f;
        for (int r = 0; r < 3; ++r)
          for (int q = 0; q < 3; ++q) { S->fbk.torso_rot_mat_z(r, q) = Rz[3 * r + q]; S->fbk.torso_rot_mat(r, q) = Rz[3 * r + q]; }
      }
      for (int r = 0; r < 3; ++r) {
        a.fbk.torso_pos_world[r] = b.fbk.torso_pos_world[r] = r == 2 ? 0.2 + 0.2 * uniform() : 4.0 * (uniform() - 0.5);
        a.fbk.torso_lin_vel_world[r] = b.fbk.torso_lin_vel_world[r] = 6.0 * (uniform() - 0.5);      // (large: both clamps are reached)
        a.ctrl.torso_lin_vel_d_rel[r] = b.ctrl.torso_lin_vel_d_rel[r] = r == 2 ? 0.0 : 6.0 * (uniform() - 0.5);
      }
      for (int l = 0; l < 4; ++l)
        for (int r = 0; r < 3; ++r) a.param.default_foot_pos_rel(r, l) = b.param.default_foot_pos_rel(r, l) = uniform() - 0.5;
      legged::raibert_foot_targets(a);
      legged::raibert_foot_targets_gait(b, record(kGaits[0], f));
      for (int l = 0; l < 4; ++l)
        for (int r = 0; r < 3; ++r) {
          const double x = a.ctrl.foot_pos_target_world(r, l), y = b.ctrl.foot_pos_target_world(r, l);
          if (std::memcmp(&x, &y, sizeof x) != 0) ++rb;
        }
    }
    CHECK(rb == 0, "%d Raibert targets differ", rb);
    std::printf("raibert: 2000 feedbacks, %d targets differ\n", rb);
  }
  {   // (e)
    int transitions = 0, early = 0, bad = 0;
    for (int k = 1; k < 6; ++k)
      for (double f : {1.7, 3.0}) bad += walk(record(kGaits[k], f), false, 400, &transitions, &early);
    CHECK(bad == 0, "%d (tick, leg) pairs differ", bad);
    std::printf("class after set_gait: 10 x 400 ticks, %d transitions, %d legs differ\n", transitions, bad);
  }
  std::printf("passed: %d failures\n", failures);
  return failures ? 1 : 0;
}
