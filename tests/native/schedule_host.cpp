// Host-only check of the gait predictor (qmpc_gait_predict: loop_gait_predict of qmpc_loop_math.h), a stand-alone program with
// its own main, built like loop_gait_host.cpp (hipcc -x hip --offload-host-only; no device code, no device needed) -- also the
// program to run under -fsanitize=address,undefined (add -Xarch_host -fsanitize=address,undefined to that line).
// For the six named gaits at 1.7 / 2.2 / 3.0 Hz, from 200 phases each (a state walked b ticks by loop_gait_update on flat feet,
// odd b with early contacts), N = 10, 20 and 32 at h = 5 ms: the masks equal, byte for byte, those of stepping a COPY of the
// state N - 1 more times with loop_gait_update itself (flag = false), knot 0 is the state's contacts, the state is unchanged, and
// the bytes on either side of the N the predictor may write stay as they were.
// Prints one summary line; exit status 0 when nothing failed.
#include "../../quaternion-mpc_amd/csrc/qmpc_loop_math.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

struct Named { const char* name; double fs[4], split[4], phase0[4]; };
const Named kGaits[6] = {{"trot", {1, 0, 0, 1}, {.5, .5, .5, .5}, {0, 0, 0, 0}},
                         {"pace", {1, 0, 1, 0}, {.5, .5, .5, .5}, {0, 0, 0, 0}},
                         {"bound", {1, 1, 0, 0}, {.5, .5, .5, .5}, {0, 0, 0, 0}},
                         {"trot_overlap", {1, 0, 0, 1}, {.625, .375, .375, .625}, {0, .875, .875, 0}},
                         {"crawl", {0, 0, 0, 0}, {.25, .25, .25, .25}, {0, .75, .5, .25}},
                         {"amble", {0, 0, 0, 0}, {.375, .375, .375, .375}, {0, .5, .75, .25}}};

// the swing quintic is not part of the schedule: a trajectory that stays where it starts
void no_swing(float, float, const double* a, const double*, double* out) {
  for (int i = 0; i < 9; ++i) out[i] = i < 3 ? a[i] : 0.0;
}

void walk(const qmpc_gait_params& g, qmpc_loop_state& s, double dt, bool early, unsigned& rng) {
  const double cur[3] = {0.1, 0.05, 0.0}, tgt[3] = {0.15, 0.05, 0.0};
  for (int l = 0; l < 4; ++l) {
    rng = rng * 1664525u + 1013904223u;
    const bool flag = early && (rng >> 24) < 77;
    s.gait_counter[l] = qmpc_loop::loop_gait_update(g, l, s.leg[l], dt, cur, tgt, flag, no_swing);
    s.contacts[l] = s.leg[l].state;
  }
}

}  // namespace

int main() {
  const double h = 5.0 / 1000.0, freqs[3] = {1.7, 2.2, 3.0};
  const int Ns[3] = {10, 20, 32};
  int failures = 0, cases = 0, switches = 0;
  unsigned rng = 12345u;
  for (const Named& n : kGaits)
    for (double f : freqs) {
      qmpc_gait_params g;
      std::memset(&g, 0, sizeof g);
      g.gait_freq = f;
      for (int l = 0; l < 4; ++l) { g.first_stance[l] = n.fs[l]; g.split[l] = n.split[l]; g.phase0[l] = n.phase0[l]; }
      if (!qmpc_loop::loop_gait_valid(g, h)) { std::printf("FAIL %s %.1f: record not valid\n", n.name, f); ++failures; continue; }
      for (int b = 0; b < 200; ++b) {
        qmpc_loop_state s;
        std::memset(&s, 0, sizeof s);
        for (int l = 0; l < 4; ++l) { qmpc_loop::loop_gait_reset(g, l, s.leg[l]); s.contacts[l] = s.leg[l].state; }
        for (int t = 0; t < b; ++t) walk(g, s, h, (b & 1) != 0, rng);
        for (int N : Ns) {
          qmpc_loop_state before = s;
          std::vector<unsigned char> got(N + 2, 0xAA);      // one guard byte on either side
          qmpc_loop::loop_gait_predict(g, s, h, N, got.data() + 1);
          qmpc_loop_state c = s;
          std::vector<unsigned char> want(N);
          for (int k = 0; k < N; ++k) {
            if (k) walk(g, c, h, false, rng);
            unsigned m = 0;
            for (int l = 0; l < 4; ++l) m |= c.contacts[l] != 0.0 ? 1u << l : 0u;
            want[k] = (unsigned char)m;
            if (k && want[k] != want[k - 1]) ++switches;
          }
          const bool same = std::memcmp(got.data() + 1, want.data(), N) == 0;
          const bool guards = got[0] == 0xAA && got[N + 1] == 0xAA;
          const bool untouched = std::memcmp(&before, &s, sizeof s) == 0;
          if (!same || !guards || !untouched) {
            if (failures < 20) std::printf("FAIL %s %.1f Hz phase %d N %d: masks %d guards %d state %d\n", n.name, f, b, N, same, guards, untouched);
            ++failures;
          }
          ++cases;
        }
      }
    }
  // N < 1 writes nothing
  unsigned char one = 0xAA;
  qmpc_loop_state s0;
  std::memset(&s0, 0, sizeof s0);
  qmpc_gait_params g0;
  std::memset(&g0, 0, sizeof g0);
  g0.gait_freq = 2.2;
  qmpc_loop::loop_gait_predict(g0, s0, h, 0, &one);
  if (one != 0xAA) { std::printf("FAIL N = 0 wrote a mask\n"); ++failures; }
  std::printf("predictor: %d cases, %d mask changes inside the horizons, %d differ\n", cases, switches, failures);
  std::printf("passed: %d failures\n", failures);
  return failures ? 1 : 0;
}
