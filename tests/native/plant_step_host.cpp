// Host-only access to the closed loop's plant and the attitude helpers of csrc/qmpc_loop_math.h, one call per input row, for
// tests/test_plant_reference_cpu.py (built like loop_instances_host.cpp: hipcc -x hip --offload-host-only; no device code, no
// device needed).  The test compares what comes out with tests/plant_reference.py, a longdouble statement of the model.
//
// stdin: one row per call, an operation name followed by doubles in C hex notation (%a); stdout: one row of hex doubles per
// input row.  Operations (counts of doubles in brackets):
//   step   mass inertia[9] dt x[13] u[12] feet[12]                   -> x[13]   inv3, then plant_step
//   stepx  mass inertia[9] dt x[13] u[12] feet[12] f_ext[3] t_ext[3] -> x[13]   inv3, then plant_step_ext
//   rot    q[4]                                                      -> R[9]    quat_to_rot
//   euler  q[4]                                                      -> e[3]    quat_to_euler
//   rotz   R[9]                                                      -> Rz[9]   rot_to_rot_z
//   inv    A[9]                                                      -> B[9]    inv3
//   rotv   q[4] f[3]                                                 -> R f [3], R' f [3]: quat_to_rot, then the two 3x3
//                                                                       products as the post step writes them (sums of three
//                                                                       products, left to right, no contraction)
//   push   n t force[3] torque[3] (start ticks force[3] torque[3]) x n -> force[3] torque[3]   loop_push_wrench
// The inverse inertia of a step is taken by inv3 from the inertia, as the library derives a plant's from its record.
// Exit status 0 unless a row could not be read.
#include "../../quaternion-mpc_amd/csrc/qmpc_loop_math.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

namespace {

bool read(std::istringstream& in, double* v, int n) {
  std::string tok;
  for (int i = 0; i < n; ++i) {
    if (!(in >> tok)) return false;
    char* end = nullptr;
    v[i] = std::strtod(tok.c_str(), &end);
    if (end == tok.c_str() || *end) return false;
  }
  return true;
}

void write(const double* v, int n) {
  for (int i = 0; i < n; ++i) std::printf(i ? " %a" : "%a", v[i]);
  std::printf("\n");
}

}  // namespace

int main() {
  std::string line, op;
  long row = 0;
  while (std::getline(std::cin, line)) {
    ++row;
    std::istringstream in(line);
    if (!(in >> op)) continue;
    bool ok = true;
    if (op == "step" || op == "stepx") {
      double mass, I[9], dt, x[13], u[12], feet[12], f[3], t[3], Iinv[9];
      ok = read(in, &mass, 1) && read(in, I, 9) && read(in, &dt, 1) && read(in, x, 13) && read(in, u, 12) && read(in, feet, 12);
      if (ok && op == "stepx") ok = read(in, f, 3) && read(in, t, 3);
      if (ok) {
        qmpc_loop::inv3(I, Iinv);
        if (op == "step") qmpc_loop::plant_step(x, u, feet, 4, mass, Iinv, dt);
        else qmpc_loop::plant_step_ext(x, u, feet, 4, mass, Iinv, f, t, dt);
        write(x, 13);
      }
    } else if (op == "rot") {
      double q[4], R[9];
      if ((ok = read(in, q, 4))) { qmpc_loop::quat_to_rot(q, R); write(R, 9); }
    } else if (op == "euler") {
      double q[4], e[3];
      if ((ok = read(in, q, 4))) { qmpc_loop::quat_to_euler(q, e); write(e, 3); }
    } else if (op == "rotz") {
      double R[9], Rz[9];
      if ((ok = read(in, R, 9))) { qmpc_loop::rot_to_rot_z(R, Rz); write(Rz, 9); }
    } else if (op == "inv") {
      double A[9], B[9];
      if ((ok = read(in, A, 9))) { qmpc_loop::inv3(A, B); write(B, 9); }
    } else if (op == "rotv") {
      double q[4], f[3], R[9], y[6];
      if ((ok = read(in, q, 4) && read(in, f, 3))) {
        QMPC_NO_CONTRACT
        qmpc_loop::quat_to_rot(q, R);
        for (int r = 0; r < 3; ++r) {
          y[r] = R[3 * r] * f[0] + R[3 * r + 1] * f[1] + R[3 * r + 2] * f[2];
          y[3 + r] = R[r] * f[0] + R[3 + r] * f[1] + R[6 + r] * f[2];
        }
        write(y, 6);
      }
    } else if (op == "push") {
      double n, t, w[6];
      ok = read(in, &n, 1) && read(in, &t, 1) && read(in, w, 6) && n >= 0 && n <= 64;
      std::vector<qmpc_push_params> push(ok ? (size_t)n : 0);
      for (size_t k = 0; ok && k < push.size(); ++k) {
        double v[8];
        if ((ok = read(in, v, 8))) {
          push[k].start_tick = v[0];
          push[k].ticks = v[1];
          std::memcpy(push[k].force_world, v + 2, sizeof(double) * 3);
          std::memcpy(push[k].torque_body, v + 5, sizeof(double) * 3);
        }
      }
      if (ok) {
        qmpc_loop::loop_push_wrench(push.data(), (int)push.size(), t, w, w + 3);
        write(w, 6);
      }
    } else {
      ok = false;
    }
    if (!ok) {
      std::fprintf(stderr, "row %ld: cannot read '%s'\n", row, op.c_str());
      return 1;
    }
  }
  return 0;
}
