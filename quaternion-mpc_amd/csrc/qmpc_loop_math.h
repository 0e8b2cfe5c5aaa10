// qmpc_loop_math.h -- arithmetic shared by the device-resident closed loop (qmpc_loop.hip) and its host
// reference driver (host/ClosedLoopHost.h): attitude conversions and the single-rigid-body PLANT that closes the
// loop around the MPC.  The plant is this repository's (the reference closes its loop through Gazebo / the robot);
// everything on the controller side of it mirrors the reference (qmpc_loop.hip cites the lines).
#pragma once

#include <math.h>

#include "../../include/qmpc.h"      // the outcome record of loop_outcome_one

#if defined(__HIPCC__)
#define QMPC_HD __host__ __device__ inline
#else
#define QMPC_HD inline
#endif
// no fused multiply-adds on the device side either (g++ does not fuse on the host): both sides then differ only
// through their math libraries' atan2 / sin / cos
#if defined(__clang__)
#define QMPC_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define QMPC_NO_CONTRACT
#endif

namespace qmpc_loop {

// body -> world rotation of q = (w, x, y, z); row-major 3x3 (Eigen's Quaterniond::toRotationMatrix)
QMPC_HD void quat_to_rot(const double* q, double* R) {
  QMPC_NO_CONTRACT
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz;         R[2] = txz + twy;
  R[3] = txy + twz;         R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy;         R[7] = tyz + twx;         R[8] = 1.0 - (txx + tyy);
}

// roll, pitch, yaw of q = (w, x, y, z): Utils::quat_to_euler (legged_ctrl/src/utils/Utils.cpp:7-33), fbk.torso_euler
QMPC_HD void quat_to_euler(const double* q, double* e) {
  QMPC_NO_CONTRACT
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double yy = y * y;
  e[0] = atan2(2.0 * (w * x + y * z), 1.0 - 2.0 * (x * x + yy));
  double t2 = 2.0 * (w * y - z * x);
  t2 = t2 > 1.0 ? 1.0 : t2;
  t2 = t2 < -1.0 ? -1.0 : t2;
  e[1] = asin(t2);
  e[2] = atan2(2.0 * (w * z + x * y), 1.0 - 2.0 * (yy + z * z));
}

// yaw-only rotation next to the full one (fbk.torso_rot_mat_z beside fbk.torso_rot_mat)
QMPC_HD void rot_to_rot_z(const double* R, double* Rz) {
  const double yaw = atan2(R[3], R[0]);
  const double c = cos(yaw), s = sin(yaw);
  Rz[0] = c;   Rz[1] = -s;  Rz[2] = 0.0;
  Rz[3] = s;   Rz[4] = c;   Rz[5] = 0.0;
  Rz[6] = 0.0; Rz[7] = 0.0; Rz[8] = 1.0;
}

// Plant: one explicit-midpoint step of a free rigid body under the body-frame foot forces u (3 per leg; swing legs
// carry zero force), world-frame position / velocity, body-frame angular velocity, no gyroscopic term (as the
// controller's own model, AltroUtils.cpp:389-391), feet fixed in the world during the step:
//   p' = v,  v' = R(q) sum(u)/m + g,  q' = 1/2 G(q) w,  w' = Iinv sum(r_l x u_l),  r_l = R(q)'(foot_l - p)
// state x = [p(3) q(4) v(3) w(3)]; the quaternion is re-normalised after the step.
QMPC_HD void plant_rate(const double* x, const double* u, const double* feet_world, int nleg, double mass,
                        const double* Iinv, double* xd) {
  QMPC_NO_CONTRACT
  double R[9];
  quat_to_rot(&x[3], R);
  double F[3] = {0.0, 0.0, 0.0}, tau[3] = {0.0, 0.0, 0.0};
  for (int l = 0; l < nleg; ++l) {
    const double d[3] = {feet_world[3 * l] - x[0], feet_world[3 * l + 1] - x[1], feet_world[3 * l + 2] - x[2]};
    const double r[3] = {R[0] * d[0] + R[3] * d[1] + R[6] * d[2], R[1] * d[0] + R[4] * d[1] + R[7] * d[2],
                         R[2] * d[0] + R[5] * d[1] + R[8] * d[2]};
    const double* f = &u[3 * l];
    F[0] += f[0]; F[1] += f[1]; F[2] += f[2];
    tau[0] += r[1] * f[2] - r[2] * f[1];
    tau[1] += r[2] * f[0] - r[0] * f[2];
    tau[2] += r[0] * f[1] - r[1] * f[0];
  }
  xd[0] = x[7]; xd[1] = x[8]; xd[2] = x[9];
  const double s = x[3], qx = x[4], qy = x[5], qz = x[6], wx = x[10], wy = x[11], wz = x[12];
  xd[3] = 0.5 * (-qx * wx - qy * wy - qz * wz);        // 1/2 G(q) w, QuaternionUtils.cpp:30-52
  xd[4] = 0.5 * (s * wx - qz * wy + qy * wz);
  xd[5] = 0.5 * (qz * wx + s * wy - qx * wz);
  xd[6] = 0.5 * (-qy * wx + qx * wy + s * wz);
  for (int a = 0; a < 3; ++a) {
    xd[7 + a] = (R[3 * a] * F[0] + R[3 * a + 1] * F[1] + R[3 * a + 2] * F[2]) / mass;
    xd[10 + a] = Iinv[3 * a] * tau[0] + Iinv[3 * a + 1] * tau[1] + Iinv[3 * a + 2] * tau[2];
  }
  xd[9] += -9.81;
}

QMPC_HD void plant_step(double* x, const double* u, const double* feet_world, int nleg, double mass,
                        const double* Iinv, double dt) {
  QMPC_NO_CONTRACT
  double k1[13], xm[13], k2[13];
  plant_rate(x, u, feet_world, nleg, mass, Iinv, k1);
  for (int i = 0; i < 13; ++i) xm[i] = x[i] + 0.5 * dt * k1[i];
  plant_rate(xm, u, feet_world, nleg, mass, Iinv, k2);
  for (int i = 0; i < 13; ++i) x[i] = x[i] + dt * k2[i];
  const double n = sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5] + x[6] * x[6]);
  for (int i = 3; i < 7; ++i) x[i] = x[i] / n;
}

// The same plant under a constant disturbance wrench as well (the closed loop with per-robot plants,
// qmpc_loop_run_instances*): f_ext in the world frame at the CoM, tau_ext in the body frame,
//   v' = (R(q) sum(u) + f_ext)/m + g,  w' = Iinv (sum(r_l x u_l) + tau_ext).
// A component that is exactly zero adds nothing -- not even `+ 0.0`, which would turn a -0.0 into +0.0 -- so a zero
// disturbance gives the bits of plant_step.  plant_rate / plant_step are left as they are (their callers' code is
// unchanged); this is their text with the two additions.
QMPC_HD void plant_rate_ext(const double* x, const double* u, const double* feet_world, int nleg, double mass,
                            const double* Iinv, const double* f_ext, const double* tau_ext, double* xd) {
  QMPC_NO_CONTRACT
  double R[9];
  quat_to_rot(&x[3], R);
  double F[3] = {0.0, 0.0, 0.0}, tau[3] = {0.0, 0.0, 0.0};
  for (int l = 0; l < nleg; ++l) {
    const double d[3] = {feet_world[3 * l] - x[0], feet_world[3 * l + 1] - x[1], feet_world[3 * l + 2] - x[2]};
    const double r[3] = {R[0] * d[0] + R[3] * d[1] + R[6] * d[2], R[1] * d[0] + R[4] * d[1] + R[7] * d[2],
                         R[2] * d[0] + R[5] * d[1] + R[8] * d[2]};
    const double* f = &u[3 * l];
    F[0] += f[0]; F[1] += f[1]; F[2] += f[2];
    tau[0] += r[1] * f[2] - r[2] * f[1];
    tau[1] += r[2] * f[0] - r[0] * f[2];
    tau[2] += r[0] * f[1] - r[1] * f[0];
  }
  for (int a = 0; a < 3; ++a)
    if (tau_ext[a] != 0.0) tau[a] += tau_ext[a];
  xd[0] = x[7]; xd[1] = x[8]; xd[2] = x[9];
  const double s = x[3], qx = x[4], qy = x[5], qz = x[6], wx = x[10], wy = x[11], wz = x[12];
  xd[3] = 0.5 * (-qx * wx - qy * wy - qz * wz);
  xd[4] = 0.5 * (s * wx - qz * wy + qy * wz);
  xd[5] = 0.5 * (qz * wx + s * wy - qx * wz);
  xd[6] = 0.5 * (-qy * wx + qx * wy + s * wz);
  for (int a = 0; a < 3; ++a) {
    double fw = R[3 * a] * F[0] + R[3 * a + 1] * F[1] + R[3 * a + 2] * F[2];
    if (f_ext[a] != 0.0) fw += f_ext[a];
    xd[7 + a] = fw / mass;
    xd[10 + a] = Iinv[3 * a] * tau[0] + Iinv[3 * a + 1] * tau[1] + Iinv[3 * a + 2] * tau[2];
  }
  xd[9] += -9.81;
}

QMPC_HD void plant_step_ext(double* x, const double* u, const double* feet_world, int nleg, double mass,
                            const double* Iinv, const double* f_ext, const double* tau_ext, double dt) {
  QMPC_NO_CONTRACT
  double k1[13], xm[13], k2[13];
  plant_rate_ext(x, u, feet_world, nleg, mass, Iinv, f_ext, tau_ext, k1);
  for (int i = 0; i < 13; ++i) xm[i] = x[i] + 0.5 * dt * k1[i];
  plant_rate_ext(xm, u, feet_world, nleg, mass, Iinv, f_ext, tau_ext, k2);
  for (int i = 0; i < 13; ++i) x[i] = x[i] + dt * k2[i];
  const double n = sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5] + x[6] * x[6]);
  for (int i = 3; i < 7; ++i) x[i] = x[i] / n;
}

// One tick of a robot's outcome record (qmpc_loop_run_outcomes*, include/qmpc.h): s is the robot's state AFTER the post step of
// the tick -- the new plant state, this tick's lin_vel_d_rel and joy, the applied forces_body, status and iterations.  A record
// whose down_tick is set is frozen.  Minima and maxima are selections by `<` / `>`: a non-finite value selects nothing (it
// makes the robot down instead).  The tick that leaves the robot down is accumulated, then down_tick = s.tick.
// One source for the device kernels (qmpc_loop_outcome.hip), the host class (host/ClosedLoopHost.h) and the native test.
QMPC_HD void loop_outcome_one(const qmpc_outcome_params& op, const qmpc_loop_state& s, qmpc_loop_outcome& o) {
  QMPC_NO_CONTRACT
  if (o.down_tick >= 0.0) return;
  double R[9];
  quat_to_rot(s.quat, R);
  const double height = s.pos_world[2], upright = R[8];
  o.ticks += 1.0;
  if (height < o.min_height) o.min_height = height;
  if (upright < o.min_upright) o.min_upright = upright;
  const double he = fabs(height - s.joy[2]);
  if (he > o.max_height_err) o.max_height_err = he;
  const double vx = R[0] * s.lin_vel_world[0] + R[3] * s.lin_vel_world[1] + R[6] * s.lin_vel_world[2];
  const double vy = R[1] * s.lin_vel_world[0] + R[4] * s.lin_vel_world[1] + R[7] * s.lin_vel_world[2];
  const double dx = vx - s.lin_vel_d_rel[0], dy = vy - s.lin_vel_d_rel[1];
  const double e2 = dx * dx + dy * dy;
  const double ev = sqrt(e2);
  if (ev > o.max_vel_err) o.max_vel_err = ev;
  o.sum_vel_err_sq += e2;
  for (int a = 0; a < 3; ++a) {
    const double w = fabs(s.ang_vel_body[a]);
    if (w > o.max_ang_vel) o.max_ang_vel = w;
  }
  for (int l = 0; l < 4; ++l)
    if (s.forces_body[3 * l + 2] > o.max_force_z) o.max_force_z = s.forces_body[3 * l + 2];
  if (s.status != (double)QMPC_OK) {
    o.not_ok_ticks += 1.0;
    if (s.status != (double)QMPC_MAX_ITER) {
      o.rejected_ticks += 1.0;
      if (o.first_rejected_tick < 0.0) o.first_rejected_tick = s.tick;
    }
  }
  o.iterations_sum += s.iterations;
  if (s.iterations > o.iterations_max) o.iterations_max = s.iterations;
  // down: either value non-finite (x - x is 0 only for a finite x) or below its threshold
  const bool finite = (height - height == 0.0) && (upright - upright == 0.0);
  if (!finite || height < op.down_height || upright < op.down_upright) o.down_tick = s.tick;
}

// The effective disturbance wrench of one tick under a robot's push windows (qmpc_loop_run_pushes*, include/qmpc.h): t is
// state.tick BEFORE the tick, force / torque come in as the plant's constant disturbance and go out as the wrench of this tick.
// Window k acts when t >= start_tick and t < start_tick + ticks (ticks <= 0: never).  Per component, in index order: an active
// window's value that is not exactly zero replaces a running value that is exactly zero (either sign: the bits become the
// window's) and is added to any other with one IEEE add; an inactive window or a zero component touches nothing -- the rule of
// plant_rate_ext, so windows that never act leave the bytes of force / torque alone.
// One source for the device kernels (qmpc_loop_push.hip), the host class (host/ClosedLoopHost.h) and the native test.
QMPC_HD void loop_push_wrench(const qmpc_push_params* push, int n, double t, double* force, double* torque) {
  QMPC_NO_CONTRACT
  for (int k = 0; k < n; ++k) {
    const qmpc_push_params& w = push[k];
    if (!(w.ticks > 0.0) || !(t >= w.start_tick) || !(t < w.start_tick + w.ticks)) continue;
    for (int a = 0; a < 3; ++a) {
      if (w.force_world[a] != 0.0) force[a] = force[a] == 0.0 ? w.force_world[a] : force[a] + w.force_world[a];
      if (w.torque_body[a] != 0.0) torque[a] = torque[a] == 0.0 ? w.torque_body[a] : torque[a] + w.torque_body[a];
    }
  }
}

// A push window is valid when its eight fields are finite (x - x is 0 only for a finite x); the robot of an invalid one is frozen
QMPC_HD bool loop_push_valid(const qmpc_push_params& w) {
  QMPC_NO_CONTRACT
  bool ok = (w.start_tick - w.start_tick == 0.0) && (w.ticks - w.ticks == 0.0);
  for (int a = 0; a < 3; ++a)
    ok = ok && (w.force_world[a] - w.force_world[a] == 0.0) && (w.torque_body[a] - w.torque_body[a] == 0.0);
  return ok;
}

// What the TRUE ground under one stance foot delivers of a commanded world-frame force f (qmpc_loop_run_ground*, include/qmpc.h),
// in this order: fz < 0 -> f = 0 (the ground does not pull); fz > fz_max -> fz = fz_max; t = |f_xy| > mu fz -> f_xy scaled by
// (mu fz) / t.  Returns the verdict: LOOP_GROUND_NORMAL and / or LOOP_GROUND_FRICTION, 0 for a leg no rule changed -- whose
// bytes are then untouched: no arithmetic reaches f, no `+ 0.0` (the rule of plant_rate_ext and loop_push_wrench).  A +inf
// limit never binds (mu = +inf with fz = 0 compares against NaN: false).  mu = 0 leaves zeros of either sign in f_xy.
enum { LOOP_GROUND_NORMAL = 1, LOOP_GROUND_FRICTION = 2 };
QMPC_HD int loop_ground_leg(double mu, double fz_max, double* f) {
  QMPC_NO_CONTRACT
  int v = 0;
  if (f[2] < 0.0) {
    f[0] = 0.0; f[1] = 0.0; f[2] = 0.0;
    v |= LOOP_GROUND_NORMAL;
  }
  if (f[2] > fz_max) {
    f[2] = fz_max;
    v |= LOOP_GROUND_NORMAL;
  }
  const double t = sqrt(f[0] * f[0] + f[1] * f[1]);
  const double cap = mu * f[2];
  if (t > cap) {
    const double s = cap / t;
    f[0] *= s; f[1] *= s;
    v |= LOOP_GROUND_FRICTION;
  }
  return v;
}

// A ground record limits something when at least one of its eight fields is finite (x - x is 0 only for a finite x); the legs
// of an all-+inf record are not looked at
QMPC_HD bool loop_ground_active(const qmpc_ground_params& g) {
  QMPC_NO_CONTRACT
  bool any = false;
  for (int l = 0; l < 4; ++l) any = any || (g.mu[l] - g.mu[l] == 0.0) || (g.fz_max[l] - g.fz_max[l] == 0.0);
  return any;
}

// ... and is valid when no field is NaN, every mu >= 0 and every fz_max > 0 (+inf passes both); the robot of an invalid one is
// frozen like that of an invalid plant record
QMPC_HD bool loop_ground_valid(const qmpc_ground_params& g) {
  bool ok = true;
  for (int l = 0; l < 4; ++l) ok = ok && (g.mu[l] >= 0.0) && (g.fz_max[l] > 0.0);      // (a NaN fails either comparison)
  return ok;
}

// The ground's part of one tick: grf (12, world frame, as the back end formed it) is clamped leg by leg where
// contacts[l] != 0 (swing legs are not looked at), verdict[l] gets loop_ground_leg's word (0 for a swing leg).  Returns the OR
// of the four.  An inactive record leaves everything alone.
QMPC_HD int loop_ground_clamp(const qmpc_ground_params& g, const double* contacts, double* grf, int* verdict) {
  int any = 0;
  const bool active = loop_ground_active(g);
  for (int l = 0; l < 4; ++l) {
    verdict[l] = (active && contacts[l] != 0.0) ? loop_ground_leg(g.mu[l], g.fz_max[l], grf + 3 * l) : 0;
    any |= verdict[l];
  }
  return any;
}

// The tally of a tick with these verdicts; tick_after is state.tick AFTER the tick
QMPC_HD void loop_ground_tally_one(const int* verdict, double tick_after, qmpc_ground_tally& t) {
  int any = 0;
  for (int l = 0; l < 4; ++l) {
    any |= verdict[l];
    if (verdict[l] & LOOP_GROUND_FRICTION) t.friction_leg_ticks += 1.0;
    if (verdict[l] & LOOP_GROUND_NORMAL) t.normal_leg_ticks += 1.0;
  }
  if (any) {
    t.clipped_ticks += 1.0;
    if (t.first_clipped_tick < 0.0) t.first_clipped_tick = tick_after;
  }
}

// The delivered body-frame force of a clamped leg: R' f, in the expression shape of the ConvexMpc back end's R' u
QMPC_HD void loop_ground_to_body(const double* R, const double* f, double* fb) {
  QMPC_NO_CONTRACT
  for (int r = 0; r < 3; ++r) fb[r] = R[r] * f[0] + R[3 + r] * f[1] + R[6 + r] * f[2];
}

// The time between the solve and the force under the feet (qmpc_loop_run_actuation*, include/qmpc.h): a record is the identity
// when it neither delays nor lags -- its robot takes the ground call's post step as it stands
QMPC_HD bool loop_actuation_identity(const qmpc_actuation_params& p) { return p.delay_ticks == 0.0 && p.alpha == 1.0; }

// ... and is valid when delay_ticks is an integer in 0 .. QMPC_MAX_DELAY, alpha lies in (0, 1] and the reserved words are
// finite (a NaN fails every comparison; x - x is 0 only for a finite x); a line when its count is a non-negative integer
// that `+ 1.0` still advances (below 2^53).  The robot of an invalid one is frozen like that of an invalid plant record.
QMPC_HD bool loop_actuation_valid(const qmpc_actuation_params& p, const qmpc_actuation_line& line) {
  QMPC_NO_CONTRACT
  bool ok = p.delay_ticks >= 0.0 && p.delay_ticks <= (double)QMPC_MAX_DELAY && p.delay_ticks == (double)(int)p.delay_ticks;
  ok = ok && p.alpha > 0.0 && p.alpha <= 1.0;
  ok = ok && (p.reserved[0] - p.reserved[0] == 0.0) && (p.reserved[1] - p.reserved[1] == 0.0);
  const double n = line.count;
  ok = ok && n >= 0.0 && n < 9007199254740992.0 && n == (double)(long long)n;
  return ok;
}

// One tick of a robot's actuation (the rule of include/qmpc.h in full): c (12) is the tick's body-frame command, contacts (4)
// its stance flags, a (12) receives the body-frame force the actuators produce.  Push c into slot count mod 8; the target y is
// the slot of command count - delay_ticks (before the first command: the slot that still holds the initial force; `& 7` of a
// negative two's-complement number is its non-negative remainder).  Each word of the target's slot is read before the
// command's word is written, since with delay_ticks = QMPC_MAX_DELAY the two are one slot; with delay_ticks = 0 y is c itself.
// alpha == 1: a = y as bytes; otherwise a = applied + alpha * (y - applied).  A swing leg delivers +0.0 and its applied becomes
// +0.0.  Then applied = a, count += 1.  The ring is indexed in the line's own memory (global memory on the device): one slot
// read, one written, applied read-modify-written, no local copy of the line.  p and line must be valid (loop_actuation_valid).
QMPC_HD void loop_actuation_one(const qmpc_actuation_params& p, qmpc_actuation_line& line, const double* c, const double* contacts,
                                double* a) {
  QMPC_NO_CONTRACT
  const long long n = (long long)line.count;
  const int d = (int)p.delay_ticks;
  const double alpha = p.alpha;
  double* wr = line.cmd[(int)(n & (QMPC_MAX_DELAY - 1))];
  const double* rd = line.cmd[(int)((n - d) & (QMPC_MAX_DELAY - 1))];
  for (int l = 0; l < 4; ++l)
    for (int r = 0; r < 3; ++r) {
      const int k = 3 * l + r;
      const double old = rd[k];
      wr[k] = c[k];
      const double y = d == 0 ? c[k] : old;
      double v;
      if (contacts[l] == 0.0) v = 0.0;
      else if (alpha == 1.0) v = y;
      else {
        const double ap = line.applied[k];
        v = ap + alpha * (y - ap);
      }
      a[k] = v;
      line.applied[k] = v;
    }
  line.count = (double)(n + 1);
}

// What the controller reads instead of the plant's state (qmpc_loop_run_sensing*, include/qmpc.h): a record is the identity
// when all of bias and sigma are zero (either sign; the seed is not looked at) -- its robot takes the front end as it stands
QMPC_HD bool loop_sense_identity(const qmpc_sense_params& p) {
  bool id = true;
  for (int c = 0; c < 12; ++c) id = id && p.bias[c] == 0.0 && p.sigma[c] == 0.0;
  return id;
}

// ... and is valid when every field is finite (a NaN fails every comparison; x - x is 0 only for a finite x), no sigma is
// negative and the seed is an integer in [0, 2^53).  The robot of an invalid one is frozen like that of an invalid plant record.
QMPC_HD bool loop_sense_valid(const qmpc_sense_params& p) {
  QMPC_NO_CONTRACT
  bool ok = true;
  for (int c = 0; c < 12; ++c) ok = ok && (p.bias[c] - p.bias[c] == 0.0) && (p.sigma[c] - p.sigma[c] == 0.0) && p.sigma[c] >= 0.0;
  for (int c = 0; c < 7; ++c) ok = ok && (p.reserved[c] - p.reserved[c] == 0.0);
  const double sd = p.seed;
  ok = ok && sd >= 0.0 && sd < 9007199254740992.0 && sd == (double)(long long)sd;
  return ok;
}

// S of channel c in the tick that starts at t, for an integer seed: the sum of the four 16-bit fields of
// mix(seed + 0x9E3779B97F4A7C15 * (12 t + c + 1)), mix the splitmix64 finaliser; 64-bit wrapping integer arithmetic only
QMPC_HD unsigned loop_sense_sum(unsigned long long seed, unsigned long long t, int c) {
  unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (12ull * t + (unsigned long long)c + 1ull);
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (unsigned)(z & 0xFFFFull) + (unsigned)((z >> 16) & 0xFFFFull) + (unsigned)((z >> 32) & 0xFFFFull) + (unsigned)(z >> 48);
}

// ... and n of it: an Irwin-Hall(4) variate, mean 0, variance 1, |n| <= 131070 / sqrt((2^32 - 1) / 3) = 3.4641 (2 sqrt 3) --
// bounded on purpose.  One conversion and one multiply by 1 / sqrt((2^32 - 1) / 3): no libm, the same bits on every side.
QMPC_HD double loop_sense_noise(unsigned long long seed, unsigned long long t, int c) {
  QMPC_NO_CONTRACT
  return (double)(int)(loop_sense_sum(seed, t, c) - 131070u) * 0x1.bb67ae86627e7p-16;
}

// One tick's measurement (the rule of include/qmpc.h in full): x (13) = pos_world[3] quat[4] lin_vel_world[3] ang_vel_body[3]
// of the true state, tick = state.tick, m (13) receives what the controller reads.  Per channel e = bias + sigma * n, the
// hash evaluated only where sigma != 0; a channel with bias == 0 and sigma == 0 copies its field as bytes.  Position, velocity
// and body rate: m = x + e.  Attitude, when one of channels 3-5 is active: q_m = normalize(q (x) (1, phi / 2)), scalar first,
// the norm written as the front end writes quat_d's (sqrt of the four squares summed left to right, four divisions): a
// rotation by 2 atan(|phi| / 2) about phi, no sin / cos; otherwise the quaternion is copied as bytes.  p must be valid
// (loop_sense_valid).  x and m must not overlap.
QMPC_HD void loop_sense_one(const qmpc_sense_params& p, double tick, const double* x, double* m) {
  QMPC_NO_CONTRACT
  const unsigned long long seed = (unsigned long long)(long long)p.seed, t = (unsigned long long)(long long)tick;
  double e[12];
  bool on[12];
  for (int c = 0; c < 12; ++c) {
    on[c] = !(p.bias[c] == 0.0 && p.sigma[c] == 0.0);
    e[c] = 0.0;
    if (on[c]) e[c] = p.sigma[c] == 0.0 ? p.bias[c] : p.bias[c] + p.sigma[c] * loop_sense_noise(seed, t, c);
  }
  for (int a = 0; a < 3; ++a) {
    m[a] = on[a] ? x[a] + e[a] : x[a];
    m[7 + a] = on[6 + a] ? x[7 + a] + e[6 + a] : x[7 + a];
    m[10 + a] = on[9 + a] ? x[10 + a] + e[9 + a] : x[10 + a];
  }
  if (on[3] || on[4] || on[5]) {
    const double w = x[3], qx = x[4], qy = x[5], qz = x[6];
    const double a = 0.5 * e[3], b = 0.5 * e[4], c = 0.5 * e[5];
    double q[4] = {w - qx * a - qy * b - qz * c, w * a + qx + qy * c - qz * b, w * b - qx * c + qy + qz * a,
                   w * c + qx * b - qy * a + qz};
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int k = 0; k < 4; ++k) m[3 + k] = q[k] / n;
  } else {
    for (int k = 0; k < 4; ++k) m[3 + k] = x[3 + k];
  }
}

// ---- a robot's own gait (qmpc_loop_run_gaits*, include/qmpc.h): the rule, for the kernels, the host classes and the tests ----
// The leg's two-entry pattern and its switch times
QMPC_HD double loop_gait_pattern(const qmpc_gait_params& g, int leg, int idx) {
  return (idx == 0) == (g.first_stance[leg] != 0.0) ? 1.0 : 0.0;
}
QMPC_HD double loop_gait_switch_time(const qmpc_gait_params& g, int leg, int idx) { return idx == 0 ? g.split[leg] : 1.0; }
// the fraction of a cycle the leg swings (the trot's 0.5 in the reference's swing times and Raibert stance time)
QMPC_HD double loop_gait_swing_fraction(const qmpc_gait_params& g, int leg) {
  QMPC_NO_CONTRACT
  return g.first_stance[leg] != 0.0 ? 1.0 - g.split[leg] : g.split[leg];
}

// A record is the identity when it is the reference's trot at the call's frequency: its robot takes the front end as it stands
QMPC_HD bool loop_gait_identity(const qmpc_gait_params& g, double lp_gait_freq) {
  bool id = g.gait_freq == lp_gait_freq;
  for (int l = 0; l < 4; ++l)
    id = id && g.first_stance[l] == ((l == 0 || l == 3) ? 1.0 : 0.0) && g.split[l] == 0.5 && g.phase0[l] == 0.0;
  return id;
}

// x in [0, 2) -> its fractional part; exact
QMPC_HD double loop_gait_frac(double x) {
  QMPC_NO_CONTRACT
  return x >= 1.0 ? x - 1.0 : x;
}

// ... and valid when (include/qmpc.h) every field is finite and the reserved words are 0, 0 < gait_freq and gait_freq * dt <= 1/16,
// first_stance is 0 or 1, split is a multiple of 2^-8 in [1/8, 7/8], phase0 a multiple of 2^-8 in [0, 1), and no flight is
// planned: the end of every leg's stance arc, in the robot's phase, lies in some leg's stance arc.  All of the arc arithmetic is
// exact: sums and differences of multiples of 2^-8 below 2.
QMPC_HD bool loop_gait_valid(const qmpc_gait_params& g, double dt) {
  QMPC_NO_CONTRACT
  bool ok = (g.gait_freq - g.gait_freq == 0.0) && g.gait_freq > 0.0 && g.gait_freq * dt <= 0.0625;
  for (int c = 0; c < 3; ++c) ok = ok && g.reserved[c] == 0.0;
  for (int l = 0; l < 4; ++l) {
    const double fs = g.first_stance[l], sp = g.split[l], ph = g.phase0[l];
    ok = ok && (fs == 0.0 || fs == 1.0);
    ok = ok && sp >= 0.125 && sp <= 0.875 && sp * 256.0 == (double)(int)(sp * 256.0);
    ok = ok && ph >= 0.0 && ph < 1.0 && ph * 256.0 == (double)(int)(ph * 256.0);
  }
  if (!ok) return false;
  double A[4], len[4];
  for (int l = 0; l < 4; ++l) {
    const bool fs = g.first_stance[l] != 0.0;
    const double a = fs ? 0.0 : g.split[l];
    len[l] = fs ? g.split[l] : 1.0 - g.split[l];
    A[l] = loop_gait_frac(a - g.phase0[l] + 1.0);
  }
  for (int l = 0; l < 4; ++l) {
    const double E = loop_gait_frac(A[l] + len[l]);
    bool covered = false;
    for (int m = 0; m < 4; ++m) covered = covered || loop_gait_frac(E - A[m] + 1.0) < len[m];
    ok = ok && covered;
  }
  return ok;
}

// The reset of one leg (LeggedContactFSM.cpp:11-31 with the record's pattern and the leg's own starting phase)
QMPC_HD void loop_gait_reset(const qmpc_gait_params& g, int leg, qmpc_loop_leg& L) {
  const double ph = g.phase0[leg], sp = g.split[leg];
  const int idx = ph < sp ? 0 : 1;
  L.gait_phase = ph;
  L.pattern_index = (double)idx;
  L.prev_pattern_index = (double)(1 - idx);
  L.start_time = idx ? sp : 0.0;
  L.end_time = idx ? 1.0 : sp;
  if (L.state == 0.0) {
    for (int a = 0; a < 3; ++a) { L.fsm_pos[a] = L.swing_end[a]; L.fsm_vel[a] = 0.0; }
  }
  L.state = loop_gait_pattern(g, leg, idx);
  L.not_first_call = 0.0;
}
QMPC_HD void loop_gait_common_enter(const qmpc_gait_params& g, int leg, qmpc_loop_leg& L) {   // :208-223
  QMPC_NO_CONTRACT
  const int prev = (int)L.pattern_index;
  const int idx = (prev + 1) % 2;
  L.prev_pattern_index = (double)prev;
  L.pattern_index = (double)idx;
  if (idx < prev) L.gait_phase -= 1.0;
  L.start_time = L.gait_phase;
  L.end_time = loop_gait_switch_time(g, leg, idx);
}
QMPC_HD double loop_gait_percent(const qmpc_loop_leg& L) {   // :261-270
  QMPC_NO_CONTRACT
  double percent = (L.gait_phase - L.start_time) / (L.end_time - L.start_time);
  if (percent < 0.0) percent = 0.0;
  else if (percent > 1.0) percent = 1.0;
  return percent;
}
// One update of one leg (:33-78): the schedule step and the foot targets of the state entered / held.  swing(t, T, start, fin,
// out) is the side's swing-foot quintic (the device's loop_swing_target, the host's QuinticCurveHip).
template <class Swing>
QMPC_HD double loop_gait_update(const qmpc_gait_params& g, int leg, qmpc_loop_leg& L, double dt, const double* cur, const double* tgt,
                                bool flag, Swing swing) {
  QMPC_NO_CONTRACT
  if (L.not_first_call == 0.0) {
    for (int a = 0; a < 3; ++a) {
      L.swing_start[a] = cur[a];
      L.swing_end[a] = tgt[a];
      L.fsm_pos[a] = tgt[a];
      L.fsm_vel[a] = 0.0;
    }
    L.not_first_call = 1.0;
  }
  L.gait_phase += g.gait_freq * dt;
  if (L.state == 1.0) {
    if (L.gait_phase >= L.end_time) {
      L.terrain_height = cur[2];                        // stance_exit
      loop_gait_common_enter(g, leg, L);                // swing_enter
      for (int a = 0; a < 3; ++a) { L.swing_start[a] = cur[a]; L.swing_extend[a] = 0.0; }
      L.state = 0.0;
    }
  } else {
    if ((loop_gait_percent(L) > 0.9 && flag) || loop_gait_percent(L) >= 1.0) {
      L.state = 1.0;
      loop_gait_common_enter(g, leg, L);                // stance_enter
      for (int a = 0; a < 3; ++a) { L.fsm_pos[a] = cur[a]; L.fsm_vel[a] = 0.0; }
    }
  }
  if (L.state == 0.0) {                                 // swing_update
    const double t = loop_gait_percent(L);
    const double w = loop_gait_swing_fraction(g, leg);
    double fin[3], out[9];
    for (int a = 0; a < 3; ++a) fin[a] = tgt[a] + L.swing_extend[a];
    swing((float)(w * t / g.gait_freq), (float)(w / g.gait_freq), L.swing_start, fin, out);
    for (int a = 0; a < 3; ++a) { L.fsm_pos[a] = out[a]; L.fsm_vel[a] = out[3 + a]; L.fsm_acc[a] = out[6 + a]; }
  }
  return L.gait_phase;
}
// The contact schedule a robot's gait state implies over a horizon of N knots h apart (qmpc_gait_predict, include/qmpc.h; the
// rows qmpc_solve_schedule* reads): masks[k], bit l set where leg l stands during knot k.  Knot 0 is the state's current contacts;
// then a COPY of each leg's schedule fields (gait_phase, state, pattern_index, start_time, end_time) is advanced N - 1 times by
// gait_freq h with exactly the schedule step of loop_gait_update -- the stance-exit test, the percent >= 1 swing exit,
// loop_gait_common_enter -- without an early contact (flag = false) and without the swing trajectory.  Nothing in *s changes.
QMPC_HD void loop_gait_predict(const qmpc_gait_params& g, const qmpc_loop_state& s, double h, int N, unsigned char* masks) {
  QMPC_NO_CONTRACT
  if (N < 1) return;
  qmpc_loop_leg L[4] = {};
  unsigned m0 = 0;
  for (int l = 0; l < 4; ++l) {
    L[l].gait_phase = s.leg[l].gait_phase;
    L[l].state = s.leg[l].state;
    L[l].pattern_index = s.leg[l].pattern_index;
    L[l].start_time = s.leg[l].start_time;
    L[l].end_time = s.leg[l].end_time;
    m0 |= (s.contacts[l] != 0.0) ? (1u << l) : 0u;
  }
  masks[0] = (unsigned char)m0;
  for (int k = 1; k < N; ++k) {
    unsigned m = 0;
    for (int l = 0; l < 4; ++l) {
      L[l].gait_phase += g.gait_freq * h;
      if (L[l].state == 1.0) {
        if (L[l].gait_phase >= L[l].end_time) {
          loop_gait_common_enter(g, l, L[l]);               // swing_enter
          L[l].state = 0.0;
        }
      } else if (loop_gait_percent(L[l]) >= 1.0) {
        L[l].state = 1.0;
        loop_gait_common_enter(g, l, L[l]);                 // stance_enter
      }
      m |= (L[l].state != 0.0) ? (1u << l) : 0u;
    }
    masks[k] = (unsigned char)m;
  }
}
// Raibert foothold offset of one leg in the yaw frame (BaseInterface.cpp:266-288 with the leg's own stance time (1 / f)(1 - w)):
// vrel = R_z' v, vd = last tick's torso_lin_vel_d_rel, k = sqrt(|z| / 9.81); d (3) receives the clamped offset, d[2] = 0
QMPC_HD void loop_gait_raibert_delta(const qmpc_gait_params& g, int leg, double k, const double* vrel, const double* vd, double* d) {
  QMPC_NO_CONTRACT
  const double w = loop_gait_swing_fraction(g, leg);
  d[0] = k * (vrel[0] - vd[0]) + (1.0 / g.gait_freq) * (1.0 - w) * vd[0];
  if (d[0] < -0.5) d[0] = -0.5;
  if (d[0] > 0.5) d[0] = 0.5;
  d[1] = k * (vrel[1] - vd[1]) + (1.0 / g.gait_freq) * (1.0 - w) * vd[1];
  if (d[1] < -0.3) d[1] = -0.3;
  if (d[1] > 0.3) d[1] = 0.3;
  d[2] = 0.0;
}

// Condition matrix of the swing-foot quintic p(t) = sum_k a_k t^k (QuinticCurve::get_foot_swing_target,
// Utils.cpp:236-293): rows p(0), p(T), p'(0), p'(T), p(T/2), p'(T/2).  Generated, with the reference's FLOAT
// evaluation order so that every entry carries the same rounding as upstream's hand-written expressions: a power is
// the left-to-right product  (c * T) * T * ...  started from the derivative factor c, and the half-time rows divide
// that product by 2^j afterwards.
QMPC_HD void swing_condition_matrix(float T, double C[6][6]) {
  QMPC_NO_CONTRACT
  for (int r = 0; r < 6; ++r)
    for (int k = 0; k < 6; ++k) C[r][k] = 0.0;
  C[0][0] = 1.0;                                   // p(0)
  C[2][1] = 1.0;                                   // p'(0)
  for (int k = 0; k < 6; ++k) {
    float pw = 1.0f;                               // T^k
    for (int j = 0; j < k; ++j) pw = pw * T;
    C[1][k] = pw;                                  // p(T)
    C[4][k] = (k == 0) ? 1.0f : pw / (float)(1 << k);             // p(T/2) = T^k / 2^k
    if (k >= 1) {
      float dv = (float)k;                         // k T^(k-1), as (k * T) * T * ...
      for (int j = 0; j < k - 1; ++j) dv = dv * T;
      C[3][k] = (k == 1) ? 1.0f : dv;              // p'(T)
      C[5][k] = (k == 1) ? 1.0f : dv / (float)(1 << (k - 1));     // p'(T/2) = k T^(k-1) / 2^(k-1)
    }
  }
}

// 3x3 inverse by cofactors (row-major)
QMPC_HD void inv3(const double* A, double* B) {
  QMPC_NO_CONTRACT
  const double c00 = A[4] * A[8] - A[5] * A[7], c01 = A[5] * A[6] - A[3] * A[8], c02 = A[3] * A[7] - A[4] * A[6];
  const double id = 1.0 / (A[0] * c00 + A[1] * c01 + A[2] * c02);
  B[0] = c00 * id; B[1] = (A[2] * A[7] - A[1] * A[8]) * id; B[2] = (A[1] * A[5] - A[2] * A[4]) * id;
  B[3] = c01 * id; B[4] = (A[0] * A[8] - A[2] * A[6]) * id; B[5] = (A[2] * A[3] - A[0] * A[5]) * id;
  B[6] = c02 * id; B[7] = (A[1] * A[6] - A[0] * A[7]) * id; B[8] = (A[0] * A[4] - A[1] * A[3]) * id;
}

}  // namespace qmpc_loop
