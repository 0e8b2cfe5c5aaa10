// qmpc_loop_rec.inc -- the kernels of the closed loop with per-robot records and their launchers, defined once.  Included by
// qmpc_loop_inst.hip, qmpc_loop_outcome.hip, qmpc_loop_push.hip, qmpc_loop_ground.hip, qmpc_loop_act.hip, qmpc_loop_sense.hip,
// qmpc_loop_gait.hip and qmpc_loop_motor.hip inside the unit's namespace, after qmpc_loop.hip, with
//   QMPC_REC_EXT 0   controller and plant records only                          (qmpc_loop_run_instances*)
//                1   ... and the outcome step after the post step               (qmpc_loop_run_outcomes*)
//                2   ... whose plant step integrates under timed push windows   (qmpc_loop_run_pushes*)
//                3   ... under the force the robot's true ground delivers       (qmpc_loop_run_ground*; qmpc_loop_cground.hip: the
//                    same with QMPC_REC_CONVEX, beside qmpc_loop_crec.hip, which stays at EXT 2)
//                4   ... through the robot's delay line and actuator lag         (qmpc_loop_run_actuation*; qmpc_loop_cact.hip: the
//                    same with QMPC_REC_CONVEX; the ground record may be absent)
//                5   ... whose controller reads a measured state                 (qmpc_loop_run_sensing*; qmpc_loop_csense.hip: the
//                    same with QMPC_REC_CONVEX; the actuation record may be absent too).  The first layer in the FRONT end
//                6   ... and walks the robot's own gait                          (qmpc_loop_run_gaits*; qmpc_loop_cgait.hip: the
//                    same with QMPC_REC_CONVEX; the sensing record may be absent too)
//                7   ... whose delivered foot force respects the motors' torque limits (qmpc_loop_run_motors*; qmpc_loop_cmotor.hip:
//                    the same with QMPC_REC_CONVEX; the gait record may be absent too).  Back in the POST step
// and, for the sibling controller (qmpc_loop_crec.hip; a handle opts in with qmpc_set_convex_records),
//   QMPC_REC_CONVEX  defined: ConvexMpc's problem -- ConvexModel and the wrench-form body with QMPC_WMODEL WM_CONVEX, the front
//                    end loop_front_convex_one on qmpc_convex_input records, the world-frame back end with the robot's plant
//                    (loop_post_plant_world_one below).  That unit is built at EXT 2 and has a front kernel of its own; it serves
//                    the three calls (the calls without windows pass per_robot = 0, the call without outcome records a scratch).
// Textual inclusion, not a template over EXT: each unit compiles to the instructions it had as a file of its own (a shared
// __forceinline__ function template moved the register assignment of every kernel; DESIGN.md).  The parameters a smaller EXT
// does not have are written with the two macros below; a kernel's parameter list is that of its EXT and of no other.
//   per tick    qmpc_loop_rec_front_kernel (EXT 0 / 1 / 5 / 6; the calls of EXT 2-4 launch the outcome unit's) and qmpc_loop_rec_post_kernel
//               around the solve the C entry point launches
//   persistent  qmpc_loop_rec_fused_kernel<3|5|6>: qmpc_loop_fused_kernel<VAR, false, false, false> (QuatMpc's problem,
//               converged mode, wrench-form body) with the robot's own controller and plant
//   launchers   rec_set_lds, rec_fused_launch, rec_front_launch, rec_post_launch: one signature for all units -- the call's
//               buffers (rec_launch) and its records (loop_recs), both of qmpc_loop_records.h, of which a unit passes its
//               kernels what they take (declared for qmpc_hip.hip by its QMPC_REC_DECLARE)
#ifdef QMPC_REC_CONVEX
#define QMPC_REC_MODEL ConvexModel
#define QMPC_REC_FRONT(OCC_, LP_, s_, r_) loop_front_convex_one<OCC_>(LP_, s_, reinterpret_cast<qmpc_convex_input&>(r_))
#else
#define QMPC_REC_MODEL QuatModel
#define QMPC_REC_FRONT(OCC_, LP_, s_, r_) loop_front_one<OCC_>(LP_, s_, r_)
#endif
// the post step and, at EXT 3, the two arguments it has beyond the plant block: robot i_'s ground record and tally; at EXT 4
// (where there may be no ground record) the robot's actuation record and delay line after them; at EXT 5 those may be absent too
#if QMPC_REC_EXT >= 7
#define QMPC_REC_POST loop_post_actuation_one
#define QMPC_REC_POST_GROUND(i_)                                                                                               \
  , ground ? ground + (size_t)(i_) : nullptr, tally ? tally + (size_t)(i_) : nullptr, act ? act + (size_t)(i_) : nullptr, \
      line ? line + (size_t)(i_) : nullptr, G, motor + (size_t)(i_), mtally + (size_t)(i_)
#elif QMPC_REC_EXT >= 5
#define QMPC_REC_POST loop_post_actuation_one
#define QMPC_REC_POST_GROUND(i_)                                                                                               \
  , ground ? ground + (size_t)(i_) : nullptr, tally ? tally + (size_t)(i_) : nullptr, act ? act + (size_t)(i_) : nullptr, \
      line ? line + (size_t)(i_) : nullptr
#elif QMPC_REC_EXT >= 4
#define QMPC_REC_POST loop_post_actuation_one
#define QMPC_REC_POST_GROUND(i_) \
  , ground ? ground + (size_t)(i_) : nullptr, tally ? tally + (size_t)(i_) : nullptr, act + (size_t)(i_), line + (size_t)(i_)
#elif QMPC_REC_EXT >= 3
#define QMPC_REC_POST loop_post_ground_one
#define QMPC_REC_POST_GROUND(i_) , ground + (size_t)(i_), tally ? tally + (size_t)(i_) : nullptr
#elif defined(QMPC_REC_CONVEX)
#define QMPC_REC_POST loop_post_plant_world_one
#define QMPC_REC_POST_GROUND(i_)
#else
#define QMPC_REC_POST loop_post_plant_one
#define QMPC_REC_POST_GROUND(i_)
#endif
#if QMPC_REC_EXT >= 1
#define QMPC_REC_OUTCOME(...) __VA_ARGS__
#else
#define QMPC_REC_OUTCOME(...)
#endif
#if QMPC_REC_EXT >= 2
#define QMPC_REC_PUSH(...) __VA_ARGS__
#else
#define QMPC_REC_PUSH(...)
#endif
#if QMPC_REC_EXT >= 3
#define QMPC_REC_GROUND(...) __VA_ARGS__
#else
#define QMPC_REC_GROUND(...)
#endif
#if QMPC_REC_EXT >= 4
#define QMPC_REC_ACT(...) __VA_ARGS__
#else
#define QMPC_REC_ACT(...)
#endif
#if QMPC_REC_EXT >= 5
#define QMPC_REC_SENSE(...) __VA_ARGS__
#else
#define QMPC_REC_SENSE(...)
#endif
#if QMPC_REC_EXT >= 6
#define QMPC_REC_GAIT(...) __VA_ARGS__
// the front end of a robot with a non-identity gait record g_
#ifdef QMPC_REC_CONVEX
#define QMPC_REC_FRONT_GAIT(OCC_, LP_, s_, r_, g_) loop_front_convex_gait_one<OCC_>(LP_, s_, reinterpret_cast<qmpc_convex_input&>(r_), g_)
#else
#define QMPC_REC_FRONT_GAIT(OCC_, LP_, s_, r_, g_) loop_front_gait_one<OCC_>(LP_, s_, r_, g_)
#endif
#else
#define QMPC_REC_GAIT(...)
#endif
#if QMPC_REC_EXT >= 7
#define QMPC_REC_MOTOR(...) __VA_ARGS__
#else
#define QMPC_REC_MOTOR(...)
#endif

// the trace row of a robot that does not move in this tick
__device__ inline void loop_zero_row(double* __restrict__ trace_f, double* __restrict__ trace_c) {
  if (trace_f) for (int a = 0; a < 12; ++a) trace_f[a] = 0.0;
  if (trace_c) for (int a = 0; a < 4; ++a) trace_c[a] = 0.0;
}

// A frozen robot (invalid record): its state untouched except status and iterations, its trace row of this tick zero
__device__ inline void loop_freeze(qmpc_loop_state& s, double* __restrict__ trace_f, double* __restrict__ trace_c) {
  s.status = (double)QMPC_BAD_PARAMS;
  s.iterations = 0.0;
  loop_zero_row(trace_f, trace_c);
}

#if QMPC_REC_EXT >= 1
// the robot of record o is halted: it went down in an earlier tick (or call) and the caller asked to stop such robots
__device__ inline bool outcome_halted(const qmpc_outcome_params& OP, const qmpc_loop_outcome& o) {
  return OP.stop_when_down != 0.0 && o.down_tick >= 0.0;
}
#endif

#if QMPC_REC_EXT >= 2
// the robot's plant block with the effective wrench of the tick that starts at state.tick = t
__device__ inline PlantDev push_plant(const PlantDev& pl, const qmpc_push_params* __restrict__ w, int per_robot, double t) {
  PlantDev p = pl;
  qmpc_loop::loop_push_wrench(w, per_robot, t, p.force, p.torque);
  return p;
}
#endif

#if QMPC_REC_EXT >= 7
// The motor step of a robot's tick (qmpc_loop_run_motors*; the rule: qmpc_joint::loop_motor_one of qmpc_joint_math.h), called by
// loop_post_actuation_one below once u, the body-frame force the actuators produce, is known.  Out of line: the inverse
// kinematics and the 3x3 elimination get a register allocation of their own and stay out of the solve's.  m and t point at the
// robot's 128 B record and 320 B tally in global memory; t is read-modify-written in place.  um receives u' on the legs with
// changed[l] != 0.  s is read only: R, pos_world and foot_pos_world are the pose before the plant step, s.tick + 1 the tick after.
__device__ __noinline__ int loop_post_motor(const LegGeom& G, const qmpc_motor_params* __restrict__ m, qmpc_motor_tally* __restrict__ t,
                                            const double* R, const qmpc_loop_state& s, const double* u, double* um, int* changed) {
  return qmpc_joint::loop_motor_one(G.rho_opt, G.rho_fix, *m, *t, R, s.pos_world, s.foot_pos_world, s.contacts, u, s.tick + 1.0, um,
                                    changed);
}
// dst_[3l ..] = R u' on the legs the motors changed, in the expression of the non-identity actuation branch
#define QMPC_REC_MOTOR_GRF(dst_)                                                                                         \
  do {                                                                                                                   \
    for (int l = 0; l < 4; ++l)                                                                                          \
      if (mch[l])                                                                                                        \
        for (int r = 0; r < 3; ++r)                                                                                      \
          (dst_)[3 * l + r] = R[3 * r] * um[3 * l] + R[3 * r + 1] * um[3 * l + 1] + R[3 * r + 2] * um[3 * l + 2];       \
  } while (0)
#endif

#if QMPC_REC_EXT >= 4
// The back end of a tick whose force reaches the feet through the robot's delay line and actuator lag
// (qmpc_loop_run_actuation*), a sibling of loop_post_ground_one below.  After forces_body holds the tick's command,
// qmpc_loop::loop_actuation_one pushes it into the line and returns a, the body-frame force the actuators produce.  A robot whose
// record is the identity then goes through loop_post_ground_one's text as it stands (a is not looked at; the line stays
// current), so it gets that function's state, bit for bit.  Any other robot forms grf_world = R a (a swing leg: +0.0), the
// stance legs are clamped as there, a changed leg hands the plant R' f and an unchanged one a.  g may be null: no clamp, the
// tally untouched.  grf_world holds the delivered force, forces_body and the trace row the command.  act, line, g and tally
// point into global memory: one ring slot is read, one written and applied read-modify-written here, inside the post step --
// nothing of the feature is live across the solve, no block is copied, the ring is indexed in global memory.
// EXT 7 (qmpc_loop_run_motors*): between a and the ground clamp the motor step (loop_post_motor above) runs on a -- or, for an
// identity robot, on the forces_body bytes.  A leg it changed gets grf_world = R u' before the clamp sees it and hands the plant
// u' (R' f if the ground changes it too); every other leg goes through the text below as it stands.  `applied` stays what the
// line made it.  ConvexMpc with a rejected solve and no ground record: only the changed legs' grf_world entries are written.
template <int OCC = 1>
QMPC_LOOP_FN void loop_post_actuation_one(const PlantDev& pl, const qmpc_loop_params& LP, qmpc_loop_state& s,
                                          const double* __restrict__ forces, const qmpc_info& inf, double* __restrict__ trace_f,
                                          double* __restrict__ trace_c, const qmpc_ground_params* __restrict__ g,
                                          qmpc_ground_tally* __restrict__ tally, const qmpc_actuation_params* __restrict__ act,
                                          qmpc_actuation_line* __restrict__ line
                                          QMPC_REC_MOTOR(, const LegGeom& G, const qmpc_motor_params* __restrict__ motor,
                                                         qmpc_motor_tally* __restrict__ mtally)) {
#pragma clang fp contract(off)
  const int status = inf.status;
  s.status = (double)status;
  s.iterations = (double)inf.iterations;
  const bool accepted = status == QMPC_OK || status == QMPC_MAX_ITER;     // (the converged mode only)
  double R[9];
  qmpc_loop::quat_to_rot(s.quat, R);
  int verdict[4] = {0, 0, 0, 0};
  int any = 0;
#if QMPC_REC_EXT >= 5
  const bool ident = !act || qmpc_loop::loop_actuation_identity(*act);     // (no record: every command acts in its own tick)
#else
  const bool ident = qmpc_loop::loop_actuation_identity(*act);
#endif
#ifdef QMPC_REC_CONVEX
  if (accepted)
    for (int l = 0; l < 4; ++l)
      for (int r = 0; r < 3; ++r) {
        s.grf_world[3 * l + r] = forces[3 * l + r];
        s.forces_body[3 * l + r] = R[r] * forces[3 * l] + R[3 + r] * forces[3 * l + 1] + R[6 + r] * forces[3 * l + 2];
      }
#else
  if (accepted)
    for (int a = 0; a < 12; ++a) s.forces_body[a] = forces[a];
#endif
  double u[12];      // what the plant receives
#if QMPC_REC_EXT >= 5
  if (act)
#endif
  qmpc_loop::loop_actuation_one(*act, *line, s.forces_body, s.contacts, u);
#if QMPC_REC_EXT >= 7
  double um[12];     // u' of the legs the motors changed (mch)
  int mch[4];
  const int many = loop_post_motor(G, motor, mtally, R, s, ident ? s.forces_body : u, um, mch);
#endif
  if (ident) {
#ifdef QMPC_REC_CONVEX
    if (accepted) {
#if QMPC_REC_EXT >= 7
      if (many) QMPC_REC_MOTOR_GRF(s.grf_world);
#endif
      if (g) any = qmpc_loop::loop_ground_clamp(*g, s.contacts, s.grf_world, verdict);
#if QMPC_REC_EXT >= 7
    } else if (g || many) {
      double fw[12];
      for (int l = 0; l < 4; ++l)
        for (int r = 0; r < 3; ++r)
          fw[3 * l + r] = R[3 * r] * s.forces_body[3 * l] + R[3 * r + 1] * s.forces_body[3 * l + 1] + R[3 * r + 2] * s.forces_body[3 * l + 2];
      if (many) QMPC_REC_MOTOR_GRF(fw);
      if (g) any = qmpc_loop::loop_ground_clamp(*g, s.contacts, fw, verdict);
      for (int l = 0; l < 4; ++l)
        if (verdict[l] || (many && mch[l]))
          for (int r = 0; r < 3; ++r) s.grf_world[3 * l + r] = fw[3 * l + r];
    }
#else
    } else if (g) {
      double fw[12];
      for (int l = 0; l < 4; ++l)
        for (int r = 0; r < 3; ++r)
          fw[3 * l + r] = R[3 * r] * s.forces_body[3 * l] + R[3 * r + 1] * s.forces_body[3 * l + 1] + R[3 * r + 2] * s.forces_body[3 * l + 2];
      any = qmpc_loop::loop_ground_clamp(*g, s.contacts, fw, verdict);
      for (int l = 0; l < 4; ++l)
        if (verdict[l])
          for (int r = 0; r < 3; ++r) s.grf_world[3 * l + r] = fw[3 * l + r];
    }
#endif
#else
    for (int l = 0; l < 4; ++l)
      for (int r = 0; r < 3; ++r)
        s.grf_world[3 * l + r] = R[3 * r] * s.forces_body[3 * l] + R[3 * r + 1] * s.forces_body[3 * l + 1] +
                                 R[3 * r + 2] * s.forces_body[3 * l + 2];
#if QMPC_REC_EXT >= 7
    if (many) QMPC_REC_MOTOR_GRF(s.grf_world);
#endif
    if (g) any = qmpc_loop::loop_ground_clamp(*g, s.contacts, s.grf_world, verdict);
#endif
    for (int a = 0; a < 12; ++a) u[a] = s.forces_body[a];
#if QMPC_REC_EXT >= 7
    if (many)
      for (int l = 0; l < 4; ++l)
        if (mch[l])
          for (int r = 0; r < 3; ++r) u[3 * l + r] = um[3 * l + r];
#endif
  } else {
#if QMPC_REC_EXT >= 7
    if (many)
      for (int l = 0; l < 4; ++l)
        if (mch[l])
          for (int r = 0; r < 3; ++r) u[3 * l + r] = um[3 * l + r];
#endif
    for (int l = 0; l < 4; ++l)
      for (int r = 0; r < 3; ++r)
        s.grf_world[3 * l + r] = s.contacts[l] == 0.0 ? 0.0
                                                      : R[3 * r] * u[3 * l] + R[3 * r + 1] * u[3 * l + 1] + R[3 * r + 2] * u[3 * l + 2];
    if (g) any = qmpc_loop::loop_ground_clamp(*g, s.contacts, s.grf_world, verdict);
  }
  if (trace_f) for (int a = 0; a < 12; ++a) trace_f[a] = s.forces_body[a];
  if (trace_c) for (int a = 0; a < 4; ++a) trace_c[a] = s.contacts[a];
  for (int l = 0; l < 4; ++l)
    if (verdict[l]) qmpc_loop::loop_ground_to_body(R, s.grf_world + 3 * l, u + 3 * l);
  double x[13];
  for (int a = 0; a < 3; ++a) { x[a] = s.pos_world[a]; x[7 + a] = s.lin_vel_world[a]; x[10 + a] = s.ang_vel_body[a]; }
  for (int a = 0; a < 4; ++a) x[3 + a] = s.quat[a];
  qmpc_loop::plant_step_ext(x, u, s.foot_pos_world, 4, pl.mass, pl.Iinv, pl.force, pl.torque, LP.dt);
  for (int a = 0; a < 3; ++a) { s.pos_world[a] = x[a]; s.lin_vel_world[a] = x[7 + a]; s.ang_vel_body[a] = x[10 + a]; }
  for (int a = 0; a < 4; ++a) s.quat[a] = x[3 + a];
  if (s.movement_mode != 0.0)
    for (int l = 0; l < 4; ++l)
      if (s.contacts[l] == 0.0)
        for (int a = 0; a < 3; ++a) s.foot_pos_world[3 * l + a] = s.leg[l].fsm_pos[a];
  s.tick += 1.0;
  if (tally && any) {
    qmpc_ground_tally t = *tally;
    qmpc_loop::loop_ground_tally_one(verdict, s.tick, t);
    *tally = t;
  }
}
#elif QMPC_REC_EXT >= 3
// The back end of a tick on the robot's TRUE ground (qmpc_loop_run_ground*): loop_post_plant_one (QMPC_REC_CONVEX:
// loop_post_plant_world_one) whose plant step takes the DELIVERED forces.  After grf_world has been formed as there, the stance
// legs are clamped in the world frame (qmpc_loop::loop_ground_clamp); a changed leg hands the plant R' f, an unchanged one the
// commanded forces_body bytes, so a record that changes no leg gives that function's state, bit for bit.  grf_world holds the
// delivered force, forces_body and the trace row the command.  g and tally point into global memory: the record is read and the
// tally read-modify-written here, inside the post step -- nothing of either is live across the solve, and no block is copied.
// ConvexMpc, solve rejected: grf_world still holds the last accepted tick's entry, so the clamp runs on R forces_body, the
// command the plant keeps applying; only a leg it changes is written.
template <int OCC = 1>
QMPC_LOOP_FN void loop_post_ground_one(const PlantDev& pl, const qmpc_loop_params& LP, qmpc_loop_state& s,
                                       const double* __restrict__ forces, const qmpc_info& inf, double* __restrict__ trace_f,
                                       double* __restrict__ trace_c, const qmpc_ground_params* __restrict__ g,
                                       qmpc_ground_tally* __restrict__ tally) {
#pragma clang fp contract(off)
  const int status = inf.status;
  s.status = (double)status;
  s.iterations = (double)inf.iterations;
  const bool accepted = status == QMPC_OK || status == QMPC_MAX_ITER;     // (the converged mode only)
  double R[9];
  qmpc_loop::quat_to_rot(s.quat, R);
  int verdict[4];
  int any;
#ifdef QMPC_REC_CONVEX
  if (accepted) {
    for (int l = 0; l < 4; ++l)
      for (int r = 0; r < 3; ++r) {
        s.grf_world[3 * l + r] = forces[3 * l + r];
        s.forces_body[3 * l + r] = R[r] * forces[3 * l] + R[3 + r] * forces[3 * l + 1] + R[6 + r] * forces[3 * l + 2];
      }
    any = qmpc_loop::loop_ground_clamp(*g, s.contacts, s.grf_world, verdict);
  } else {
    double fw[12];
    for (int l = 0; l < 4; ++l)
      for (int r = 0; r < 3; ++r)
        fw[3 * l + r] = R[3 * r] * s.forces_body[3 * l] + R[3 * r + 1] * s.forces_body[3 * l + 1] + R[3 * r + 2] * s.forces_body[3 * l + 2];
    any = qmpc_loop::loop_ground_clamp(*g, s.contacts, fw, verdict);
    for (int l = 0; l < 4; ++l)
      if (verdict[l])
        for (int r = 0; r < 3; ++r) s.grf_world[3 * l + r] = fw[3 * l + r];
  }
#else
  if (accepted)
    for (int a = 0; a < 12; ++a) s.forces_body[a] = forces[a];
  for (int l = 0; l < 4; ++l)
    for (int r = 0; r < 3; ++r)
      s.grf_world[3 * l + r] = R[3 * r] * s.forces_body[3 * l] + R[3 * r + 1] * s.forces_body[3 * l + 1] +
                               R[3 * r + 2] * s.forces_body[3 * l + 2];
  any = qmpc_loop::loop_ground_clamp(*g, s.contacts, s.grf_world, verdict);
#endif
  if (trace_f) for (int a = 0; a < 12; ++a) trace_f[a] = s.forces_body[a];
  if (trace_c) for (int a = 0; a < 4; ++a) trace_c[a] = s.contacts[a];
  double u[12];      // what the plant receives
  for (int l = 0; l < 4; ++l) {
    if (verdict[l]) qmpc_loop::loop_ground_to_body(R, s.grf_world + 3 * l, u + 3 * l);
    else
      for (int r = 0; r < 3; ++r) u[3 * l + r] = s.forces_body[3 * l + r];
  }
  double x[13];
  for (int a = 0; a < 3; ++a) { x[a] = s.pos_world[a]; x[7 + a] = s.lin_vel_world[a]; x[10 + a] = s.ang_vel_body[a]; }
  for (int a = 0; a < 4; ++a) x[3 + a] = s.quat[a];
  qmpc_loop::plant_step_ext(x, u, s.foot_pos_world, 4, pl.mass, pl.Iinv, pl.force, pl.torque, LP.dt);
  for (int a = 0; a < 3; ++a) { s.pos_world[a] = x[a]; s.lin_vel_world[a] = x[7 + a]; s.ang_vel_body[a] = x[10 + a]; }
  for (int a = 0; a < 4; ++a) s.quat[a] = x[3 + a];
  if (s.movement_mode != 0.0)
    for (int l = 0; l < 4; ++l)
      if (s.contacts[l] == 0.0)
        for (int a = 0; a < 3; ++a) s.foot_pos_world[3 * l + a] = s.leg[l].fsm_pos[a];
  s.tick += 1.0;
  if (tally && any) {
    qmpc_ground_tally t = *tally;
    qmpc_loop::loop_ground_tally_one(verdict, s.tick, t);
    *tally = t;
  }
}
#elif defined(QMPC_REC_CONVEX)
// The back end of ConvexMpc's tick with the robot's own TRUE plant: loop_post_one<true> (qmpc_loop.hip: the solve returns
// WORLD-frame forces, optimized_input = R' u; converged mode) with pl's mass, inverse inertia and disturbance wrench in the plant
// step, as loop_post_plant_one is loop_post_one<false> with them.  plant_step_ext with the handle's mass and inertia and a zero
// wrench gives plant_step's bits, so such a plant gives loop_post_one<true>'s state and trace rows.
template <int OCC = 1>
QMPC_LOOP_FN void loop_post_plant_world_one(const PlantDev& pl, const qmpc_loop_params& LP, qmpc_loop_state& s,
                                            const double* __restrict__ forces, const qmpc_info& inf, double* __restrict__ trace_f,
                                            double* __restrict__ trace_c) {
#pragma clang fp contract(off)
  const int status = inf.status;
  s.status = (double)status;
  s.iterations = (double)inf.iterations;
  const bool accepted = status == QMPC_OK || status == QMPC_MAX_ITER;     // (the converged mode only)
  double R[9];
  qmpc_loop::quat_to_rot(s.quat, R);
  if (accepted)
    for (int l = 0; l < 4; ++l)
      for (int r = 0; r < 3; ++r) {
        s.grf_world[3 * l + r] = forces[3 * l + r];
        s.forces_body[3 * l + r] = R[r] * forces[3 * l] + R[3 + r] * forces[3 * l + 1] + R[6 + r] * forces[3 * l + 2];
      }
  if (trace_f) for (int a = 0; a < 12; ++a) trace_f[a] = s.forces_body[a];
  if (trace_c) for (int a = 0; a < 4; ++a) trace_c[a] = s.contacts[a];
  double x[13];
  for (int a = 0; a < 3; ++a) { x[a] = s.pos_world[a]; x[7 + a] = s.lin_vel_world[a]; x[10 + a] = s.ang_vel_body[a]; }
  for (int a = 0; a < 4; ++a) x[3 + a] = s.quat[a];
  qmpc_loop::plant_step_ext(x, s.forces_body, s.foot_pos_world, 4, pl.mass, pl.Iinv, pl.force, pl.torque, LP.dt);
  for (int a = 0; a < 3; ++a) { s.pos_world[a] = x[a]; s.lin_vel_world[a] = x[7 + a]; s.ang_vel_body[a] = x[10 + a]; }
  for (int a = 0; a < 4; ++a) s.quat[a] = x[3 + a];
  if (s.movement_mode != 0.0)
    for (int l = 0; l < 4; ++l)
      if (s.contacts[l] == 0.0)
        for (int a = 0; a < 3; ++a) s.foot_pos_world[3 * l + a] = s.leg[l].fsm_pos[a];
  s.tick += 1.0;
}
#endif

#if QMPC_REC_EXT >= 5
// The front end of a tick whose controller reads a MEASURED state (qmpc_loop_run_sensing*).  A robot without a record, or whose
// record is the identity, runs the front end as it stands and its seen stays untouched.  Any other robot: the 13 true doubles
// at the head of the state (pos_world, quat, lin_vel_world, ang_vel_body) are saved, qmpc_loop::loop_sense_one's measurement of
// them is written in their place, the front end runs unchanged -- it writes none of the 13 --, the true doubles are put back as
// bytes and seen, when given, takes the measurement.  sense and seen point into global memory and are reached here, inside
// the front step: the 13 saved doubles live across the front end's call only, nothing of the feature across the solve.
// EXT 6 (qmpc_loop_run_gaits*): gait points at the robot's 128 B gait record in global memory, or is null.  Where this text says
// "the front end" a robot with a non-identity record runs loop_front_gait_one / loop_front_convex_gait_one on that record, read
// by reference inside that call; a robot without one, or with the identity, the fixed front end.  Nothing else changes.
template <int OCC = 1>
QMPC_LOOP_FN void loop_front_sense_one(const qmpc_loop_params& LP, qmpc_loop_state& s, qmpc_input& in,
                                       const qmpc_sense_params* __restrict__ sense, qmpc_sense_seen* __restrict__ seen
                                       QMPC_REC_GAIT(, const qmpc_gait_params* __restrict__ gait)) {
#pragma clang fp contract(off)
#if QMPC_REC_EXT >= 6
  const bool walk = gait && !qmpc_loop::loop_gait_identity(*gait, LP.gait_freq);
#define QMPC_REC_FRONT_PICK()                              \
  do {                                                     \
    if (walk) QMPC_REC_FRONT_GAIT(OCC, LP, s, in, *gait);  \
    else QMPC_REC_FRONT(OCC, LP, s, in);                   \
  } while (0)
#else
#define QMPC_REC_FRONT_PICK() QMPC_REC_FRONT(OCC, LP, s, in)
#endif
  if (!sense || qmpc_loop::loop_sense_identity(*sense)) {
    QMPC_REC_FRONT_PICK();
    return;
  }
  double x[13], m[13];
  for (int a = 0; a < 3; ++a) { x[a] = s.pos_world[a]; x[7 + a] = s.lin_vel_world[a]; x[10 + a] = s.ang_vel_body[a]; }
  for (int a = 0; a < 4; ++a) x[3 + a] = s.quat[a];
  qmpc_loop::loop_sense_one(*sense, s.tick, x, m);
  for (int a = 0; a < 3; ++a) { s.pos_world[a] = m[a]; s.lin_vel_world[a] = m[7 + a]; s.ang_vel_body[a] = m[10 + a]; }
  for (int a = 0; a < 4; ++a) s.quat[a] = m[3 + a];
  if (seen) {      // (before the call: m is not live across it)
    for (int a = 0; a < 13; ++a) seen->meas[a] = m[a];
    seen->ticks += 1.0;
  }
  QMPC_REC_FRONT_PICK();
  for (int a = 0; a < 3; ++a) { s.pos_world[a] = x[a]; s.lin_vel_world[a] = x[7 + a]; s.ang_vel_body[a] = x[10 + a]; }
  for (int a = 0; a < 4; ++a) s.quat[a] = x[3 + a];
#undef QMPC_REC_FRONT_PICK
}
#endif

// ---- per-tick form -----------------------------------------------------------------------------------------------------
#if QMPC_REC_EXT <= 1 || QMPC_REC_EXT >= 5 || defined(QMPC_REC_CONVEX)
// The front end of qmpc_loop_front_kernel; the record of a frozen robot, or of one halted under stop_when_down, gets a NaN
// attitude instead, which every solve kernel rejects before its first iteration (QMPC_NAN_INPUT; the post kernel ignores it)
__global__ __launch_bounds__(64) void qmpc_loop_rec_front_kernel(
    qmpc_loop_params LP, QMPC_REC_OUTCOME(qmpc_outcome_params OP, ) qmpc_loop_state* __restrict__ st, qmpc_input* __restrict__ rec,
    int* __restrict__ row, const PlantDev* __restrict__ pl, QMPC_REC_OUTCOME(const qmpc_loop_outcome* __restrict__ oc, )
    QMPC_REC_SENSE(const qmpc_sense_params* __restrict__ sense, qmpc_sense_seen* __restrict__ seen, )
    QMPC_REC_GAIT(const qmpc_gait_params* __restrict__ gait, ) int batch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0 && row) *row += 1;                         // trace row of this tick (stream order: after the last post)
  if (i >= batch) return;
  if (pl[i].status != QMPC_OK QMPC_REC_OUTCOME(|| outcome_halted(OP, oc[i]))) {
    rec[i].quat[0] = __builtin_nan("");      // (ConvexMpc's record: its first word, euler[0])
    return;
  }
#if QMPC_REC_EXT >= 5
  loop_front_sense_one<1>(LP, st[i], rec[i], sense ? sense + (size_t)i : nullptr, seen ? seen + (size_t)i : nullptr
                          QMPC_REC_GAIT(, gait ? gait + (size_t)i : nullptr));
#else
  QMPC_REC_FRONT(1, LP, st[i], rec[i]);
#endif
}
#endif

__global__ __launch_bounds__(64) void qmpc_loop_rec_post_kernel(
    qmpc_loop_params LP, QMPC_REC_OUTCOME(qmpc_outcome_params OP, ) qmpc_loop_state* __restrict__ st,
    const double* __restrict__ forces, const qmpc_info* __restrict__ info, double* __restrict__ trace_f, double* __restrict__ trace_c,
    const int* __restrict__ row, const PlantDev* __restrict__ pl, QMPC_REC_OUTCOME(qmpc_loop_outcome* __restrict__ oc, )
    QMPC_REC_PUSH(const qmpc_push_params* __restrict__ push, int per_robot, )
    QMPC_REC_GROUND(const qmpc_ground_params* __restrict__ ground, qmpc_ground_tally* __restrict__ tally, )
    QMPC_REC_ACT(const qmpc_actuation_params* __restrict__ act, qmpc_actuation_line* __restrict__ line, )
    QMPC_REC_MOTOR(LegGeom G, const qmpc_motor_params* __restrict__ motor, qmpc_motor_tally* __restrict__ mtally, ) int batch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch) return;
  const size_t slot = (trace_f || trace_c) ? (size_t)(*row) * batch + i : 0;
  double* tf = trace_f ? trace_f + 12 * slot : nullptr;
  double* tc = trace_c ? trace_c + 4 * slot : nullptr;
  if (pl[i].status != QMPC_OK) {      // frozen; an outcome record stays as it is
    loop_freeze(st[i], tf, tc);
    return;
  }
#if QMPC_REC_EXT >= 1
  qmpc_loop_outcome o = oc[i];
  if (outcome_halted(OP, o)) {        // halted: state and record untouched, a zero trace row
    loop_zero_row(tf, tc);
    return;
  }
#endif
#if QMPC_REC_EXT >= 2
  const PlantDev p = push_plant(pl[i], push + (size_t)i * per_robot, per_robot, st[i].tick);
  QMPC_REC_POST(p, LP, st[i], forces + 12 * (size_t)i, info[i], tf, tc QMPC_REC_POST_GROUND(i));
#else
  QMPC_REC_POST(pl[i], LP, st[i], forces + 12 * (size_t)i, info[i], tf, tc);
#endif
#if QMPC_REC_EXT >= 1
  qmpc_loop::loop_outcome_one(OP, st[i], o);
  oc[i] = o;
#endif
}

// ---- persistent form ---------------------------------------------------------------------------------------------------
// P is bound to Pi[b] as in qmpc_solve_w_inst_kernel (the address depends on blockIdx.x only, the reads stay scalar loads), the
// post step reads plants[b].  A frozen robot's wave writes its status and zero trace rows and leaves.  The warm start works as
// in the plain kernel (warm_t); with controller records the entry point accepts it on a handle that opted in
// (qmpc_set_loop_warm_records; the per-tick form's kernels: qmpc_wform_inst_warm.hip, qmpc_lane_inst_warm.hip).
// EXT >= 1: lane 0 holds the robot's outcome record from the first tick to the last and stores it once.  `halt` is lane 0's
// verdict after the outcome step, made uniform with a readfirstlane (all lanes are active there): the wave zero-fills the trace
// rows left and returns, which frees its SIMD slot for the next robot.  A robot halted by an earlier call leaves like a frozen
// one, its state untouched.
// EXT 2: lane 0 reads the robot's windows from global memory inside the post step of each tick: nothing of the push is live
// across the solve (variants 5 / 6 sit at their 256-register limit).
// EXT 3: lane 0's post step also reads the robot's 64 B ground record and read-modify-writes its 32 B tally, by pointer, in each
// tick -- the same rule: nothing live across the solve, no block copied.
// EXT 4: ... and reaches the robot's actuation record and delay line by pointer there: one 96 B ring slot read, one written, the
// 96 B applied read-modify-written, the ring indexed in global memory with the run-time slot number (no local array, no scratch).
// EXT 5: lane 0's FRONT step reaches the robot's 256 B sensing record and its 128 B seen by pointer (loop_front_sense_one): the 13
// true doubles it saves live across the front end's call only -- the same rule, nothing of the feature is live across the solve.
// EXT 6: ... and the robot's 128 B gait record, read inside the front end it selects -- the same rule once more.
// EXT 7: lane 0's POST step calls loop_post_motor, out of line, on the robot's 128 B motor record and 320 B tally by pointer; the
// geometry (256 B) is a kernel argument -- nothing of the feature is live across the solve.
// (The two zero-fill loops stay written out: as calls of one inline function they compile to other instructions.)
template <int VAR>
__global__ __launch_bounds__(64, QMPC_SOLVE_WAVES(QMPC_REC_MODEL, VAR)) void qmpc_loop_rec_fused_kernel(
    const DevParams* __restrict__ Pi, const PlantDev* __restrict__ plants, qmpc_loop_params LP, QMPC_REC_OUTCOME(qmpc_outcome_params OP, )
    qmpc_loop_state* __restrict__ st, qmpc_input* __restrict__ rec, double* __restrict__ forces, qmpc_info* __restrict__ info,
    double* __restrict__ trace_f, double* __restrict__ trace_c, QMPC_REC_OUTCOME(qmpc_loop_outcome* __restrict__ outcomes, )
    QMPC_REC_PUSH(const qmpc_push_params* __restrict__ push, int per_robot, )
    QMPC_REC_GROUND(const qmpc_ground_params* __restrict__ ground, qmpc_ground_tally* __restrict__ tally, )
    QMPC_REC_ACT(const qmpc_actuation_params* __restrict__ act, qmpc_actuation_line* __restrict__ line, )
    QMPC_REC_SENSE(const qmpc_sense_params* __restrict__ sense, qmpc_sense_seen* __restrict__ seen, )
    QMPC_REC_GAIT(const qmpc_gait_params* __restrict__ gait, )
    QMPC_REC_MOTOR(LegGeom G, const qmpc_motor_params* __restrict__ motor, qmpc_motor_tally* __restrict__ mtally, ) int ticks, int batch,
    double* __restrict__ gws) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int b = blockIdx.x;
  if (b >= batch) return;
  const int lane = threadIdx.x;
  typedef QMPC_REC_MODEL MD;
  constexpr bool PROF = false;
  constexpr int OCC = QMPC_SOLVE_WAVES(QMPC_REC_MODEL, VAR);
  const qmpc_input* in_ = rec;
  double *traj_u = nullptr, *traj_x = nullptr;
  long long* prof_out = nullptr;
  const bool frozen = plants[b].status != QMPC_OK;
  if (frozen QMPC_REC_OUTCOME(|| outcome_halted(OP, outcomes[b]))) {      // uniform: every lane reads the same words
    if (frozen && lane == 0) {
      st[b].status = (double)QMPC_BAD_PARAMS;
      st[b].iterations = 0.0;
    }
    for (int t = 0; t < ticks; ++t) {
      const size_t slot = (size_t)t * batch + b;
      if (trace_f && lane < 12) trace_f[12 * slot + lane] = 0.0;
      if (trace_c && lane < 4) trace_c[4 * slot + lane] = 0.0;
    }
    return;
  }
  const DevParams& P = Pi[b];
#if QMPC_REC_EXT >= 1
  qmpc_loop_outcome oc;
  if (lane == 0) oc = outcomes[b];
#endif
  bool prev_ok = false;
  for (int t = 0; t < ticks; ++t) {
#if QMPC_REC_EXT >= 5
    if (lane == 0)
      loop_front_sense_one<OCC>(LP, st[b], rec[b], sense ? sense + (size_t)b : nullptr, seen ? seen + (size_t)b : nullptr
                                QMPC_REC_GAIT(, gait ? gait + (size_t)b : nullptr));
#else
    if (lane == 0) QMPC_REC_FRONT(OCC, LP, st[b], rec[b]);
#endif
    __syncthreads();                      // the record (global memory) is visible to the wave
    [&]() {
      const int warm_t = (LP.warm_start != 0.0 && prev_ok) ? t : 0;   // t > 0 and the last solve left a usable U in LDS
      constexpr int WVAR = VAR;
      const int wslot = b;
      constexpr const double* resume = nullptr;
#ifdef QMPC_REC_CONVEX
#define QMPC_WMODEL WM_CONVEX
#endif
#include "qmpc_wform_body.inc"
#ifdef QMPC_REC_CONVEX
#undef QMPC_WMODEL
#endif
    }();
    __syncthreads();
    prev_ok = info[b].status == QMPC_OK || info[b].status == QMPC_MAX_ITER;   // uniform: every lane reads the same word
#if QMPC_REC_EXT >= 1
    int halt = 0;
#endif
    if (lane == 0) {
      const size_t slot = (size_t)t * batch + b;
#if QMPC_REC_EXT >= 2
      const PlantDev p = push_plant(plants[b], push + (size_t)b * per_robot, per_robot, st[b].tick);
      QMPC_REC_POST<OCC>(p, LP, st[b], forces + 12 * (size_t)b, info[b], trace_f ? trace_f + 12 * slot : nullptr,
                               trace_c ? trace_c + 4 * slot : nullptr QMPC_REC_POST_GROUND(b));
#else
      QMPC_REC_POST<OCC>(plants[b], LP, st[b], forces + 12 * (size_t)b, info[b], trace_f ? trace_f + 12 * slot : nullptr,
                               trace_c ? trace_c + 4 * slot : nullptr);
#endif
#if QMPC_REC_EXT >= 1
      qmpc_loop::loop_outcome_one(OP, st[b], oc);
      halt = outcome_halted(OP, oc) ? 1 : 0;
#endif
    }
    __syncthreads();
#if QMPC_REC_EXT >= 1
    if (__builtin_amdgcn_readfirstlane(halt)) {
      for (int u = t + 1; u < ticks; ++u) {
        const size_t slot = (size_t)u * batch + b;
        if (trace_f && lane < 12) trace_f[12 * slot + lane] = 0.0;
        if (trace_c && lane < 4) trace_c[4 * slot + lane] = 0.0;
      }
      break;
    }
#endif
  }
#if QMPC_REC_EXT >= 1
  if (lane == 0) outcomes[b] = oc;
#endif
}

#if QMPC_REC_EXT == 7 && !defined(QMPC_REC_CONVEX)
// ---- the check of the motor records and tallies (QuatMpc's unit only: it does not depend on the model) ----------------------
// One thread per robot: the verdict of the robot's record and tally (qmpc_joint::loop_motor_valid) into its plant block (a
// verdict already there stays); the tally is read, never written
__global__ __launch_bounds__(256) void qmpc_motor_check_kernel(const qmpc_motor_params* __restrict__ motor,
                                                               const qmpc_motor_tally* __restrict__ mtally, PlantDev* __restrict__ pl,
                                                               int batch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch) return;
  if (!qmpc_joint::loop_motor_valid(motor[i], mtally[i])) pl[i].status = QMPC_BAD_PARAMS;
}

__attribute__((visibility("hidden"))) hipError_t rec_motor_check_launch(hipStream_t s, const qmpc_motor_params* motor,
                                                                        const qmpc_motor_tally* mtally, void* plants, int batch) {
  hipLaunchKernelGGL(qmpc_motor_check_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, s, motor, mtally,
                     static_cast<PlantDev*>(plants), batch);
  return hipGetLastError();
}
#endif

#if QMPC_REC_EXT == 6 && !defined(QMPC_REC_CONVEX)
// ---- the check of the gait records (QuatMpc's unit only: it does not depend on the model) ----------------------------------
// One thread per robot: the verdict of the robot's gait record (qmpc_loop::loop_gait_valid, with the call's tick dt) into its
// plant block (a verdict already there stays)
__global__ __launch_bounds__(256) void qmpc_gait_check_kernel(const qmpc_gait_params* __restrict__ gait, PlantDev* __restrict__ pl,
                                                              double dt, int batch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch) return;
  if (!qmpc_loop::loop_gait_valid(gait[i], dt)) pl[i].status = QMPC_BAD_PARAMS;
}

__attribute__((visibility("hidden"))) hipError_t rec_gait_check_launch(hipStream_t s, const qmpc_gait_params* gait, void* plants,
                                                                       double dt, int batch) {
  hipLaunchKernelGGL(qmpc_gait_check_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, s, gait,
                     static_cast<PlantDev*>(plants), dt, batch);
  return hipGetLastError();
}
#endif

#if QMPC_REC_EXT == 5 && !defined(QMPC_REC_CONVEX)
// ---- the check of the sensing records (QuatMpc's unit only: it does not depend on the model) -------------------------------
// One thread per robot: the verdict of the robot's sensing record into its plant block (a verdict already there stays)
__global__ __launch_bounds__(256) void qmpc_sense_check_kernel(const qmpc_sense_params* __restrict__ sense, PlantDev* __restrict__ pl,
                                                               int batch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch) return;
  if (!qmpc_loop::loop_sense_valid(sense[i])) pl[i].status = QMPC_BAD_PARAMS;
}

__attribute__((visibility("hidden"))) hipError_t rec_sense_check_launch(hipStream_t s, const qmpc_sense_params* sense, void* plants,
                                                                        int batch) {
  hipLaunchKernelGGL(qmpc_sense_check_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, s, sense,
                     static_cast<PlantDev*>(plants), batch);
  return hipGetLastError();
}
#endif

#if QMPC_REC_EXT == 4 && !defined(QMPC_REC_CONVEX)
// ---- the check of the actuation records and delay lines (QuatMpc's unit only: it does not depend on the model) ------------
// One thread per robot: the verdict of the robot's record and of its line's count into its plant block (a verdict already there
// stays); the line is read, never written
__global__ __launch_bounds__(256) void qmpc_act_check_kernel(const qmpc_actuation_params* __restrict__ act,
                                                             const qmpc_actuation_line* __restrict__ line, PlantDev* __restrict__ pl,
                                                             int batch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch) return;
  if (!qmpc_loop::loop_actuation_valid(act[i], line[i])) pl[i].status = QMPC_BAD_PARAMS;
}

__attribute__((visibility("hidden"))) hipError_t rec_act_check_launch(hipStream_t s, const qmpc_actuation_params* act,
                                                                      const qmpc_actuation_line* line, void* plants, int batch) {
  hipLaunchKernelGGL(qmpc_act_check_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, s, act, line,
                     static_cast<PlantDev*>(plants), batch);
  return hipGetLastError();
}
#endif

#if QMPC_REC_EXT == 3 && !defined(QMPC_REC_CONVEX)
// ---- the check of the ground records (QuatMpc's unit only: it does not depend on the model) -------------------------------
// One thread per robot: the verdict of the robot's ground record into its plant block (a verdict already there stays)
__global__ __launch_bounds__(256) void qmpc_ground_check_kernel(const qmpc_ground_params* __restrict__ ground, PlantDev* __restrict__ pl,
                                                                int batch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch) return;
  if (!qmpc_loop::loop_ground_valid(ground[i])) pl[i].status = QMPC_BAD_PARAMS;
}

__attribute__((visibility("hidden"))) hipError_t rec_ground_check_launch(hipStream_t s, const qmpc_ground_params* ground, void* plants,
                                                                         int batch) {
  hipLaunchKernelGGL(qmpc_ground_check_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, s, ground,
                     static_cast<PlantDev*>(plants), batch);
  return hipGetLastError();
}
#endif

// ---- launchers (host; called from qmpc_hip.hip; hidden: not part of the C ABI) ------------------------------------------------
// the launch table of this unit: the persistent kernels by wrench-form variant 3 / 5 / 6 (qmpc_kernel_slots.h: wform_index)
static decltype(&qmpc_loop_rec_fused_kernel<3>) const kRecFused[] = {qmpc_loop_rec_fused_kernel<3>, qmpc_loop_rec_fused_kernel<5>, qmpc_loop_rec_fused_kernel<6>};
static_assert(sizeof kRecFused / sizeof kRecFused[0] == qmpc::kWformVars, "qmpc_kernel_slots.h");

__attribute__((visibility("hidden"))) hipError_t rec_set_lds() { return set_max_lds(kRecFused); }

// The launchers read what their kernels take from the call's buffers L and its records r (qmpc_loop_records.h) through the
// QMPC_REC_* macros; the structs themselves go to no kernel.
// one launch for all ticks: var 3 / 5 / 6 (qmpc_plan.h: plan_loop_instances)
__attribute__((visibility("hidden"))) hipError_t rec_fused_launch(int var, size_t lds, int ticks, double* gws, const rec_launch& L,
                                                                  const loop_recs& r) {
  const int k = qmpc::wform_index(var);
  if (k < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kRecFused[k], dim3((unsigned)L.batch), dim3(kWave), lds, (hipStream_t)L.stream, static_cast<const DevParams*>(L.dev_blocks),
                     static_cast<const PlantDev*>(L.plants), *L.lp, QMPC_REC_OUTCOME(*r.op, ) L.st, L.rec, L.forces, L.info, r.trace_forces,
                     r.trace_contacts, QMPC_REC_OUTCOME(r.outcomes, ) QMPC_REC_PUSH(r.push, (int)r.per_robot, ) QMPC_REC_GROUND(r.ground, r.tally, )
                     QMPC_REC_ACT(r.act, r.line, ) QMPC_REC_SENSE(r.sense, r.seen, ) QMPC_REC_GAIT(r.gait, )
                     QMPC_REC_MOTOR(*reinterpret_cast<const LegGeom*>(r.geom), r.motor, r.mtally, ) ticks, L.batch, gws);
  return hipGetLastError();
}

#if QMPC_REC_EXT <= 1 || QMPC_REC_EXT >= 5 || defined(QMPC_REC_CONVEX)
__attribute__((visibility("hidden"))) hipError_t rec_front_launch(const rec_launch& L, const loop_recs& r) {
  hipLaunchKernelGGL(qmpc_loop_rec_front_kernel, dim3((unsigned)((L.batch + 63) / 64)), dim3(64), 0, (hipStream_t)L.stream, *L.lp,
                     QMPC_REC_OUTCOME(*r.op, ) L.st, L.rec, L.row, static_cast<const PlantDev*>(L.plants),
                     QMPC_REC_OUTCOME((const qmpc_loop_outcome*)r.outcomes, ) QMPC_REC_SENSE(r.sense, r.seen, ) QMPC_REC_GAIT(r.gait, ) L.batch);
  return hipGetLastError();
}
#endif

__attribute__((visibility("hidden"))) hipError_t rec_post_launch(const rec_launch& L, const loop_recs& r) {
  hipLaunchKernelGGL(qmpc_loop_rec_post_kernel, dim3((unsigned)((L.batch + 63) / 64)), dim3(64), 0, (hipStream_t)L.stream, *L.lp,
                     QMPC_REC_OUTCOME(*r.op, ) L.st, (const double*)L.forces, (const qmpc_info*)L.info, r.trace_forces, r.trace_contacts,
                     (const int*)L.row, static_cast<const PlantDev*>(L.plants), QMPC_REC_OUTCOME(r.outcomes, )
                     QMPC_REC_PUSH(r.push, (int)r.per_robot, ) QMPC_REC_GROUND(r.ground, r.tally, ) QMPC_REC_ACT(r.act, r.line, )
                     QMPC_REC_MOTOR(*reinterpret_cast<const LegGeom*>(r.geom), r.motor, r.mtally, ) L.batch);
  return hipGetLastError();
}

#undef QMPC_REC_OUTCOME
#undef QMPC_REC_PUSH
#undef QMPC_REC_GROUND
#undef QMPC_REC_ACT
#undef QMPC_REC_SENSE
#undef QMPC_REC_GAIT
#undef QMPC_REC_MOTOR
#ifdef QMPC_REC_MOTOR_GRF
#undef QMPC_REC_MOTOR_GRF
#endif
#ifdef QMPC_REC_FRONT_GAIT
#undef QMPC_REC_FRONT_GAIT
#endif
#undef QMPC_REC_POST_GROUND
#undef QMPC_REC_EXT
#undef QMPC_REC_MODEL
#undef QMPC_REC_FRONT
#undef QMPC_REC_POST
