// Host-only check of loop_recs_normalise (quaternion-mpc_amd/csrc/qmpc_loop_records.h): which call a closed-loop entry point with
// per-robot records makes with the arguments its caller gave.  The oracle is the delegation cascade the fourteen entry points
// qmpc_loop_run_{instances,outcomes,pushes,ground,actuation,sensing,gaits,motors}[_device] were before there was one record:
// every level written out below as it stood in qmpc_hip.hip -- `if (!x) return lower(...)`, its refusals, the dependent pointers
// it nulled on the way down -- ending in the pointer checks of the path it called.  The arguments that play no part in the choice
// (handle, loop parameters, states, ticks, traces, stream) are left out: they passed through unchanged and were checked after.
// Enumerated: the eight entry kinds, both chains (device buffers, host buffers), every presence combination of the pointers an
// entry point takes (ctrl, plant, op, outcomes, push, ground, tally, act, line, sense, seen, gait, motor, mtally; geom given and
// NULL), pushes_per_robot 0, 1, QMPC_MAX_PUSHES and QMPC_MAX_PUSHES + 1, batch 0 and 2.  Compared: the status, the call's kind and
// every argument after the nulling.  Prints a summary and `passed: 0 failures`; exit status 0 when nothing failed.
#include "../../quaternion-mpc_amd/csrc/qmpc_loop_records.h"

#include <cstdio>
#include <cstring>

namespace {

int32_t g_batch;               // the batch of the call under enumeration
qmpc_leg_geometry g_go1;       // stands for the caller's copy of the Go1 geometry

// what the cascade ended in: the status of the pointer checks and, where they pass, the call that was made
struct Call {
  qmpc_status status;
  int kind;
  loop_recs r;
};
Call refuse() {
  Call c;
  std::memset(&c, 0, sizeof c);
  c.status = QMPC_BAD_ARGUMENT;
  return c;
}

// ---- the oracle: the parent revision's cascade -----------------------------------------------------------------------------------
struct loop_motor_args {
  const qmpc_leg_geometry* geom;
  const qmpc_motor_params* motor;
  qmpc_motor_tally* tally;
};

// the pointer checks at the head of loop_records_device and its per_robot = 0 without windows; then the call is made
Call loop_records_device(int kind, const qmpc_instance_params* d_ctrl, const qmpc_plant_params* d_plant, const qmpc_outcome_params* op,
                         qmpc_loop_outcome* d_outcomes, const qmpc_push_params* d_push, int32_t per_robot, const qmpc_ground_params* d_ground,
                         qmpc_ground_tally* d_tally, const qmpc_actuation_params* d_act, qmpc_actuation_line* d_line,
                         const qmpc_sense_params* d_sense, qmpc_sense_seen* d_seen, const qmpc_gait_params* d_gait,
                         const loop_motor_args* mo = nullptr) {
  const int32_t batch = g_batch;
  if ((kind == REC_MOTOR) != (mo != nullptr) || (mo && (!mo->geom || (batch > 0 && (!mo->motor || !mo->tally))))) return refuse();
  if (kind != REC_PLAIN && (!op || (batch > 0 && !d_outcomes))) return refuse();
  if (!d_push) {
    d_push = nullptr;
    per_robot = 0;
  }
  Call c;
  c.status = QMPC_OK;
  c.kind = kind;
  c.r = loop_recs{d_ctrl, d_plant, nullptr, nullptr, op, d_outcomes, d_push, per_robot, d_ground, d_tally, d_act, d_line, d_sense, d_seen, d_gait,
                  mo ? mo->geom : nullptr, mo ? mo->motor : nullptr, mo ? mo->tally : nullptr};
  return c;
}

Call instances_device(const qmpc_instance_params* d_ctrl, const qmpc_plant_params* d_plant) {
  return loop_records_device(REC_PLAIN, d_ctrl, d_plant, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

Call outcomes_device(const qmpc_instance_params* d_ctrl, const qmpc_plant_params* d_plant, const qmpc_outcome_params* op,
                     qmpc_loop_outcome* d_outcomes) {
  return loop_records_device(REC_OUTCOME, d_ctrl, d_plant, op, d_outcomes, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

Call pushes_device(const qmpc_instance_params* d_ctrl, const qmpc_plant_params* d_plant, const qmpc_outcome_params* op,
                   qmpc_loop_outcome* d_outcomes, const qmpc_push_params* d_push, int32_t pushes_per_robot) {
  if (!d_push) return outcomes_device(d_ctrl, d_plant, op, d_outcomes);
  if (pushes_per_robot < 1 || pushes_per_robot > QMPC_MAX_PUSHES) return refuse();
  return loop_records_device(REC_PUSH, d_ctrl, d_plant, op, d_outcomes, d_push, pushes_per_robot, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                             nullptr);
}

Call ground_device(const qmpc_instance_params* d_ctrl, const qmpc_plant_params* d_plant, const qmpc_outcome_params* op,
                   qmpc_loop_outcome* d_outcomes, const qmpc_push_params* d_push, int32_t pushes_per_robot, const qmpc_ground_params* d_ground,
                   qmpc_ground_tally* d_tally) {
  if (!d_ground) return pushes_device(d_ctrl, d_plant, op, d_outcomes, d_push, pushes_per_robot);
  if (d_push && (pushes_per_robot < 1 || pushes_per_robot > QMPC_MAX_PUSHES)) return refuse();
  return loop_records_device(REC_GROUND, d_ctrl, d_plant, op, d_outcomes, d_push, d_push ? pushes_per_robot : 0, d_ground, d_tally, nullptr, nullptr,
                             nullptr, nullptr, nullptr);
}

Call actuation_device(const qmpc_instance_params* d_ctrl, const qmpc_plant_params* d_plant, const qmpc_outcome_params* op,
                      qmpc_loop_outcome* d_outcomes, const qmpc_push_params* d_push, int32_t pushes_per_robot, const qmpc_ground_params* d_ground,
                      qmpc_ground_tally* d_tally, const qmpc_actuation_params* d_act, qmpc_actuation_line* d_line) {
  if (!d_act) return ground_device(d_ctrl, d_plant, op, d_outcomes, d_push, pushes_per_robot, d_ground, d_tally);
  if (!d_line) return refuse();
  if (d_push && (pushes_per_robot < 1 || pushes_per_robot > QMPC_MAX_PUSHES)) return refuse();
  return loop_records_device(REC_ACT, d_ctrl, d_plant, op, d_outcomes, d_push, d_push ? pushes_per_robot : 0, d_ground, d_ground ? d_tally : nullptr,
                             d_act, d_line, nullptr, nullptr, nullptr);
}

Call sensing_device(const qmpc_instance_params* d_ctrl, const qmpc_plant_params* d_plant, const qmpc_outcome_params* op,
                    qmpc_loop_outcome* d_outcomes, const qmpc_push_params* d_push, int32_t pushes_per_robot, const qmpc_ground_params* d_ground,
                    qmpc_ground_tally* d_tally, const qmpc_actuation_params* d_act, qmpc_actuation_line* d_line,
                    const qmpc_sense_params* d_sense, qmpc_sense_seen* d_seen) {
  if (!d_sense) return actuation_device(d_ctrl, d_plant, op, d_outcomes, d_push, pushes_per_robot, d_ground, d_tally, d_act, d_line);
  if (d_act && !d_line) return refuse();
  if (d_push && (pushes_per_robot < 1 || pushes_per_robot > QMPC_MAX_PUSHES)) return refuse();
  return loop_records_device(REC_SENSE, d_ctrl, d_plant, op, d_outcomes, d_push, d_push ? pushes_per_robot : 0, d_ground, d_ground ? d_tally : nullptr,
                             d_act, d_act ? d_line : nullptr, d_sense, d_seen, nullptr);
}

Call gaits_device(const qmpc_instance_params* d_ctrl, const qmpc_plant_params* d_plant, const qmpc_outcome_params* op,
                  qmpc_loop_outcome* d_outcomes, const qmpc_push_params* d_push, int32_t pushes_per_robot, const qmpc_ground_params* d_ground,
                  qmpc_ground_tally* d_tally, const qmpc_actuation_params* d_act, qmpc_actuation_line* d_line, const qmpc_sense_params* d_sense,
                  qmpc_sense_seen* d_seen, const qmpc_gait_params* d_gait) {
  if (!d_gait) return sensing_device(d_ctrl, d_plant, op, d_outcomes, d_push, pushes_per_robot, d_ground, d_tally, d_act, d_line, d_sense, d_seen);
  if (d_act && !d_line) return refuse();
  if (d_push && (pushes_per_robot < 1 || pushes_per_robot > QMPC_MAX_PUSHES)) return refuse();
  return loop_records_device(REC_GAIT, d_ctrl, d_plant, op, d_outcomes, d_push, d_push ? pushes_per_robot : 0, d_ground, d_ground ? d_tally : nullptr,
                             d_act, d_act ? d_line : nullptr, d_sense, d_sense ? d_seen : nullptr, d_gait);
}

Call motors_device(const qmpc_instance_params* d_ctrl, const qmpc_plant_params* d_plant, const qmpc_outcome_params* op,
                   qmpc_loop_outcome* d_outcomes, const qmpc_push_params* d_push, int32_t pushes_per_robot, const qmpc_ground_params* d_ground,
                   qmpc_ground_tally* d_tally, const qmpc_actuation_params* d_act, qmpc_actuation_line* d_line, const qmpc_sense_params* d_sense,
                   qmpc_sense_seen* d_seen, const qmpc_gait_params* d_gait, const qmpc_leg_geometry* geom, const qmpc_motor_params* d_motor,
                   qmpc_motor_tally* d_motor_tally) {
  if (!d_motor)
    return gaits_device(d_ctrl, d_plant, op, d_outcomes, d_push, pushes_per_robot, d_ground, d_tally, d_act, d_line, d_sense, d_seen, d_gait);
  if (!d_motor_tally) return refuse();
  if (d_act && !d_line) return refuse();
  if (d_push && (pushes_per_robot < 1 || pushes_per_robot > QMPC_MAX_PUSHES)) return refuse();
  const qmpc_leg_geometry& go1 = g_go1;      // (there: a local filled by qmpc_default_go1_geometry when geom is NULL)
  const loop_motor_args mo = {geom ? geom : &go1, d_motor, d_motor_tally};
  return loop_records_device(REC_MOTOR, d_ctrl, d_plant, op, d_outcomes, d_push, d_push ? pushes_per_robot : 0, d_ground, d_ground ? d_tally : nullptr,
                             d_act, d_act ? d_line : nullptr, d_sense, d_sense ? d_seen : nullptr, d_gait, &mo);
}

// the host-buffer chain: loop_outcomes_host's pointer checks and its kind, then loop_records_host, which staged the records and
// called loop_records_device with the same presence of every pointer
Call loop_outcomes_host(const qmpc_instance_params* ctrl, const qmpc_plant_params* plant, const qmpc_outcome_params* op,
                        qmpc_loop_outcome* outcomes, const qmpc_push_params* push, int32_t per_robot, const qmpc_ground_params* ground,
                        qmpc_ground_tally* tally, const qmpc_actuation_params* act = nullptr, qmpc_actuation_line* line = nullptr,
                        const qmpc_sense_params* sense = nullptr, qmpc_sense_seen* seen = nullptr, const qmpc_gait_params* gait = nullptr,
                        const loop_motor_args* mo = nullptr) {
  const int32_t batch = g_batch;
  if (!op || (batch > 0 && !outcomes)) return refuse();
  return loop_records_device(mo ? REC_MOTOR : gait ? REC_GAIT : sense ? REC_SENSE : act ? REC_ACT : ground ? REC_GROUND : push ? REC_PUSH : REC_OUTCOME,
                             ctrl, plant, op, outcomes, push, per_robot, ground, (ground && tally) ? tally : nullptr, act, act ? line : nullptr, sense,
                             (sense && seen) ? seen : nullptr, gait, mo);
}

Call instances_host(const qmpc_instance_params* ctrl, const qmpc_plant_params* plant) {
  return loop_records_device(REC_PLAIN, ctrl, plant, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

Call outcomes_host(const qmpc_instance_params* ctrl, const qmpc_plant_params* plant, const qmpc_outcome_params* op, qmpc_loop_outcome* outcomes) {
  return loop_outcomes_host(ctrl, plant, op, outcomes, nullptr, 0, nullptr, nullptr);
}

Call pushes_host(const qmpc_instance_params* ctrl, const qmpc_plant_params* plant, const qmpc_outcome_params* op, qmpc_loop_outcome* outcomes,
                 const qmpc_push_params* push, int32_t pushes_per_robot) {
  if (!push) return outcomes_host(ctrl, plant, op, outcomes);
  if (pushes_per_robot < 1 || pushes_per_robot > QMPC_MAX_PUSHES) return refuse();
  return loop_outcomes_host(ctrl, plant, op, outcomes, push, pushes_per_robot, nullptr, nullptr);
}

Call ground_host(const qmpc_instance_params* ctrl, const qmpc_plant_params* plant, const qmpc_outcome_params* op, qmpc_loop_outcome* outcomes,
                 const qmpc_push_params* push, int32_t pushes_per_robot, const qmpc_ground_params* ground, qmpc_ground_tally* tally) {
  if (!ground) return pushes_host(ctrl, plant, op, outcomes, push, pushes_per_robot);
  if (push && (pushes_per_robot < 1 || pushes_per_robot > QMPC_MAX_PUSHES)) return refuse();
  return loop_outcomes_host(ctrl, plant, op, outcomes, push, push ? pushes_per_robot : 0, ground, tally);
}

Call actuation_host(const qmpc_instance_params* ctrl, const qmpc_plant_params* plant, const qmpc_outcome_params* op, qmpc_loop_outcome* outcomes,
                    const qmpc_push_params* push, int32_t pushes_per_robot, const qmpc_ground_params* ground, qmpc_ground_tally* tally,
                    const qmpc_actuation_params* act, qmpc_actuation_line* line) {
  if (!act) return ground_host(ctrl, plant, op, outcomes, push, pushes_per_robot, ground, tally);
  if (!line) return refuse();
  if (push && (pushes_per_robot < 1 || pushes_per_robot > QMPC_MAX_PUSHES)) return refuse();
  return loop_outcomes_host(ctrl, plant, op, outcomes, push, push ? pushes_per_robot : 0, ground, ground ? tally : nullptr, act, line);
}

Call sensing_host(const qmpc_instance_params* ctrl, const qmpc_plant_params* plant, const qmpc_outcome_params* op, qmpc_loop_outcome* outcomes,
                  const qmpc_push_params* push, int32_t pushes_per_robot, const qmpc_ground_params* ground, qmpc_ground_tally* tally,
                  const qmpc_actuation_params* act, qmpc_actuation_line* line, const qmpc_sense_params* sense, qmpc_sense_seen* seen) {
  if (!sense) return actuation_host(ctrl, plant, op, outcomes, push, pushes_per_robot, ground, tally, act, line);
  if (act && !line) return refuse();
  if (push && (pushes_per_robot < 1 || pushes_per_robot > QMPC_MAX_PUSHES)) return refuse();
  return loop_outcomes_host(ctrl, plant, op, outcomes, push, push ? pushes_per_robot : 0, ground, ground ? tally : nullptr, act, act ? line : nullptr,
                            sense, seen);
}

Call gaits_host(const qmpc_instance_params* ctrl, const qmpc_plant_params* plant, const qmpc_outcome_params* op, qmpc_loop_outcome* outcomes,
                const qmpc_push_params* push, int32_t pushes_per_robot, const qmpc_ground_params* ground, qmpc_ground_tally* tally,
                const qmpc_actuation_params* act, qmpc_actuation_line* line, const qmpc_sense_params* sense, qmpc_sense_seen* seen,
                const qmpc_gait_params* gait) {
  if (!gait) return sensing_host(ctrl, plant, op, outcomes, push, pushes_per_robot, ground, tally, act, line, sense, seen);
  if (act && !line) return refuse();
  if (push && (pushes_per_robot < 1 || pushes_per_robot > QMPC_MAX_PUSHES)) return refuse();
  return loop_outcomes_host(ctrl, plant, op, outcomes, push, push ? pushes_per_robot : 0, ground, ground ? tally : nullptr, act, act ? line : nullptr,
                            sense, sense ? seen : nullptr, gait);
}

Call motors_host(const qmpc_instance_params* ctrl, const qmpc_plant_params* plant, const qmpc_outcome_params* op, qmpc_loop_outcome* outcomes,
                 const qmpc_push_params* push, int32_t pushes_per_robot, const qmpc_ground_params* ground, qmpc_ground_tally* tally,
                 const qmpc_actuation_params* act, qmpc_actuation_line* line, const qmpc_sense_params* sense, qmpc_sense_seen* seen,
                 const qmpc_gait_params* gait, const qmpc_leg_geometry* geom, const qmpc_motor_params* motor, qmpc_motor_tally* motor_tally) {
  if (!motor) return gaits_host(ctrl, plant, op, outcomes, push, pushes_per_robot, ground, tally, act, line, sense, seen, gait);
  if (!motor_tally) return refuse();
  if (act && !line) return refuse();
  if (push && (pushes_per_robot < 1 || pushes_per_robot > QMPC_MAX_PUSHES)) return refuse();
  const qmpc_leg_geometry& go1 = g_go1;
  const loop_motor_args mo = {geom ? geom : &go1, motor, motor_tally};
  return loop_outcomes_host(ctrl, plant, op, outcomes, push, push ? pushes_per_robot : 0, ground, ground ? tally : nullptr, act, act ? line : nullptr,
                            sense, sense ? seen : nullptr, gait, &mo);
}

// the entry point of kind `entry` on the arguments a (those it takes), through the cascade
Call oracle(bool device, int entry, const loop_recs& a) {
  switch (entry) {
    case REC_PLAIN: return device ? instances_device(a.ctrl, a.plant) : instances_host(a.ctrl, a.plant);
    case REC_OUTCOME: return device ? outcomes_device(a.ctrl, a.plant, a.op, a.outcomes) : outcomes_host(a.ctrl, a.plant, a.op, a.outcomes);
    case REC_PUSH:
      return device ? pushes_device(a.ctrl, a.plant, a.op, a.outcomes, a.push, a.per_robot) : pushes_host(a.ctrl, a.plant, a.op, a.outcomes, a.push, a.per_robot);
    case REC_GROUND:
      return device ? ground_device(a.ctrl, a.plant, a.op, a.outcomes, a.push, a.per_robot, a.ground, a.tally)
                    : ground_host(a.ctrl, a.plant, a.op, a.outcomes, a.push, a.per_robot, a.ground, a.tally);
    case REC_ACT:
      return device ? actuation_device(a.ctrl, a.plant, a.op, a.outcomes, a.push, a.per_robot, a.ground, a.tally, a.act, a.line)
                    : actuation_host(a.ctrl, a.plant, a.op, a.outcomes, a.push, a.per_robot, a.ground, a.tally, a.act, a.line);
    case REC_SENSE:
      return device ? sensing_device(a.ctrl, a.plant, a.op, a.outcomes, a.push, a.per_robot, a.ground, a.tally, a.act, a.line, a.sense, a.seen)
                    : sensing_host(a.ctrl, a.plant, a.op, a.outcomes, a.push, a.per_robot, a.ground, a.tally, a.act, a.line, a.sense, a.seen);
    case REC_GAIT:
      return device ? gaits_device(a.ctrl, a.plant, a.op, a.outcomes, a.push, a.per_robot, a.ground, a.tally, a.act, a.line, a.sense, a.seen, a.gait)
                    : gaits_host(a.ctrl, a.plant, a.op, a.outcomes, a.push, a.per_robot, a.ground, a.tally, a.act, a.line, a.sense, a.seen, a.gait);
    default:
      return device ? motors_device(a.ctrl, a.plant, a.op, a.outcomes, a.push, a.per_robot, a.ground, a.tally, a.act, a.line, a.sense, a.seen, a.gait,
                                    a.geom, a.motor, a.mtally)
                    : motors_host(a.ctrl, a.plant, a.op, a.outcomes, a.push, a.per_robot, a.ground, a.tally, a.act, a.line, a.sense, a.seen, a.gait,
                                  a.geom, a.motor, a.mtally);
  }
}

// ---- the enumeration -----------------------------------------------------------------------------------------------------------------
// one object per pointer: its address stands for the caller's buffer (nothing is read through it)
qmpc_instance_params o_ctrl;
qmpc_plant_params o_plant;
qmpc_outcome_params o_op;
qmpc_loop_outcome o_outcomes;
qmpc_push_params o_push;
qmpc_ground_params o_ground;
qmpc_ground_tally o_tally;
qmpc_actuation_params o_act;
qmpc_actuation_line o_line;
qmpc_sense_params o_sense;
qmpc_sense_seen o_seen;
qmpc_gait_params o_gait;
qmpc_motor_params o_motor;
qmpc_motor_tally o_mtally;
qmpc_leg_geometry o_geom;
enum { P_CTRL, P_PLANT, P_OP, P_OUTCOMES, P_PUSH, P_GROUND, P_TALLY, P_ACT, P_LINE, P_SENSE, P_SEEN, P_GAIT, P_MOTOR, P_MTALLY, P_GEOM, P_COUNT };
// the pointers an entry point of each kind takes (bit P_x), and whether it takes pushes_per_robot
const unsigned kTakes[REC_KINDS] = {0x3, 0xF, 0x1F, 0x7F, 0x1FF, 0x7FF, 0xFFF, 0x7FFF};

// the record an entry point fills: what is in `present` and the entry point takes, NULL (0) for everything else
loop_recs fill(int entry, unsigned present, int32_t per_robot) {
  const unsigned m = present & kTakes[entry];
  auto on = [&](int bit) { return (m >> bit & 1u) != 0; };
  loop_recs r;
  std::memset(&r, 0, sizeof r);
  r.ctrl = on(P_CTRL) ? &o_ctrl : nullptr;
  r.plant = on(P_PLANT) ? &o_plant : nullptr;
  r.op = on(P_OP) ? &o_op : nullptr;
  r.outcomes = on(P_OUTCOMES) ? &o_outcomes : nullptr;
  r.push = on(P_PUSH) ? &o_push : nullptr;
  r.per_robot = entry >= REC_PUSH ? per_robot : 0;
  r.ground = on(P_GROUND) ? &o_ground : nullptr;
  r.tally = on(P_TALLY) ? &o_tally : nullptr;
  r.act = on(P_ACT) ? &o_act : nullptr;
  r.line = on(P_LINE) ? &o_line : nullptr;
  r.sense = on(P_SENSE) ? &o_sense : nullptr;
  r.seen = on(P_SEEN) ? &o_seen : nullptr;
  r.gait = on(P_GAIT) ? &o_gait : nullptr;
  r.motor = on(P_MOTOR) ? &o_motor : nullptr;
  r.mtally = on(P_MTALLY) ? &o_mtally : nullptr;
  r.geom = on(P_GEOM) ? &o_geom : nullptr;
  return r;
}

bool same(const loop_recs& a, const loop_recs& b) {
  return a.ctrl == b.ctrl && a.plant == b.plant && a.trace_forces == b.trace_forces && a.trace_contacts == b.trace_contacts && a.op == b.op &&
         a.outcomes == b.outcomes && a.push == b.push && a.per_robot == b.per_robot && a.ground == b.ground && a.tally == b.tally && a.act == b.act &&
         a.line == b.line && a.sense == b.sense && a.seen == b.seen && a.gait == b.gait && a.geom == b.geom && a.motor == b.motor &&
         a.mtally == b.mtally;
}

}  // namespace

int main() {
  long cases = 0, refused = 0, failures = 0;
  long by_kind[REC_KINDS] = {0};
  const int32_t per_robot[] = {0, 1, QMPC_MAX_PUSHES, QMPC_MAX_PUSHES + 1};
  for (int entry = 0; entry < REC_KINDS; ++entry)
    for (unsigned present = 0; present < (1u << P_COUNT); ++present) {
      if (present & ~kTakes[entry]) continue;      // (a pointer the entry point does not take: the same call as without it)
      for (int32_t ppr : per_robot) {
        if (entry < REC_PUSH && ppr != 0) continue;
        for (int32_t batch : {0, 2})
          for (int device = 0; device < 2; ++device) {
            g_batch = batch;
            const loop_recs a = fill(entry, present, ppr);
            const Call want = oracle(device != 0, entry, a);
            loop_recs r = a;
            int kind = -1;
            const qmpc_status st = loop_recs_normalise(entry, batch, &g_go1, &r, &kind);
            ++cases;
            bool ok = st == want.status;
            if (ok && st == QMPC_OK) ok = kind == want.kind && same(r, want.r);
            if (st != QMPC_OK) ++refused;
            else if (kind >= 0 && kind < REC_KINDS) ++by_kind[kind];
            if (!ok && ++failures <= 20)
              std::printf("FAIL entry %d present 0x%04x per_robot %d batch %d %s: status %d (cascade %d), kind %d (cascade %d)\n", entry, present,
                          (int)ppr, (int)batch, device ? "device" : "host", (int)st, (int)want.status, kind, want.kind);
          }
      }
    }
  std::printf("normalise against the cascade: %ld calls, %ld refused; made by kind", cases, refused);
  for (int k = 0; k < REC_KINDS; ++k) std::printf(" %ld", by_kind[k]);
  std::printf("\n");
  bool all_kinds = true;
  for (int k = 0; k < REC_KINDS; ++k) all_kinds = all_kinds && by_kind[k] > 0;
  if (!all_kinds || refused == 0) {
    std::printf("FAIL the enumeration misses a kind or every refusal\n");
    ++failures;
  }
  std::printf("passed: %ld failures\n", failures);
  return failures ? 1 : 0;
}
