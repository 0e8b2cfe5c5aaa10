// qmpc_loop_records.h -- the per-robot arguments of a closed-loop call with records (qmpc_loop_run_instances* ..
// qmpc_loop_run_motors*, include/qmpc.h) as ONE record, and the one place that says which call a set of arguments is.  Plain C++,
// no HIP: the entry points of qmpc_hip.hip fill a loop_recs, loop_recs_normalise() turns it into the call that is made, and both
// paths (loop_records_host, loop_records_device) and the launchers of qmpc_loop_rec.inc take it from there.  A host-only program
// can include this file (tests/native/loop_records_host.cpp).
#pragma once

#include <cstdint>

#include "../../include/qmpc.h"

// the kind of a call with records: the QMPC_REC_EXT of the unit that serves it (qmpc_loop_rec.inc), one per entry point
enum { REC_PLAIN = 0, REC_OUTCOME = 1, REC_PUSH = 2, REC_GROUND = 3, REC_ACT = 4, REC_SENSE = 5, REC_GAIT = 6, REC_MOTOR = 7, REC_KINDS = 8 };

// Everything a call with records may bring.  The same record serves host pointers (as the caller of a host-buffer entry point
// gave them) and device pointers (as the kernels read them); op and geom are host records in both.  A kind's own record is the
// const one of its group; what a call does not have is NULL (per_robot: 0).
struct loop_recs {
  const qmpc_instance_params* ctrl;
  const qmpc_plant_params* plant;
  double* trace_forces;
  double* trace_contacts;
  const qmpc_outcome_params* op;      // REC_OUTCOME and above
  qmpc_loop_outcome* outcomes;
  const qmpc_push_params* push;       // REC_PUSH and above: per_robot windows per robot
  int32_t per_robot;
  const qmpc_ground_params* ground;   // REC_GROUND and above
  qmpc_ground_tally* tally;
  const qmpc_actuation_params* act;   // REC_ACT and above
  qmpc_actuation_line* line;
  const qmpc_sense_params* sense;     // REC_SENSE and above
  qmpc_sense_seen* seen;
  const qmpc_gait_params* gait;       // REC_GAIT and above
  const qmpc_leg_geometry* geom;      // REC_MOTOR
  const qmpc_motor_params* motor;
  qmpc_motor_tally* mtally;
};

// What every launch of such a call takes beside its records: the stream, the handle's buffers and the states (device pointers;
// the launchers of qmpc_loop_rec.inc)
struct rec_launch {
  void* stream;                 // hipStream_t
  const void* dev_blocks;       // the controllers' expanded blocks [batch] DevParams (the persistent kernel only)
  const void* plants;           // the plants' expanded blocks [batch] PlantDev, with each robot's verdict
  const qmpc_loop_params* lp;   // host
  qmpc_loop_state* st;
  qmpc_input* rec;              // the tick's solve: its input records, forces and info
  double* forces;
  qmpc_info* info;
  int* row;                     // the trace row counter of the per-tick form
  int batch;
};

// The call an entry point of kind `entry` makes with the arguments *r as its caller gave them (what the entry point does not
// take: NULL): QMPC_BAD_ARGUMENT, or QMPC_OK with *kind the call's kind and *r its arguments.
//   kind       the highest kind whose own record is there (push, ground, act, sense, gait, motor): the motors
//              call without a motor record is the gaits call, and so on down to the outcome call; REC_PLAIN stays REC_PLAIN
//              (without ctrl and plant it is the plain loop: the paths see to that)
//   refused    act without line; a push with per_robot outside 1 .. QMPC_MAX_PUSHES; motor without its tally; above REC_PLAIN a
//              missing op, or missing outcomes for batch > 0
//   dropped    what belongs to a record that is not there: tally without ground, line without act, seen without sense, per_robot
//              without push, geom and mtally without motor -- and everything above the call's kind
//   geom       NULL on a motors call: go1, the caller's copy of qmpc_default_go1_geometry
// Pointers only: nothing is dereferenced, so the refusals come before anything touches the handle.
inline qmpc_status loop_recs_normalise(int entry, int32_t batch, const qmpc_leg_geometry* go1, loop_recs* r, int* kind) {
  if (r->motor && !r->mtally) return QMPC_BAD_ARGUMENT;
  if (r->act && !r->line) return QMPC_BAD_ARGUMENT;
  if (r->push && (r->per_robot < 1 || r->per_robot > QMPC_MAX_PUSHES)) return QMPC_BAD_ARGUMENT;
  if (entry != REC_PLAIN && (!r->op || (batch > 0 && !r->outcomes))) return QMPC_BAD_ARGUMENT;
  *kind = r->motor ? REC_MOTOR : r->gait ? REC_GAIT : r->sense ? REC_SENSE : r->act ? REC_ACT : r->ground ? REC_GROUND : r->push ? REC_PUSH : entry != REC_PLAIN ? REC_OUTCOME : REC_PLAIN;
  if (!r->push) r->per_robot = 0;
  if (!r->ground) r->tally = nullptr;
  if (!r->act) r->line = nullptr;
  if (!r->sense) r->seen = nullptr;
  if (!r->motor) r->mtally = nullptr;
  r->geom = !r->motor ? nullptr : r->geom ? r->geom : go1;
  return QMPC_OK;
}
