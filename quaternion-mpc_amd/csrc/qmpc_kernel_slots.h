// qmpc_kernel_slots.h -- the wave kernels each translation unit of libqmpc_hip.so instantiates, as slots of its launch tables
// (arrays of kernel pointers, one per argument list; qmpc_create raises the dynamic LDS limit of every entry).  A launcher turns
// the fields of a plan (qmpc_plan.h) into a slot here and launches table[slot]; -1: no such kernel, hipErrorInvalidValue.  Each
// unit static_asserts its table sizes against the counts here; tests/native/plan_host.cpp checks that every plan has a slot.
// Pure host C++.  A table lists exactly the instantiations of its unit: a kernel instantiated in an extra unit, or an extra
// kernel in a unit, changes the register allocation of its neighbours.
#pragma once

#include <cstddef>

#include "../../include/qmpc.h"

namespace qmpc {

// the wrench-form variants 3 / 5 / 6 -> 0 / 1 / 2 (qmpc_solve_w_inst_kernel, qmpc_loop_rec_fused_kernel: the slot itself)
constexpr int kWformVars = 3;
static inline int wform_index(int var) { return var == 3 ? 0 : var == 5 ? 1 : var == 6 ? 2 : -1; }
// the variants 0 1 2 3 5 6 of a body every launch form of the converged mode shares -> 0 .. 5
static inline int body_index(int var) { return var >= 0 && var <= 2 ? var : (wform_index(var) >= 0 ? 3 + wform_index(var) : -1); }

// ---- qmpc_hip.hip -------------------------------------------------------------------------------------------------------
// qmpc_solve_kernel<Model, PROF, VAR>: QuatMpc 0 1 2, ConvexMpc 0 1 2, eight points 1 2 (never everything in LDS), QuatMpc
// with its phase counters (qmpc_debug_profile) 0 1
constexpr int kDenseSolveSlots = 10;
static inline int dense_solve_slot(int model, int var, bool prof) {
  if (var < 0 || var > 2) return -1;
  if (prof) return (model == QMPC_MODEL_QUAT && var < 2) ? 8 + var : -1;
  return model == QMPC_MODEL_QUAT ? var : model == QMPC_MODEL_CONVEX ? 3 + var : (model == QMPC_MODEL_QUAT8 && var) ? 5 + var : -1;
}
// qmpc_ref_kernel<Model, VAR> (the reference mode): QuatMpc 0 1, ConvexMpc 0 1, eight points 1
constexpr int kDenseRefSlots = 5;
static inline int dense_ref_slot(int model, int var) {
  if (var < 0 || var > 1) return -1;
  return model == QMPC_MODEL_QUAT ? var : model == QMPC_MODEL_CONVEX ? 2 + var : (model == QMPC_MODEL_QUAT8 && var) ? 4 : -1;
}
// qmpc_linearize_kernel<Model>: QuatMpc, ConvexMpc
constexpr int kLinearizeSlots = 2;
static inline int linearize_slot(int model) { return model == QMPC_MODEL_QUAT ? 0 : model == QMPC_MODEL_CONVEX ? 1 : -1; }

// ---- qmpc_loop_fused.hip ------------------------------------------------------------------------------------------------
// qmpc_loop_fused_kernel<VAR, JOINT, REF, CONVEX>, for JOINT false then true: the converged mode 0 1 2 3 5 6 for QuatMpc and
// for ConvexMpc, the reference mode 0 1 3 5 for QuatMpc and 3 5 for ConvexMpc (its own mode: the wrench-form bodies only)
constexpr int kFusedSlots = 36;
static inline int fused_slot(int var, bool ref, bool convex, bool joint) {
  const int i = body_index(var);
  const int s = !ref ? (i < 0 ? -1 : (convex ? 6 : 0) + i)
                : convex ? (var == 3 || var == 5 ? 16 + wform_index(var) : -1)
                         : (var == 0 || var == 1 || var == 3 || var == 5 ? 12 + (var < 3 ? var : 2 + wform_index(var)) : -1);
  return s < 0 ? -1 : s + (joint ? 18 : 0);
}
// qmpc_solve_warm_kernel<VAR, CONVEX>: 0 1 2 3 5 6 for QuatMpc, then for ConvexMpc
constexpr int kWarmSlots = 12;
static inline int warm_slot(int var, bool convex) {
  const int i = body_index(var);
  return i < 0 ? -1 : (convex ? 6 : 0) + i;
}

// ---- qmpc_wform.hip -----------------------------------------------------------------------------------------------------
// qmpc_solve_w_kernel<PROF, WVAR> (QuatMpc, converged mode): 3 5 6, with the phase counters 3 5.  Variant 6 has no profiling
// instantiation: its profile runs the plain kernel (the counters stay zero).
constexpr int kWformQuatSlots = 5;
static inline int wform_quat_slot(int var, bool prof) {
  const int i = wform_index(var);
  return (prof && i >= 0 && i < 2) ? 3 + i : i;
}
// The reference mode's workspace form (5) of QuatMpc's and ConvexMpc's problem takes the instantiation with the whole register
// file at one instance per SIMD at most -- a small batch, or a horizon whose LDS (> 20 KB: N >= 11) leaves a CU four instances
// anyway (the 256-register instantiation spills 157 VGPRs and would gain no occupancy for it)
static inline bool wform_ref_one_wave(int batch, size_t lds) { return batch <= 1024 || lds > 20 * 1024; }
// the kernels with qmpc_solve8_w_kernel's arguments: the converged mode's qmpc_solve8_w_kernel<WVAR> 3 5 6 and
// qmpc_solve_cw_kernel<WVAR> 3 5 6; the reference mode's qmpc_ref_w_kernel<WVAR, OCC> and qmpc_ref_cw_kernel<WVAR, OCC>
// <3, 1> <5, 1> <5, 2> each, qmpc_ref8_w_kernel<WVAR, 1> 3 5 (one wave per SIMD in either form)
constexpr int kWformSlots = 14;
static inline int wform_slot(int model, bool ref, int var, bool one_wave) {
  const int i = wform_index(var);
  if (i < 0) return -1;
  if (!ref) return model == QMPC_MODEL_QUAT8 ? i : model == QMPC_MODEL_CONVEX ? 3 + i : -1;
  if (i == 2) return -1;
  if (model == QMPC_MODEL_QUAT8) return 12 + i;
  const int j = i == 0 ? 0 : (one_wave ? 1 : 2);
  return model == QMPC_MODEL_QUAT ? 6 + j : model == QMPC_MODEL_CONVEX ? 9 + j : -1;
}
// qmpc_solve_w_list_kernel<WVAR> (the straggler hand-off): 3 5
constexpr int kWformListSlots = 2;
static inline int wform_list_slot(int var) { return var == 3 || var == 5 ? wform_index(var) : -1; }

// ---- qmpc_wform_inst_list.hip -------------------------------------------------------------------------------------------
// qmpc_solve_w_list_inst_kernel<WVAR> (the hand-off of qmpc_solve_instances* on the lane kernel): 3 5
constexpr int kWformListInstSlots = 2;
static inline int wform_list_inst_slot(int var) { return wform_list_slot(var); }

// ---- qmpc_wform_inst_warm.hip -------------------------------------------------------------------------------------------
// qmpc_solve_w_inst_warm_kernel<WVAR> (the warm-started ticks of a closed loop with controller records): 3 5 6
constexpr int kWformInstWarmSlots = 3;
static inline int wform_inst_warm_slot(int var) { return wform_index(var); }

// ---- qmpc_wform_cinst.hip -----------------------------------------------------------------------------------------------
// qmpc_solve_cw_inst_kernel<WVAR> (qmpc_convex_solve_instances*: ConvexMpc's problem with per-instance parameters): 3 5 6
constexpr int kWformConvexInstSlots = 3;
static inline int wform_convex_inst_slot(int var) { return wform_index(var); }

// ---- qmpc_wform_cinst_warm.hip ------------------------------------------------------------------------------------------
// qmpc_solve_cw_inst_warm_kernel<WVAR> (the warm-started ticks of a ConvexMpc closed loop with controller records): 3 5 6
constexpr int kWformConvexInstWarmSlots = 3;
static inline int wform_convex_inst_warm_slot(int var) { return wform_index(var); }

// ---- qmpc_wform_sched.hip -----------------------------------------------------------------------------------------------
// qmpc_solve_w_sched_kernel<WVAR> (qmpc_solve_schedule*: QuatMpc's problem with a contact schedule over the horizon): 3 5 6
constexpr int kWformSchedSlots = 3;
static inline int wform_sched_slot(int var) { return wform_index(var); }

}  // namespace qmpc
