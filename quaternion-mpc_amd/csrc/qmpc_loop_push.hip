// qmpc_loop_push.hip -- translation unit of libqmpc_hip.so: the closed loop with outcome records whose plant step integrates
// under timed push windows per robot (qmpc_loop_run_pushes*, include/qmpc.h; the C entry points are in qmpc_hip.hip).  The
// kernels of qmpc_loop_outcome.hip with one change, the plant block the post step is given:
//   check       qmpc_push_check_kernel, once per call after the plant expansion: one thread per robot reads the robot's windows
//               and writes QMPC_BAD_PARAMS into its plant block where one has a non-finite field -- the front kernel, the
//               persistent kernel's entry and the freeze paths then treat the robot like that of an invalid plant record
//   per tick    qmpc_loop_front_outcome_kernel of qmpc_loop_outcome.hip as it is (launched from there), then
//               qmpc_loop_post_push_kernel: qmpc_loop_post_outcome_kernel, where loop_post_plant_one gets a local copy of the
//               plant block whose force and torque are the tick's effective wrench (qmpc_loop::loop_push_wrench)
//   persistent  qmpc_loop_fused_push_kernel<3|5|6>: qmpc_loop_fused_outcome_kernel with the same change in lane 0's post step.
//               Lane 0 reads the robot's windows from global memory inside the post step of each tick: nothing of the push is
//               live across the solve (variants 5 / 6 sit at their 256-register limit)
// New kernels in a unit of their own: every existing unit compiles to the code it compiled to before.  Same flags and the same
// per-robot functions as qmpc_loop_outcome.hip; loop_push_wrench is compares, selections and single IEEE adds with contraction
// off, so windows that never act hand loop_post_plant_one the bytes of the plant block and the results are those of
// qmpc_loop_run_outcomes*, bit for bit, in both launch forms.
#define QMPC_FUSED_TU 1
#define qmpc qmpc_push_tu
#include "qmpc_kernels.hip"
#include "qmpc_joint.hip"
#include "qmpc_ref.hip"
#include "qmpc_loop.hip"
#undef qmpc

#include <cmath>
#include <cstring>

#include "qmpc_kernel_slots.h"

namespace qmpc_push_tu {

// One thread per robot: the verdict of the robot's windows into its plant block (a verdict already there stays)
__global__ __launch_bounds__(256) void qmpc_push_check_kernel(const qmpc_push_params* __restrict__ push, int per_robot,
                                                              PlantDev* __restrict__ pl, int batch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch) return;
  const qmpc_push_params* w = push + (size_t)i * per_robot;
  bool ok = true;
  for (int k = 0; k < per_robot; ++k) ok = qmpc_loop::loop_push_valid(w[k]) && ok;
  if (!ok) pl[i].status = QMPC_BAD_PARAMS;
}

// the robot of record o is halted (qmpc_loop_outcome.hip: outcome_halted)
__device__ inline bool outcome_halted(const qmpc_outcome_params& OP, const qmpc_loop_outcome& o) {
  return OP.stop_when_down != 0.0 && o.down_tick >= 0.0;
}

// the robot's plant block with the effective wrench of the tick that starts at state.tick = t
__device__ inline PlantDev push_plant(const PlantDev& pl, const qmpc_push_params* __restrict__ w, int per_robot, double t) {
  PlantDev p = pl;
  qmpc_loop::loop_push_wrench(w, per_robot, t, p.force, p.torque);
  return p;
}

// ---- per-tick form -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void qmpc_loop_post_push_kernel(qmpc_loop_params LP, qmpc_outcome_params OP,
                                                                 qmpc_loop_state* __restrict__ st, const double* __restrict__ forces,
                                                                 const qmpc_info* __restrict__ info, double* __restrict__ trace_f,
                                                                 double* __restrict__ trace_c, const int* __restrict__ row,
                                                                 const PlantDev* __restrict__ pl, qmpc_loop_outcome* __restrict__ oc,
                                                                 const qmpc_push_params* __restrict__ push, int per_robot, int batch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch) return;
  const size_t slot = (trace_f || trace_c) ? (size_t)(*row) * batch + i : 0;
  double* tf = trace_f ? trace_f + 12 * slot : nullptr;
  double* tc = trace_c ? trace_c + 4 * slot : nullptr;
  if (pl[i].status != QMPC_OK) {      // frozen (qmpc_loop_inst.hip: loop_freeze); the outcome record stays as it is
    st[i].status = (double)QMPC_BAD_PARAMS;
    st[i].iterations = 0.0;
    if (tf) for (int a = 0; a < 12; ++a) tf[a] = 0.0;
    if (tc) for (int a = 0; a < 4; ++a) tc[a] = 0.0;
    return;
  }
  qmpc_loop_outcome o = oc[i];
  if (outcome_halted(OP, o)) {        // halted: state and record untouched, a zero trace row
    if (tf) for (int a = 0; a < 12; ++a) tf[a] = 0.0;
    if (tc) for (int a = 0; a < 4; ++a) tc[a] = 0.0;
    return;
  }
  const PlantDev p = push_plant(pl[i], push + (size_t)i * per_robot, per_robot, st[i].tick);
  loop_post_plant_one(p, LP, st[i], forces + 12 * (size_t)i, info[i], tf, tc);
  qmpc_loop::loop_outcome_one(OP, st[i], o);
  oc[i] = o;
}

// ---- persistent form ---------------------------------------------------------------------------------------------------
// qmpc_loop_fused_outcome_kernel (qmpc_loop_outcome.hip) with the tick's effective wrench in lane 0's post step
template <int VAR>
__global__ __launch_bounds__(64, QMPC_SOLVE_WAVES(QuatModel, VAR)) void qmpc_loop_fused_push_kernel(
    const DevParams* __restrict__ Pi, const PlantDev* __restrict__ plants, qmpc_loop_params LP, qmpc_outcome_params OP,
    qmpc_loop_state* __restrict__ st, qmpc_input* __restrict__ rec, double* __restrict__ forces, qmpc_info* __restrict__ info,
    double* __restrict__ trace_f, double* __restrict__ trace_c, qmpc_loop_outcome* __restrict__ outcomes,
    const qmpc_push_params* __restrict__ push, int per_robot, int ticks, int batch, double* __restrict__ gws) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int b = blockIdx.x;
  if (b >= batch) return;
  const int lane = threadIdx.x;
  typedef QuatModel MD;
  constexpr bool PROF = false;
  constexpr int OCC = QMPC_SOLVE_WAVES(QuatModel, VAR);
  const qmpc_input* in_ = rec;
  double *traj_u = nullptr, *traj_x = nullptr;
  long long* prof_out = nullptr;
  const bool frozen = plants[b].status != QMPC_OK;
  if (frozen || outcome_halted(OP, outcomes[b])) {      // uniform: every lane reads the same words
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
  qmpc_loop_outcome oc;
  if (lane == 0) oc = outcomes[b];
  bool prev_ok = false;
  for (int t = 0; t < ticks; ++t) {
    if (lane == 0) loop_front_one<OCC>(LP, st[b], rec[b]);
    __syncthreads();                      // the record (global memory) is visible to the wave
    [&]() {
      const int warm_t = (LP.warm_start != 0.0 && prev_ok) ? t : 0;   // t > 0 and the last solve left a usable U in LDS
      constexpr int WVAR = VAR;
      const int wslot = b;
      constexpr const double* resume = nullptr;
#include "qmpc_wform_body.inc"
    }();
    __syncthreads();
    prev_ok = info[b].status == QMPC_OK || info[b].status == QMPC_MAX_ITER;   // uniform: every lane reads the same word
    int halt = 0;
    if (lane == 0) {
      const size_t slot = (size_t)t * batch + b;
      // the windows are read here, in every tick: nothing of the push stays live across the solve
      const PlantDev p = push_plant(plants[b], push + (size_t)b * per_robot, per_robot, st[b].tick);
      loop_post_plant_one<OCC>(p, LP, st[b], forces + 12 * (size_t)b, info[b], trace_f ? trace_f + 12 * slot : nullptr,
                               trace_c ? trace_c + 4 * slot : nullptr);
      qmpc_loop::loop_outcome_one(OP, st[b], oc);
      halt = outcome_halted(OP, oc) ? 1 : 0;
    }
    __syncthreads();
    if (__builtin_amdgcn_readfirstlane(halt)) {
      for (int u = t + 1; u < ticks; ++u) {
        const size_t slot = (size_t)u * batch + b;
        if (trace_f && lane < 12) trace_f[12 * slot + lane] = 0.0;
        if (trace_c && lane < 4) trace_c[4 * slot + lane] = 0.0;
      }
      break;
    }
  }
  if (lane == 0) outcomes[b] = oc;
}

}  // namespace qmpc_push_tu

using namespace qmpc_push_tu;
using namespace qmpc;

// called from qmpc_hip.hip (declared there); hidden: not part of the C ABI
__attribute__((visibility("hidden"))) hipError_t qmpc_loop_push_check_launch(hipStream_t s, const qmpc_push_params* push, int per_robot,
                                                                             void* plants, int batch) {
  hipLaunchKernelGGL(qmpc_push_check_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, s, push, per_robot,
                     static_cast<PlantDev*>(plants), batch);
  return hipGetLastError();
}

// the launch table of this unit: the persistent kernels by wrench-form variant 3 / 5 / 6 (qmpc_kernel_slots.h: wform_index)
static decltype(&qmpc_loop_fused_push_kernel<3>) const kLoopPush[] = {
    qmpc_loop_fused_push_kernel<3>, qmpc_loop_fused_push_kernel<5>, qmpc_loop_fused_push_kernel<6>};
static_assert(sizeof kLoopPush / sizeof kLoopPush[0] == kWformVars, "qmpc_kernel_slots.h");

__attribute__((visibility("hidden"))) hipError_t qmpc_loop_push_set_lds() { return set_max_lds(kLoopPush); }

// one launch for all ticks: var 3 / 5 / 6 (qmpc_plan.h: plan_loop_instances)
__attribute__((visibility("hidden"))) hipError_t qmpc_loop_push_fused_launch(
    int var, int batch, size_t lds, hipStream_t s, const void* dev_blocks, const void* plants, const qmpc_loop_params* lp,
    const qmpc_outcome_params* op, qmpc_loop_state* st, qmpc_input* rec, double* forces, qmpc_info* info, double* trace_f,
    double* trace_c, qmpc_loop_outcome* outcomes, const qmpc_push_params* push, int per_robot, int ticks, double* gws) {
  const int k = wform_index(var);
  if (k < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kLoopPush[k], dim3((unsigned)batch), dim3(kWave), lds, s, static_cast<const DevParams*>(dev_blocks),
                     static_cast<const PlantDev*>(plants), *lp, *op, st, rec, forces, info, trace_f, trace_c, outcomes, push, per_robot,
                     ticks, batch, gws);
  return hipGetLastError();
}

__attribute__((visibility("hidden"))) hipError_t qmpc_loop_push_post_launch(hipStream_t s, const qmpc_loop_params* lp,
                                                                            const qmpc_outcome_params* op, qmpc_loop_state* st,
                                                                            const double* forces, const qmpc_info* info, double* trace_f,
                                                                            double* trace_c, const int* row, const void* plants,
                                                                            qmpc_loop_outcome* outcomes, const qmpc_push_params* push,
                                                                            int per_robot, int batch) {
  hipLaunchKernelGGL(qmpc_loop_post_push_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, s, *lp, *op, st, forces, info,
                     trace_f, trace_c, row, static_cast<const PlantDev*>(plants), outcomes, push, per_robot, batch);
  return hipGetLastError();
}
