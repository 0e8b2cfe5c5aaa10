// qmpc_loop_outcome.hip -- translation unit of libqmpc_hip.so: the closed loop with per-robot records that also accumulates a
// 128-byte outcome record per robot inside the tick (qmpc_loop_run_outcomes*, include/qmpc.h; the C entry points are in
// qmpc_hip.hip).  The kernels of qmpc_loop_inst.hip with the outcome step after the post step:
//   expansion   qmpc_expand_base_plants_kernel: the call without records -- every robot's plant block from the handle's
//               DevParams (the records given go through qmpc_loop_inst.hip's expansion)
//   persistent  qmpc_loop_fused_outcome_kernel<3|5|6>: qmpc_loop_fused_inst_kernel; the lane that runs the post step keeps the
//               robot's record in a local copy across all ticks and writes it once; under stop_when_down a robot that goes down
//               zero-fills its remaining trace rows and its wavefront leaves
//   per tick    qmpc_loop_front_outcome_kernel / qmpc_loop_post_outcome_kernel: a halted robot's input record gets the NaN
//               attitude of a frozen robot (every solve kernel rejects it before its first iteration), the post kernel skips it
// New kernels in a unit of their own, not template arguments of the existing ones: every existing unit compiles to the code it
// compiled to before.  Same flags as qmpc_loop_inst.hip and the same per-robot functions (loop_front_one, the solve body,
// loop_post_plant_one): states and traces are those of qmpc_loop_run_instances*, bit for bit.  The outcome step
// (qmpc_loop::loop_outcome_one) is exact IEEE arithmetic with contraction off -- compares, adds, products, one square root --
// so the two launch forms give the same record whatever the compiler inlines where.
#define QMPC_FUSED_TU 1
#define qmpc qmpc_outc_tu
#include "qmpc_kernels.hip"
#include "qmpc_joint.hip"
#include "qmpc_ref.hip"
#include "qmpc_loop.hip"
#undef qmpc

#include <cmath>
#include <cstring>

#include "qmpc_kernel_slots.h"

namespace qmpc_outc_tu {

// One thread per robot: the plant block of a robot without records -- the handle's mass and inverse inertia (the bits the plain
// loop's plant step reads), no disturbance -- and, for the persistent kernel, the handle's DevParams per robot (bcast or null)
__global__ __launch_bounds__(256) void qmpc_expand_base_plants_kernel(DevParams base, DevParams* __restrict__ bcast,
                                                                      PlantDev* __restrict__ out, int batch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch) return;
  PlantDev d;
  d.mass = base.mass;
  for (int a = 0; a < 9; ++a) d.Iinv[a] = base.Iinv[a];
  for (int a = 0; a < 3; ++a) { d.force[a] = 0.0; d.torque[a] = 0.0; }
  d.status = QMPC_OK;
  d.pad_ = 0;
  out[i] = d;
  if (bcast) bcast[i] = base;
}

// the robot of record o is halted: it went down in an earlier tick (or call) and the caller asked to stop such robots
__device__ inline bool outcome_halted(const qmpc_outcome_params& OP, const qmpc_loop_outcome& o) {
  return OP.stop_when_down != 0.0 && o.down_tick >= 0.0;
}

// ---- per-tick form -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void qmpc_loop_front_outcome_kernel(qmpc_loop_params LP, qmpc_outcome_params OP,
                                                                     qmpc_loop_state* __restrict__ st, qmpc_input* __restrict__ rec,
                                                                     int* __restrict__ row, const PlantDev* __restrict__ pl,
                                                                     const qmpc_loop_outcome* __restrict__ oc, int batch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0 && row) *row += 1;                         // trace row of this tick (stream order: after the last post)
  if (i >= batch) return;
  if (pl[i].status != QMPC_OK || outcome_halted(OP, oc[i])) {
    rec[i].quat[0] = __builtin_nan("");
    return;
  }
  loop_front_one(LP, st[i], rec[i]);
}

__global__ __launch_bounds__(64) void qmpc_loop_post_outcome_kernel(qmpc_loop_params LP, qmpc_outcome_params OP,
                                                                    qmpc_loop_state* __restrict__ st, const double* __restrict__ forces,
                                                                    const qmpc_info* __restrict__ info, double* __restrict__ trace_f,
                                                                    double* __restrict__ trace_c, const int* __restrict__ row,
                                                                    const PlantDev* __restrict__ pl, qmpc_loop_outcome* __restrict__ oc,
                                                                    int batch) {
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
  loop_post_plant_one(pl[i], LP, st[i], forces + 12 * (size_t)i, info[i], tf, tc);
  qmpc_loop::loop_outcome_one(OP, st[i], o);
  oc[i] = o;
}

// ---- persistent form ---------------------------------------------------------------------------------------------------
// qmpc_loop_fused_inst_kernel (qmpc_loop_inst.hip) with the outcome step: lane 0 holds the robot's record from the first tick
// to the last and stores it once.  `halt` is lane 0's verdict after the outcome step, made uniform with a readfirstlane (all
// lanes are active there): the wave zero-fills the trace rows left and returns, which frees its SIMD slot for the next robot.
template <int VAR>
__global__ __launch_bounds__(64, QMPC_SOLVE_WAVES(QuatModel, VAR)) void qmpc_loop_fused_outcome_kernel(
    const DevParams* __restrict__ Pi, const PlantDev* __restrict__ plants, qmpc_loop_params LP, qmpc_outcome_params OP,
    qmpc_loop_state* __restrict__ st, qmpc_input* __restrict__ rec, double* __restrict__ forces, qmpc_info* __restrict__ info,
    double* __restrict__ trace_f, double* __restrict__ trace_c, qmpc_loop_outcome* __restrict__ outcomes, int ticks, int batch,
    double* __restrict__ gws) {
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
      loop_post_plant_one<OCC>(plants[b], LP, st[b], forces + 12 * (size_t)b, info[b], trace_f ? trace_f + 12 * slot : nullptr,
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

}  // namespace qmpc_outc_tu

using namespace qmpc_outc_tu;
using namespace qmpc;

// called from qmpc_hip.hip (declared there); hidden: not part of the C ABI
__attribute__((visibility("hidden"))) hipError_t qmpc_loop_outcome_expand_base_launch(hipStream_t s, const void* dev_params,
                                                                                      size_t dev_params_size, void* bcast_out,
                                                                                      void* plants_out, int batch) {
  if (dev_params_size != sizeof(DevParams)) return hipErrorInvalidValue;
  DevParams P;
  std::memcpy(&P, dev_params, sizeof P);
  hipLaunchKernelGGL(qmpc_expand_base_plants_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, s, P,
                     static_cast<DevParams*>(bcast_out), static_cast<PlantDev*>(plants_out), batch);
  return hipGetLastError();
}

// the launch table of this unit: the persistent kernels by wrench-form variant 3 / 5 / 6 (qmpc_kernel_slots.h: wform_index)
static decltype(&qmpc_loop_fused_outcome_kernel<3>) const kLoopOutcome[] = {
    qmpc_loop_fused_outcome_kernel<3>, qmpc_loop_fused_outcome_kernel<5>, qmpc_loop_fused_outcome_kernel<6>};
static_assert(sizeof kLoopOutcome / sizeof kLoopOutcome[0] == kWformVars, "qmpc_kernel_slots.h");

__attribute__((visibility("hidden"))) hipError_t qmpc_loop_outcome_set_lds() { return set_max_lds(kLoopOutcome); }

// one launch for all ticks: var 3 / 5 / 6 (qmpc_plan.h: plan_loop_instances)
__attribute__((visibility("hidden"))) hipError_t qmpc_loop_outcome_fused_launch(
    int var, int batch, size_t lds, hipStream_t s, const void* dev_blocks, const void* plants, const qmpc_loop_params* lp,
    const qmpc_outcome_params* op, qmpc_loop_state* st, qmpc_input* rec, double* forces, qmpc_info* info, double* trace_f,
    double* trace_c, qmpc_loop_outcome* outcomes, int ticks, double* gws) {
  const int k = wform_index(var);
  if (k < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kLoopOutcome[k], dim3((unsigned)batch), dim3(kWave), lds, s, static_cast<const DevParams*>(dev_blocks),
                     static_cast<const PlantDev*>(plants), *lp, *op, st, rec, forces, info, trace_f, trace_c, outcomes, ticks, batch,
                     gws);
  return hipGetLastError();
}

__attribute__((visibility("hidden"))) hipError_t qmpc_loop_outcome_front_launch(hipStream_t s, const qmpc_loop_params* lp,
                                                                                const qmpc_outcome_params* op, qmpc_loop_state* st,
                                                                                qmpc_input* rec, int* row, const void* plants,
                                                                                const qmpc_loop_outcome* outcomes, int batch) {
  hipLaunchKernelGGL(qmpc_loop_front_outcome_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, s, *lp, *op, st, rec, row,
                     static_cast<const PlantDev*>(plants), outcomes, batch);
  return hipGetLastError();
}

__attribute__((visibility("hidden"))) hipError_t qmpc_loop_outcome_post_launch(hipStream_t s, const qmpc_loop_params* lp,
                                                                               const qmpc_outcome_params* op, qmpc_loop_state* st,
                                                                               const double* forces, const qmpc_info* info,
                                                                               double* trace_f, double* trace_c, const int* row,
                                                                               const void* plants, qmpc_loop_outcome* outcomes,
                                                                               int batch) {
  hipLaunchKernelGGL(qmpc_loop_post_outcome_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, s, *lp, *op, st, forces, info,
                     trace_f, trace_c, row, static_cast<const PlantDev*>(plants), outcomes, batch);
  return hipGetLastError();
}
