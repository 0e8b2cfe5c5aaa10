// qmpc_loop_inst.hip -- fifth translation unit of libqmpc_hip.so: the closed loop with per-robot controller and plant
// records (qmpc_loop_run_instances*, include/qmpc.h; the C entry points are in qmpc_hip.hip).
//   expansion   qmpc_expand_plants_kernel: one thread per robot, the plant record (or the controller's robot) -> PlantDev
//               with the robot's verdict; where the controller records are absent, the handle's DevParams broadcast too
//   persistent  qmpc_loop_fused_inst_kernel<3|5|6>: qmpc_loop_fused_kernel's QuatMpc wrench-form path with P bound to the
//               robot's expanded block and the post step reading its plant block
//   per tick    qmpc_loop_front_inst_kernel / qmpc_loop_post_plant_kernel around the solve the C entry point launches
// The kernels live in a unit of their own so that the existing units compile to the code they compiled to before (a
// second user of the solve body beside qmpc_loop_fused_kernel could change the compiler's choices there).  Same flags as
// qmpc_loop_fused.hip, and the same per-robot functions in both launch forms: the two forms give the same bits.
#define QMPC_FUSED_TU 1
#define qmpc qmpc_inst_tu
#include "qmpc_kernels.hip"
#include "qmpc_joint.hip"
#include "qmpc_ref.hip"
#include "qmpc_loop.hip"
#undef qmpc

#include <cmath>
#include <cstring>

#include "qmpc_kernel_slots.h"

namespace qmpc_inst_tu {

// One thread per robot: the robot's plant block (from plant[i], or from ctrl[i]'s mass and inertia with no disturbance when
// plant is null; one of the two is given) and its verdict -- BAD_PARAMS where either record is invalid (ctrl_status: the verdicts of
// qmpc_expand_instances_kernel, or null).  bcast (or null): the handle's DevParams for every robot (no controller records).
__global__ __launch_bounds__(256) void qmpc_expand_plants_kernel(DevParams base, const qmpc_plant_params* __restrict__ plant,
                                                                 const qmpc_instance_params* __restrict__ ctrl,
                                                                 const int* __restrict__ ctrl_status, DevParams* __restrict__ bcast,
                                                                 PlantDev* __restrict__ out, int batch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch) return;
  qmpc_plant_params r;
  if (plant) {
    r = plant[i];
  } else {      // (the entry point passes at least one of the two)
    r.mass = ctrl[i].mass;
    for (int a = 0; a < 9; ++a) r.inertia[a] = ctrl[i].inertia[a];
    for (int a = 0; a < 3; ++a) { r.ext_force_world[a] = 0.0; r.ext_torque_body[a] = 0.0; }
  }
  PlantDev d;
  apply_plant_params(r, &d);
  if (ctrl_status && ctrl_status[i] != QMPC_OK) d.status = QMPC_BAD_PARAMS;
  out[i] = d;
  if (bcast) bcast[i] = base;
}

// A frozen robot (invalid record): its state untouched except status and iterations, its trace row of this tick zero
__device__ inline void loop_freeze(qmpc_loop_state& s, double* __restrict__ trace_f, double* __restrict__ trace_c) {
  s.status = (double)QMPC_BAD_PARAMS;
  s.iterations = 0.0;
  if (trace_f) for (int a = 0; a < 12; ++a) trace_f[a] = 0.0;
  if (trace_c) for (int a = 0; a < 4; ++a) trace_c[a] = 0.0;
}

// ---- per-tick form -----------------------------------------------------------------------------------------------------
// The front end of qmpc_loop_front_kernel; a frozen robot's record gets a NaN attitude instead, which every solve kernel
// rejects before its first iteration (QMPC_NAN_INPUT; the post kernel ignores it)
__global__ __launch_bounds__(64) void qmpc_loop_front_inst_kernel(qmpc_loop_params LP, qmpc_loop_state* __restrict__ st,
                                                                  qmpc_input* __restrict__ rec, int* __restrict__ row,
                                                                  const PlantDev* __restrict__ pl, int batch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0 && row) *row += 1;                         // trace row of this tick (stream order: after the last post)
  if (i >= batch) return;
  if (pl[i].status != QMPC_OK) {
    rec[i].quat[0] = __builtin_nan("");
    return;
  }
  loop_front_one(LP, st[i], rec[i]);
}

__global__ __launch_bounds__(64) void qmpc_loop_post_plant_kernel(qmpc_loop_params LP, qmpc_loop_state* __restrict__ st,
                                                                  const double* __restrict__ forces, const qmpc_info* __restrict__ info,
                                                                  double* __restrict__ trace_f, double* __restrict__ trace_c,
                                                                  const int* __restrict__ row, const PlantDev* __restrict__ pl,
                                                                  int batch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch) return;
  const size_t slot = (trace_f || trace_c) ? (size_t)(*row) * batch + i : 0;
  double* tf = trace_f ? trace_f + 12 * slot : nullptr;
  double* tc = trace_c ? trace_c + 4 * slot : nullptr;
  if (pl[i].status != QMPC_OK) {
    loop_freeze(st[i], tf, tc);
    return;
  }
  loop_post_plant_one(pl[i], LP, st[i], forces + 12 * (size_t)i, info[i], tf, tc);
}

// ---- persistent form ---------------------------------------------------------------------------------------------------
// qmpc_loop_fused_kernel<VAR, false, false, false> (QuatMpc's problem, converged mode, wrench-form body) with the robot's own
// controller and plant: P is bound to Pi[b] as in qmpc_solve_w_inst_kernel (the address depends on blockIdx.x only, the reads
// stay scalar loads), the post step reads plants[b].  A frozen robot's wave writes its status and zero trace rows and leaves.
// The warm start works as in the plain kernel (warm_t; the entry point refuses it with controller records, whose per-tick
// form has no warm-started kernel).
template <int VAR>
__global__ __launch_bounds__(64, QMPC_SOLVE_WAVES(QuatModel, VAR)) void qmpc_loop_fused_inst_kernel(
    const DevParams* __restrict__ Pi, const PlantDev* __restrict__ plants, qmpc_loop_params LP, qmpc_loop_state* __restrict__ st,
    qmpc_input* __restrict__ rec, double* __restrict__ forces, qmpc_info* __restrict__ info, double* __restrict__ trace_f,
    double* __restrict__ trace_c, int ticks, int batch, double* __restrict__ gws) {
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
  if (plants[b].status != QMPC_OK) {
    if (lane == 0) {
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
    if (lane == 0) {
      const size_t slot = (size_t)t * batch + b;
      loop_post_plant_one<OCC>(plants[b], LP, st[b], forces + 12 * (size_t)b, info[b], trace_f ? trace_f + 12 * slot : nullptr,
                               trace_c ? trace_c + 4 * slot : nullptr);
    }
    __syncthreads();
  }
}

}  // namespace qmpc_inst_tu

using namespace qmpc_inst_tu;
using namespace qmpc;

// called from qmpc_hip.hip (declared there); hidden: not part of the C ABI
// expand the plant records (or the controller's robots) of `batch` robots into plants_out; bcast_out (or null): the handle's
// DevParams per robot
__attribute__((visibility("hidden"))) hipError_t qmpc_loop_inst_expand_launch(hipStream_t s, const void* dev_params, size_t dev_params_size,
                                                                              const qmpc_plant_params* plant, const qmpc_instance_params* ctrl,
                                                                              const int* ctrl_status, void* bcast_out, void* plants_out,
                                                                              int batch) {
  if (dev_params_size != sizeof(DevParams)) return hipErrorInvalidValue;
  DevParams P;
  std::memcpy(&P, dev_params, sizeof P);
  hipLaunchKernelGGL(qmpc_expand_plants_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, s, P, plant, ctrl, ctrl_status,
                     static_cast<DevParams*>(bcast_out), static_cast<PlantDev*>(plants_out), batch);
  return hipGetLastError();
}

// the launch table of this unit: the persistent kernels by wrench-form variant 3 / 5 / 6 (qmpc_kernel_slots.h: wform_index)
static decltype(&qmpc_loop_fused_inst_kernel<3>) const kLoopInst[] = {qmpc_loop_fused_inst_kernel<3>, qmpc_loop_fused_inst_kernel<5>,
                                                                     qmpc_loop_fused_inst_kernel<6>};
static_assert(sizeof kLoopInst / sizeof kLoopInst[0] == kWformVars, "qmpc_kernel_slots.h");

__attribute__((visibility("hidden"))) hipError_t qmpc_loop_inst_set_lds() { return set_max_lds(kLoopInst); }

// one launch for all ticks: var 3 / 5 / 6 (qmpc_plan.h: plan_loop_instances)
__attribute__((visibility("hidden"))) hipError_t qmpc_loop_inst_fused_launch(int var, int batch, size_t lds, hipStream_t s, const void* dev_blocks,
                                                                             const void* plants, const qmpc_loop_params* lp, qmpc_loop_state* st,
                                                                             qmpc_input* rec, double* forces, qmpc_info* info, double* trace_f,
                                                                             double* trace_c, int ticks, double* gws) {
  const int k = wform_index(var);
  if (k < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kLoopInst[k], dim3((unsigned)batch), dim3(kWave), lds, s, static_cast<const DevParams*>(dev_blocks),
                     static_cast<const PlantDev*>(plants), *lp, st, rec, forces, info, trace_f, trace_c, ticks, batch, gws);
  return hipGetLastError();
}

__attribute__((visibility("hidden"))) hipError_t qmpc_loop_inst_front_launch(hipStream_t s, const qmpc_loop_params* lp, qmpc_loop_state* st,
                                                                             qmpc_input* rec, int* row, const void* plants, int batch) {
  hipLaunchKernelGGL(qmpc_loop_front_inst_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, s, *lp, st, rec, row,
                     static_cast<const PlantDev*>(plants), batch);
  return hipGetLastError();
}

__attribute__((visibility("hidden"))) hipError_t qmpc_loop_inst_post_launch(hipStream_t s, const qmpc_loop_params* lp, qmpc_loop_state* st,
                                                                            const double* forces, const qmpc_info* info, double* trace_f,
                                                                            double* trace_c, const int* row, const void* plants, int batch) {
  hipLaunchKernelGGL(qmpc_loop_post_plant_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, s, *lp, st, forces, info,
                     trace_f, trace_c, row, static_cast<const PlantDev*>(plants), batch);
  return hipGetLastError();
}
