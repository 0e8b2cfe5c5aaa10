// qmpc_loop_outcome.hip -- translation unit of libqmpc_hip.so: the closed loop with per-robot records that also accumulates a
// 128-byte outcome record per robot inside the tick (qmpc_loop_run_outcomes*, include/qmpc.h; the C entry points are in
// qmpc_hip.hip).  The kernels of qmpc_loop_inst.hip with the outcome step after the post step -- qmpc_loop_rec.inc with
// QMPC_REC_EXT 1:
//   expansion   qmpc_expand_base_plants_kernel: the call without records -- every robot's plant block from the handle's
//               DevParams (the records given go through qmpc_loop_inst.hip's expansion)
//   persistent  qmpc_loop_rec_fused_kernel<3|5|6>: the lane that runs the post step keeps the robot's record in a local copy
//               across all ticks and writes it once; under stop_when_down a robot that goes down zero-fills its remaining trace
//               rows and its wavefront leaves
//   per tick    qmpc_loop_rec_front_kernel / qmpc_loop_rec_post_kernel: a halted robot's input record gets the NaN attitude of
//               a frozen robot (every solve kernel rejects it before its first iteration), the post kernel skips it
// A unit of its own, not template arguments of the plain unit's kernels: every other unit compiles to the code it compiled to
// before.  Same flags as qmpc_loop_inst.hip and the same per-robot functions (loop_front_one, the solve body,
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
#include "qmpc_loop_records.h"

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

#define QMPC_REC_EXT 1
#include "qmpc_loop_rec.inc"

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
