// qmpc_loop_inst.hip -- fifth translation unit of libqmpc_hip.so: the closed loop with per-robot controller and plant
// records (qmpc_loop_run_instances*, include/qmpc.h; the C entry points are in qmpc_hip.hip).
//   expansion   qmpc_expand_plants_kernel: one thread per robot, the plant record (or the controller's robot) -> PlantDev
//               with the robot's verdict; where the controller records are absent, the handle's DevParams broadcast too
//   persistent  qmpc_loop_rec_fused_kernel<3|5|6>: qmpc_loop_fused_kernel's QuatMpc wrench-form path with P bound to the
//               robot's expanded block and the post step reading its plant block
//   per tick    qmpc_loop_rec_front_kernel / qmpc_loop_rec_post_kernel around the solve the C entry point launches
// The loop's kernels and their launchers are qmpc_loop_rec.inc with QMPC_REC_EXT 0: the definition this unit shares with
// qmpc_loop_outcome.hip and qmpc_loop_push.hip.  They live in a unit of their own so that the other units compile to the code
// they compiled to before (a second user of the solve body beside qmpc_loop_fused_kernel could change the compiler's choices
// there).  Same flags as qmpc_loop_fused.hip, and the same per-robot functions in both launch forms: the two forms give the
// same bits.
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
#include "qmpc_loop_records.h"

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

#define QMPC_REC_EXT 0
#include "qmpc_loop_rec.inc"

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
