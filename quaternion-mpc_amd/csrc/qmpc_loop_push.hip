// qmpc_loop_push.hip -- translation unit of libqmpc_hip.so: the closed loop with outcome records whose plant step integrates
// under timed push windows per robot (qmpc_loop_run_pushes*, include/qmpc.h; the C entry points are in qmpc_hip.hip).  The
// kernels of qmpc_loop_outcome.hip with one change, the plant block the post step is given -- qmpc_loop_rec.inc with
// QMPC_REC_EXT 2:
//   check       qmpc_push_check_kernel, once per call after the plant expansion: one thread per robot reads the robot's windows
//               and writes QMPC_BAD_PARAMS into its plant block where one has a non-finite field -- the front kernel, the
//               persistent kernel's entry and the freeze paths then treat the robot like that of an invalid plant record
//   per tick    qmpc_loop_rec_front_kernel of qmpc_loop_outcome.hip as it is (launched from there; this unit has none), then
//               qmpc_loop_rec_post_kernel, where loop_post_plant_one gets a local copy of the plant block whose force and torque
//               are the tick's effective wrench (qmpc_loop::loop_push_wrench)
//   persistent  qmpc_loop_rec_fused_kernel<3|5|6> with the same change in lane 0's post step.  Lane 0 reads the robot's
//               windows from global memory inside the post step of each tick: nothing of the push is live across the solve
//               (variants 5 / 6 sit at their 256-register limit)
// A unit of its own: every other unit compiles to the code it compiled to before.  Same flags and the same
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
#include "qmpc_loop_records.h"

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

#define QMPC_REC_EXT 2
#include "qmpc_loop_rec.inc"

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
