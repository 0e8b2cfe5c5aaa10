// qmpc_wform_inst_warm.hip -- a translation unit of libqmpc_hip.so of its own: the warm-started solve with per-instance robot
// and cost parameters, the tick a closed loop with controller records repeats under lp->warm_start in the per-tick form
// (qmpc_set_loop_warm_records; include/qmpc.h).  qmpc_solve_w_inst_kernel (qmpc_wform.hip: P bound to the instance's expanded
// block, the rejected record's early exit) with the front of qmpc_solve_warm_kernel (qmpc_loop.hip: the previous solution into
// sm[L.U], warm_t).  Same sources, same flags as qmpc_wform.hip; a unit of its own so that the kernels of every other unit keep
// their code to the byte (qmpc_kernel_slots.h).
#define QMPC_FUSED_TU 1
#define QMPC_WINST_TU qmpc_winstw_tu
#define qmpc QMPC_WINST_TU
#include "qmpc_kernels.hip"
#include "qmpc_ref.hip"
#include "qmpc_wform.h"

namespace qmpc {

// The closed loop's trace row counter back to -1 (the tick's front kernel counts it up to the row it writes).  The per-tick loops
// reset it with a 4-byte memset; inside a stream capture of the CALLER's the reset is this kernel instead, a kernel node like the
// ticks it precedes (qmpc_hip.hip: loop_setup).  Here because this unit was new with it: no other unit's code object changed.
__global__ __launch_bounds__(64) void qmpc_loop_row_reset_kernel(int* __restrict__ row) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *row = -1;
}

}  // namespace qmpc

#define QMPC_WINST_KERNEL qmpc_solve_w_inst_warm_kernel
#define QMPC_WINST_CONVEX 0
#define QMPC_WINST_WARM 1
#define QMPC_WINST_SLOT wform_inst_warm_slot
#define QMPC_WINST_SLOTS kWformInstWarmSlots
#define QMPC_WINST_SET_LDS qmpc_wform_inst_warm_set_lds
#define QMPC_WINST_LAUNCH qmpc_wform_inst_warm_launch
#include "qmpc_wform_inst_kernel.inc"

__attribute__((visibility("hidden"))) hipError_t qmpc_loop_row_reset_launch(hipStream_t s, int* row) {
  hipLaunchKernelGGL(qmpc_loop_row_reset_kernel, dim3(1), dim3(kWave), 0, s, row);
  return hipGetLastError();
}
