// qmpc_wform_cinst.hip -- a translation unit of libqmpc_hip.so of its own: ConvexMpc's solve with per-instance robot and cost
// parameters (qmpc_convex_solve_instances*; include/qmpc.h).  qmpc_solve_cw_kernel (qmpc_wform.hip: the wrench-form body with
// QMPC_WMODEL WM_CONVEX) with P bound to the instance's expanded block and the rejected record's early exit, as
// qmpc_solve_w_inst_kernel has them for QuatMpc's problem.  The blocks and verdicts are those of qmpc_expand_instances_kernel
// (qmpc_wform.hip): the record's fields go into the handle's DevParams whatever the model.  Same sources, same flags as
// qmpc_wform.hip; a unit of its own so that the kernels of every other unit keep their code to the byte (qmpc_kernel_slots.h).
#define QMPC_FUSED_TU 1
#define QMPC_WINST_TU qmpc_wcinst_tu
#define qmpc QMPC_WINST_TU
#include "qmpc_kernels.hip"
#include "qmpc_ref.hip"
#include "qmpc_wform.h"

#define QMPC_WINST_KERNEL qmpc_solve_cw_inst_kernel
#define QMPC_WINST_CONVEX 1      // (ConvexMpc's state has 12 entries -- world-frame forces, Euler angles: trajectory rows of 12)
#define QMPC_WINST_WARM 0
#define QMPC_WINST_SLOT wform_convex_inst_slot
#define QMPC_WINST_SLOTS kWformConvexInstSlots
#define QMPC_WINST_SET_LDS qmpc_wform_cinst_set_lds
#define QMPC_WINST_LAUNCH qmpc_wform_cinst_solve_launch
#include "qmpc_wform_inst_kernel.inc"
