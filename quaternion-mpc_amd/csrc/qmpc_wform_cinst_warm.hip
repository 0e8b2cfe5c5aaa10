// qmpc_wform_cinst_warm.hip -- a translation unit of libqmpc_hip.so of its own: ConvexMpc's warm-started solve with per-instance
// robot and cost parameters, the tick a closed loop with controller records repeats under lp->warm_start in the per-tick form on
// a ConvexMpc handle (qmpc_set_convex_records with qmpc_set_convex_warm_records; include/qmpc.h).  qmpc_solve_cw_inst_kernel
// (qmpc_wform_cinst.hip: P bound to the instance's expanded block, the rejected record's early exit) with the front of
// qmpc_solve_w_inst_warm_kernel (qmpc_wform_inst_warm.hip: the previous solution into sm[L.U], warm_t) -- which is that of the
// plain qmpc_solve_warm_kernel<VAR, true> (qmpc_loop.hip), so uniform records give the plain warm tick's bits.  Same sources,
// same flags as qmpc_wform.hip; a unit of its own so that the kernels of every other unit keep their code to the byte
// (qmpc_kernel_slots.h).
#define QMPC_FUSED_TU 1
#define QMPC_WINST_TU qmpc_wcinstw_tu
#define qmpc QMPC_WINST_TU
#include "qmpc_kernels.hip"
#include "qmpc_ref.hip"
#include "qmpc_wform.h"

#define QMPC_WINST_KERNEL qmpc_solve_cw_inst_warm_kernel
#define QMPC_WINST_CONVEX 1      // (ConvexMpc's state has 12 entries -- world-frame forces, Euler angles: trajectory rows of 12)
#define QMPC_WINST_WARM 1
#define QMPC_WINST_SLOT wform_convex_inst_warm_slot
#define QMPC_WINST_SLOTS kWformConvexInstWarmSlots
#define QMPC_WINST_SET_LDS qmpc_wform_cinst_warm_set_lds
#define QMPC_WINST_LAUNCH qmpc_wform_cinst_warm_launch
#include "qmpc_wform_inst_kernel.inc"
