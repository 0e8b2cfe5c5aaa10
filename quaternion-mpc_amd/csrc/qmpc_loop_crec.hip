// qmpc_loop_crec.hip -- translation unit of libqmpc_hip.so: the closed loop with per-robot records on a ConvexMpc handle
// (qmpc_loop_run_instances*, qmpc_loop_run_outcomes*, qmpc_loop_run_pushes* after qmpc_set_convex_records; include/qmpc.h, the C
// entry points are in qmpc_hip.hip).  The kernels of qmpc_loop_push.hip on the sibling controller's problem -- qmpc_loop_rec.inc
// with QMPC_REC_EXT 2 and QMPC_REC_CONVEX:
//   per tick    qmpc_loop_rec_front_kernel (loop_front_convex_one on qmpc_convex_input records; a frozen or halted robot's record
//               gets a NaN first word), the solve the C entry point launches (qmpc_solve_cw_inst_kernel with controller records,
//               the plain ConvexMpc tick without), qmpc_loop_rec_post_kernel (loop_post_plant_world_one: world-frame forces, the
//               robot's plant block with the tick's effective wrench, the outcome step)
//   persistent  qmpc_loop_rec_fused_kernel<3|5|6> on the wrench-form body with QMPC_WMODEL WM_CONVEX
// ONE unit serves the three calls: the push form's bits are the outcome form's where no window acts (per_robot = 0: none does;
// loop_push_wrench then leaves the plant block's bytes), and the outcome step never writes the state, so the call without outcome
// records runs on a scratch the handle owns.  The expansions of the plant blocks and the check of the windows are the kernels of
// the other three units (they do not depend on the model).  A unit of its own: every other unit compiles to the code it compiled
// to before.  Same flags and the same per-robot functions in both launch forms: the two forms give the same bits.
#define QMPC_FUSED_TU 1
#define qmpc qmpc_crec_tu
#include "qmpc_kernels.hip"
#include "qmpc_joint.hip"
#include "qmpc_ref.hip"
#include "qmpc_loop.hip"
#undef qmpc

#include <cmath>
#include <cstring>

#include "qmpc_kernel_slots.h"
#include "qmpc_loop_records.h"

namespace qmpc_crec_tu {

#define QMPC_REC_EXT 2
#define QMPC_REC_CONVEX 1
#include "qmpc_loop_rec.inc"
#undef QMPC_REC_CONVEX

}  // namespace qmpc_crec_tu
