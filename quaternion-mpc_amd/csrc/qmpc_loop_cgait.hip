// qmpc_loop_cgait.hip -- translation unit of libqmpc_hip.so: qmpc_loop_run_gaits* on a ConvexMpc handle that opted in with
// qmpc_set_convex_records (include/qmpc.h; the C entry points are in qmpc_hip.hip).  The kernels of qmpc_loop_csense.hip with
// the front step of qmpc_loop_gait.hip -- qmpc_loop_rec.inc with QMPC_REC_EXT 6 and QMPC_REC_CONVEX:
//   per tick    qmpc_loop_rec_front_kernel (loop_front_sense_one hands a robot with a non-identity gait record to
//               loop_front_convex_gait_one, every other robot to loop_front_convex_one), the solve the C entry point launches,
//               qmpc_loop_rec_post_kernel (loop_post_actuation_one on the true state)
//   persistent  qmpc_loop_rec_fused_kernel<3|5|6> on the wrench-form body with QMPC_WMODEL WM_CONVEX
// qmpc_loop_csense.hip stays as it is (QMPC_REC_EXT 5).  The check of the gait records is qmpc_loop_gait.hip's kernel (it does
// not depend on the model).  A unit of its own: every other unit compiles to the code it compiled to before.  Same flags and
// the same per-robot functions in both launch forms.
#define QMPC_FUSED_TU 1
#define qmpc qmpc_cgait_tu
#include "qmpc_kernels.hip"
#include "qmpc_joint.hip"
#include "qmpc_ref.hip"
#include "qmpc_loop.hip"
#undef qmpc

#include <cmath>
#include <cstring>

#include "qmpc_kernel_slots.h"
#include "qmpc_loop_records.h"

namespace qmpc_cgait_tu {

#define QMPC_REC_EXT 6
#define QMPC_REC_CONVEX 1
#include "qmpc_loop_rec.inc"
#undef QMPC_REC_CONVEX

}  // namespace qmpc_cgait_tu
