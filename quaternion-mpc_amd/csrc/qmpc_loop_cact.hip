// qmpc_loop_cact.hip -- translation unit of libqmpc_hip.so: qmpc_loop_run_actuation* on a ConvexMpc handle that opted in with
// qmpc_set_convex_records (include/qmpc.h; the C entry points are in qmpc_hip.hip).  The kernels of qmpc_loop_cground.hip with
// the post step of qmpc_loop_act.hip -- qmpc_loop_rec.inc with QMPC_REC_EXT 4 and QMPC_REC_CONVEX:
//   per tick    qmpc_loop_rec_front_kernel (loop_front_convex_one on qmpc_convex_input records), the solve the C entry point
//               launches, qmpc_loop_rec_post_kernel (loop_post_actuation_one: forces_body = R' u of an accepted solve is the
//               command that enters the delay line; an identity record keeps the solve's world-frame bytes in grf_world, any
//               other forms R a; then the clamp, the plant step, the tally, the outcome step)
//   persistent  qmpc_loop_rec_fused_kernel<3|5|6> on the wrench-form body with QMPC_WMODEL WM_CONVEX
// qmpc_loop_cground.hip stays as it is (QMPC_REC_EXT 3).  The check of the actuation records is qmpc_loop_act.hip's kernel (it
// does not depend on the model).  A unit of its own: every other unit compiles to the code it compiled to before.  Same flags
// and the same per-robot functions in both launch forms.
#define QMPC_FUSED_TU 1
#define qmpc qmpc_cact_tu
#include "qmpc_kernels.hip"
#include "qmpc_joint.hip"
#include "qmpc_ref.hip"
#include "qmpc_loop.hip"
#undef qmpc

#include <cmath>
#include <cstring>

#include "qmpc_kernel_slots.h"
#include "qmpc_loop_records.h"

namespace qmpc_cact_tu {

#define QMPC_REC_EXT 4
#define QMPC_REC_CONVEX 1
#include "qmpc_loop_rec.inc"
#undef QMPC_REC_CONVEX

}  // namespace qmpc_cact_tu
