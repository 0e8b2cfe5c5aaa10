// qmpc_loop_ground.hip -- translation unit of libqmpc_hip.so: the closed loop with outcome records and push windows whose plant
// integrates under the force the robot's TRUE ground delivers (qmpc_loop_run_ground*, include/qmpc.h; the C entry points are in
// qmpc_hip.hip).  The kernels of qmpc_loop_push.hip with one change, the post step -- qmpc_loop_rec.inc with QMPC_REC_EXT 3:
//   check       qmpc_ground_check_kernel (defined in the shared text, for this unit only), once per call after the plant expansion
//               and the check of the windows: one thread per robot reads the robot's record and writes QMPC_BAD_PARAMS into its
//               plant block where a field is NaN, a mu < 0 or an fz_max <= 0 -- the front kernel, the persistent kernel's entry
//               and the freeze paths then treat the robot like that of an invalid plant record.  It does not depend on the
//               model: qmpc_loop_cground.hip (ConvexMpc's problem) has none of its own
//   per tick    qmpc_loop_rec_front_kernel of qmpc_loop_outcome.hip as it is (launched from there; this unit has none), every
//               solve form as it is, then qmpc_loop_rec_post_kernel, where loop_post_ground_one clamps the stance legs' world-
//               frame forces (qmpc_loop::loop_ground_clamp), steps the plant under the delivered forces and updates the tally
//   persistent  qmpc_loop_rec_fused_kernel<3|5|6> with the same post step on lane 0.  The record (64 B) and the tally (32 B)
//               are reached by pointer inside the post step of each tick: nothing of either is live across the solve
//               (variants 5 / 6 sit at their 256-register limit) and no block is copied
// A unit of its own: every other unit compiles to the code it compiled to before.  Same flags and the same per-robot functions
// as qmpc_loop_push.hip; a leg that no rule changes keeps its bytes and hands the plant the commanded forces_body, so records
// that never bind give the results of qmpc_loop_run_pushes*, bit for bit, in both launch forms.
#define QMPC_FUSED_TU 1
#define qmpc qmpc_ground_tu
#include "qmpc_kernels.hip"
#include "qmpc_joint.hip"
#include "qmpc_ref.hip"
#include "qmpc_loop.hip"
#undef qmpc

#include <cmath>
#include <cstring>

#include "qmpc_kernel_slots.h"
#include "qmpc_loop_records.h"

namespace qmpc_ground_tu {

#define QMPC_REC_EXT 3
#include "qmpc_loop_rec.inc"

}  // namespace qmpc_ground_tu
