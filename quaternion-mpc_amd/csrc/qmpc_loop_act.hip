// qmpc_loop_act.hip -- translation unit of libqmpc_hip.so: the closed loop of qmpc_loop_ground.hip whose force reaches the feet
// through the robot's delay line and first-order actuator lag (qmpc_loop_run_actuation*, include/qmpc.h; the C entry points are
// in qmpc_hip.hip).  The kernels of qmpc_loop_ground.hip with one change, the post step -- qmpc_loop_rec.inc with QMPC_REC_EXT 4:
//   check       qmpc_act_check_kernel (defined in the shared text, for this unit only), once per call after the plant expansion
//               and the checks of the windows and of the ground records (qmpc_loop_ground.hip's kernel, when there is a ground
//               record): one thread per robot reads the robot's record and its line's count and writes QMPC_BAD_PARAMS into
//               its plant block where either is invalid -- the front kernel, the persistent kernel's entry and the freeze
//               paths then treat the robot like that of an invalid plant record, and its line is never written.  It does not
//               depend on the model: qmpc_loop_cact.hip (ConvexMpc's problem) has none of its own
//   per tick    qmpc_loop_rec_front_kernel of qmpc_loop_outcome.hip as it is (launched from there; this unit has none), every
//               solve form as it is, then qmpc_loop_rec_post_kernel, where loop_post_actuation_one pushes the command into the
//               line (qmpc_loop::loop_actuation_one), forms grf_world from what the actuators produce, clamps it on the true
//               ground when there is a record, and steps the plant under the delivered forces
//   persistent  qmpc_loop_rec_fused_kernel<3|5|6> with the same post step on lane 0.  The record (32 B) and the line (896 B) are
//               reached by pointer inside the post step of each tick: one ring slot read, one written, applied read-modify-
//               written, the ring indexed in global memory; nothing of the feature is live across the solve (variants 5 / 6 sit
//               at their 256-register limit) and no block is copied
// A unit of its own: every other unit compiles to the code it compiled to before.  Same flags and the same per-robot functions
// as qmpc_loop_ground.hip; a robot whose record is the identity goes through that unit's post step text, so identity records give
// the results of qmpc_loop_run_ground*, bit for bit, in both launch forms.
#define QMPC_FUSED_TU 1
#define qmpc qmpc_act_tu
#include "qmpc_kernels.hip"
#include "qmpc_joint.hip"
#include "qmpc_ref.hip"
#include "qmpc_loop.hip"
#undef qmpc

#include <cmath>
#include <cstring>

#include "qmpc_kernel_slots.h"
#include "qmpc_loop_records.h"

namespace qmpc_act_tu {

#define QMPC_REC_EXT 4
#include "qmpc_loop_rec.inc"

}  // namespace qmpc_act_tu
