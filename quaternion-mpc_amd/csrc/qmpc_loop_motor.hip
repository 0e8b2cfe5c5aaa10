// qmpc_loop_motor.hip -- translation unit of libqmpc_hip.so: the closed loop of qmpc_loop_gait.hip whose delivered foot force
// respects the motors' joint torque limits, and which records the torque every joint was asked for (qmpc_loop_run_motors*,
// include/qmpc.h; the C entry points are in qmpc_hip.hip).  The kernels of qmpc_loop_gait.hip with one change, the motor step in
// the post step -- qmpc_loop_rec.inc with QMPC_REC_EXT 7:
//   check       qmpc_motor_check_kernel (defined in the shared text, for this unit only), once per call after the checks of the
//               other records: one thread per robot writes QMPC_BAD_PARAMS into the robot's plant block where
//               qmpc_joint::loop_motor_valid refuses its record or tally -- the robot is then frozen like that of an invalid
//               plant record.  It does not depend on the model: qmpc_loop_cmotor.hip has none of its own
//   per tick    qmpc_loop_rec_front_kernel of this unit (the gait unit's text), every solve form as it is, then
//               qmpc_loop_rec_post_kernel, whose loop_post_actuation_one calls loop_post_motor between the actuation line and
//               the ground clamp: inverse kinematics of every leg, -J'u of the stance legs, the clip and J'u' = -t where a
//               limit binds (qmpc_joint::loop_motor_one of qmpc_joint_math.h)
//   persistent  qmpc_loop_rec_fused_kernel<3|5|6> with the same post step on lane 0.  The record (128 B) and the tally (320 B)
//               are reached by pointer inside loop_post_motor, which is out of line: its registers are not the solve's, and
//               nothing of the feature is live across the solve.  The geometry (256 B) is a kernel argument
// A unit of its own: every other unit compiles to the code it compiled to before.  Same flags and the same per-robot functions
// as qmpc_loop_gait.hip; a leg no limit binds on goes through that unit's post step text, so +inf limits give the results of
// qmpc_loop_run_gaits*, bit for bit, in both launch forms.
#define QMPC_FUSED_TU 1
#define qmpc qmpc_motor_tu
#include "qmpc_kernels.hip"
#include "qmpc_joint.hip"
#include "qmpc_ref.hip"
#include "qmpc_loop.hip"
#undef qmpc

#include <cmath>
#include <cstring>

#include "qmpc_kernel_slots.h"
#include "qmpc_loop_records.h"

namespace qmpc_motor_tu {

#define QMPC_REC_EXT 7
#include "qmpc_loop_rec.inc"

}  // namespace qmpc_motor_tu
