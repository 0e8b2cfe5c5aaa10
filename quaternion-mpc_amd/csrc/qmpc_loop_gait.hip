// qmpc_loop_gait.hip -- translation unit of libqmpc_hip.so: the closed loop of qmpc_loop_sense.hip in which every robot walks a
// gait of its own -- frequency, per-leg two-entry contact pattern, split and starting phase (qmpc_loop_run_gaits*,
// include/qmpc.h; the C entry points are in qmpc_hip.hip).  The kernels of qmpc_loop_sense.hip with one change, the front end the
// front step selects -- qmpc_loop_rec.inc with QMPC_REC_EXT 6:
//   check       qmpc_gait_check_kernel (defined in the shared text, for this unit only), once per call after the checks of the
//               other records: one thread per robot writes QMPC_BAD_PARAMS into the robot's plant block where
//               qmpc_loop::loop_gait_valid refuses its record -- the robot is then frozen like that of an invalid plant record.
//               It does not depend on the model: qmpc_loop_cgait.hip has none of its own
//   per tick    qmpc_loop_rec_front_kernel of this unit (it takes the gait pointer), where loop_front_sense_one hands a robot
//               with a non-identity record to loop_front_gait_one (qmpc_loop.hip: loop_front_one with loop_raibert_gait and
//               loop_foot_update_gait) and every other robot to loop_front_one as it stands; every solve form as it is -- the
//               gait only changes what the front writes into the record and the state; then the post kernel of
//               qmpc_loop_sense.hip (the sensing and actuation records may be absent)
//   persistent  qmpc_loop_rec_fused_kernel<3|5|6> with the same front step on lane 0.  The record (128 B) is reached by pointer
//               inside the front end of each tick; nothing of the feature is live across the solve and no block is copied
// A unit of its own: every other unit compiles to the code it compiled to before.  Same flags and the same per-robot functions
// as qmpc_loop_sense.hip; a robot whose record is the identity goes through that unit's front step text, so identity records
// give the results of qmpc_loop_run_sensing*, bit for bit, in both launch forms.
#define QMPC_FUSED_TU 1
#define qmpc qmpc_gait_tu
#include "qmpc_kernels.hip"
#include "qmpc_joint.hip"
#include "qmpc_ref.hip"
#include "qmpc_loop.hip"
#undef qmpc

#include <cmath>
#include <cstring>

#include "qmpc_kernel_slots.h"
#include "qmpc_loop_records.h"

namespace qmpc_gait_tu {

#define QMPC_REC_EXT 6
#include "qmpc_loop_rec.inc"

}  // namespace qmpc_gait_tu
