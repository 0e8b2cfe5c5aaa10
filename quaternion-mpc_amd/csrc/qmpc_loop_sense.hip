// qmpc_loop_sense.hip -- translation unit of libqmpc_hip.so: the closed loop of qmpc_loop_act.hip whose controller reads a
// MEASURED state, the true one plus the robot's estimator bias and reproducible bounded noise (qmpc_loop_run_sensing*,
// include/qmpc.h; the C entry points are in qmpc_hip.hip).  The kernels of qmpc_loop_act.hip with one change, the front step --
// qmpc_loop_rec.inc with QMPC_REC_EXT 5:
//   check       qmpc_sense_check_kernel (defined in the shared text, for this unit only), once per call after the plant expansion
//               and the checks of the windows, of the ground records and of the actuation records (the kernels of
//               qmpc_loop_ground.hip and qmpc_loop_act.hip, where there are such records): one thread per robot reads the
//               robot's record and writes QMPC_BAD_PARAMS into its plant block where it is invalid -- the front kernel, the
//               persistent kernel's entry and the freeze paths then treat the robot like that of an invalid plant record, and
//               its seen is never written.  It does not depend on the model: qmpc_loop_csense.hip has none of its own
//   per tick    qmpc_loop_rec_front_kernel of this unit (the first unit above EXT 1 with one of its own: it takes the sense
//               and seen pointers), where loop_front_sense_one saves the 13 true doubles of the state, writes
//               qmpc_loop::loop_sense_one's measurement in their place, calls loop_front_one as it stands and puts the true
//               doubles back; every solve form as it is -- the measured state only changes what the front writes into the
//               record; then qmpc_loop_rec_post_kernel, the post step of qmpc_loop_act.hip on the TRUE state (the actuation
//               record may be absent: every command then acts in its own tick)
//   persistent  qmpc_loop_rec_fused_kernel<3|5|6> with the same front step on lane 0.  The record (256 B) and seen (128 B) are
//               reached by pointer inside the front step of each tick; the 13 saved doubles live across the front end's call
//               only, nothing of the feature is live across the solve (variants 5 / 6 sit at their 256-register limit) and no
//               block is copied
// A unit of its own: every other unit compiles to the code it compiled to before.  Same flags and the same per-robot functions
// as qmpc_loop_act.hip; a robot whose record is the identity goes through that unit's front step text, so identity records give
// the results of qmpc_loop_run_actuation*, bit for bit, in both launch forms.
#define QMPC_FUSED_TU 1
#define qmpc qmpc_sense_tu
#include "qmpc_kernels.hip"
#include "qmpc_joint.hip"
#include "qmpc_ref.hip"
#include "qmpc_loop.hip"
#undef qmpc

#include <cmath>
#include <cstring>

#include "qmpc_kernel_slots.h"
#include "qmpc_loop_records.h"

namespace qmpc_sense_tu {

#define QMPC_REC_EXT 5
#include "qmpc_loop_rec.inc"

}  // namespace qmpc_sense_tu
