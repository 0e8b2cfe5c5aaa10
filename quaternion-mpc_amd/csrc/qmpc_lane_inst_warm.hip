// Fourth unit of the lane-per-instance kernels: qmpc_lane_inst_kernel (qmpc_lane_inst.hip: per-lane robot and cost parameters)
// WARM-STARTED -- the later ticks of a closed loop with controller records under lp->warm_start on the lane kernel
// (qmpc_set_loop_warm_records under QMPC_INSTANCES_AUTO; include/qmpc.h).  The control flow is qmpc_lane_kernel<4, MD_QUAT>'s
// with previous solutions (qmpc_lane.hip): the per-lane `usable` rule, the WARM instantiations of the passes on LaneParams while
// some lane of the wavefront still carries a slack residual, the cold ones after, the pair splits of the plain warm tick, and
// hand-off records that carry the rows' initial residuals.  The cold first tick of such a call is qmpc_lane_inst_kernel's; the
// sort kernels and the hand-off's list kernel are those of qmpc_lane_inst.hip / qmpc_wform_inst_list.hip.  A unit of its own,
// with its own parameter table: the other lane units keep their code to the byte.
#define QL_UNIT 4
#include "qmpc_lane.hip"

#define QL_INST_NAME qmpc_lane_inst_warm
#define QL_INST_MD MD_QUAT
#define QL_INST_WARM 1
#define QL_INST_PAIRS 1
#include "qmpc_lane_inst_kernel.inc"
