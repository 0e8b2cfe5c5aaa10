// Sixth unit of the lane-per-instance kernels: qmpc_lane_cinst_kernel (qmpc_lane_cinst.hip: ConvexMpc's converged-mode kernel with
// per-lane robot and cost parameters) WARM-STARTED -- the later ticks of a closed loop with controller records under
// lp->warm_start on the lane kernel, on a ConvexMpc handle that opted in with qmpc_set_convex_records, qmpc_set_convex_lane_records
// and qmpc_set_convex_warm_records, under QMPC_INSTANCES_AUTO (include/qmpc.h).  The control flow is qmpc_lane_kernel<4, MD_CONVEX>'s
// with previous solutions (qmpc_lane.hip): the per-lane `usable` rule, the WARM instantiations of the passes on LaneParams while
// some lane of the wavefront still carries a slack residual, the cold ones after.  What the plain ConvexMpc lane kernel has and no
// more: no lane pairs (half-filled wavefronts run 32 lanes masked), no iteration cap and no hand-off.  The cold first tick of such
// a call is qmpc_lane_cinst_kernel's, and the sort is that unit's too.  A unit of its own, with its own parameter table: the
// other lane units keep their code to the byte.
#define QL_UNIT 6
#include "qmpc_lane.hip"

#define QL_INST_NAME qmpc_lane_cinst_warm
#define QL_INST_MD MD_CONVEX
#define QL_INST_WARM 1
#define QL_INST_PAIRS 0
#include "qmpc_lane_inst_kernel.inc"
