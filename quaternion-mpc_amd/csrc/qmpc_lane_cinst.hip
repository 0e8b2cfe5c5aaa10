// Fifth unit of the lane-per-instance kernels: ConvexMpc's converged-mode kernel with PER-LANE robot and cost parameters
// (qmpc_lane_cinst_kernel: qmpc_convex_solve_instances* and the ticks of the record loops on a ConvexMpc handle that opted in with
// qmpc_set_convex_lane_records, under QMPC_INSTANCES_AUTO; include/qmpc.h) with its launchers, its sort and its own parameter table.
// The passes are those of qmpc_lane_kernel<4, MD_CONVEX>, instantiated on LaneParams (qmpc_lane_core.h) as in qmpc_lane_inst.hip:
// the 39 doubles a per-instance record sets are read from the wavefront's parameter block, laid out [element][lane] like the
// workspace, everything else from the handle's block in constant memory.  What the plain ConvexMpc lane kernel has and no more:
// cold launches, no lane pairs (half-filled wavefronts run 32 lanes masked), no iteration cap and no hand-off.  A unit of its own:
// the other lane units keep their code to the byte.
#define QL_UNIT 5
#include "qmpc_lane.hip"

#define QL_INST_NAME qmpc_lane_cinst
#define QL_INST_MD MD_CONVEX
#define QL_INST_WARM 0
#define QL_INST_PAIRS 0
#define QL_INST_CON_OFF 24      // ConvexMpc's records carry their contacts at offset 24 (con_off of qmpc_lane_launch)
#include "qmpc_lane_inst_kernel.inc"
