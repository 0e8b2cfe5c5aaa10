// Third unit of the lane-per-instance kernels: the converged mode's kernel with PER-LANE robot and cost parameters
// (qmpc_lane_inst_kernel: qmpc_solve_instances* under QMPC_INSTANCES_AUTO, include/qmpc.h) with its launcher and its own
// parameter table.  The passes are those of qmpc_lane_kernel<4, MD_QUAT>, instantiated on LaneParams (qmpc_lane_core.h): the 39
// doubles a per-instance record sets are read from the wavefront's parameter block, laid out [element][lane] like the
// workspace, everything else from the handle's block in constant memory.  Cold launches of the four-point quaternion model
// only; the plain and the pair forms.  A unit of its own: the units of qmpc_lane.hip keep their code to the byte.
#define QL_UNIT 3
#include "qmpc_lane.hip"

#define QL_INST_NAME qmpc_lane_inst
#define QL_INST_MD MD_QUAT
#define QL_INST_WARM 0
#define QL_INST_PAIRS 1
#define QL_INST_CON_OFF LDim<4>::R_CON
#include "qmpc_lane_inst_kernel.inc"
