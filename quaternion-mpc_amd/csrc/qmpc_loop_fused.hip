// qmpc_loop_fused.hip -- second translation unit of libqmpc_hip.so: the persistent wave-per-robot kernel of the closed
// loop (qmpc_loop_fused_kernel, defined in qmpc_loop.hip) and its launcher.  The kernel re-uses the body of the solve
// kernel (qmpc_solve_body.inc); compiled next to qmpc_solve_kernel it perturbs that kernel's inlining and register
// allocation (contract workload 2 % slower), so it gets a code object of its own.  The shared sources are included
// under another namespace name: their non-template kernels would otherwise be defined twice at link time.
#define QMPC_FUSED_TU 1
#define qmpc qmpc_fused_tu
#include "qmpc_kernels.hip"
#include "qmpc_joint.hip"
#include "qmpc_ref.hip"
#include "qmpc_loop.hip"
#undef qmpc

#include <cstring>

#include "qmpc_kernel_slots.h"

using namespace qmpc_fused_tu;
using namespace qmpc;

// the launch tables of this unit (slots: qmpc_kernel_slots.h): the persistent loop kernels and the warm-started solves
static decltype(&qmpc_loop_fused_kernel<0, false, false>) const kFused[] = {
    // JOINT = false: the converged mode, QuatMpc 0 1 2 3 5 6, ConvexMpc 0 1 2 3 5 6; the reference mode, QuatMpc 0 1 3 5, ConvexMpc 3 5
    qmpc_loop_fused_kernel<0, false, false, false>, qmpc_loop_fused_kernel<1, false, false, false>, qmpc_loop_fused_kernel<2, false, false, false>,
    qmpc_loop_fused_kernel<3, false, false, false>, qmpc_loop_fused_kernel<5, false, false, false>, qmpc_loop_fused_kernel<6, false, false, false>,
    qmpc_loop_fused_kernel<0, false, false, true>, qmpc_loop_fused_kernel<1, false, false, true>, qmpc_loop_fused_kernel<2, false, false, true>,
    qmpc_loop_fused_kernel<3, false, false, true>, qmpc_loop_fused_kernel<5, false, false, true>, qmpc_loop_fused_kernel<6, false, false, true>,
    qmpc_loop_fused_kernel<0, false, true, false>, qmpc_loop_fused_kernel<1, false, true, false>,
    qmpc_loop_fused_kernel<3, false, true, false>, qmpc_loop_fused_kernel<5, false, true, false>,
    qmpc_loop_fused_kernel<3, false, true, true>, qmpc_loop_fused_kernel<5, false, true, true>,
    // JOINT = true: the converged mode, QuatMpc 0 1 2 3 5 6, ConvexMpc 0 1 2 3 5 6; the reference mode, QuatMpc 0 1 3 5, ConvexMpc 3 5
    qmpc_loop_fused_kernel<0, true, false, false>, qmpc_loop_fused_kernel<1, true, false, false>, qmpc_loop_fused_kernel<2, true, false, false>,
    qmpc_loop_fused_kernel<3, true, false, false>, qmpc_loop_fused_kernel<5, true, false, false>, qmpc_loop_fused_kernel<6, true, false, false>,
    qmpc_loop_fused_kernel<0, true, false, true>, qmpc_loop_fused_kernel<1, true, false, true>, qmpc_loop_fused_kernel<2, true, false, true>,
    qmpc_loop_fused_kernel<3, true, false, true>, qmpc_loop_fused_kernel<5, true, false, true>, qmpc_loop_fused_kernel<6, true, false, true>,
    qmpc_loop_fused_kernel<0, true, true, false>, qmpc_loop_fused_kernel<1, true, true, false>,
    qmpc_loop_fused_kernel<3, true, true, false>, qmpc_loop_fused_kernel<5, true, true, false>,
    qmpc_loop_fused_kernel<3, true, true, true>, qmpc_loop_fused_kernel<5, true, true, true>};
static decltype(&qmpc_solve_warm_kernel<0>) const kWarm[] = {  // QuatMpc 0 1 2 3 5 6, ConvexMpc 0 1 2 3 5 6
    qmpc_solve_warm_kernel<0, false>, qmpc_solve_warm_kernel<1, false>, qmpc_solve_warm_kernel<2, false>,
    qmpc_solve_warm_kernel<3, false>, qmpc_solve_warm_kernel<5, false>, qmpc_solve_warm_kernel<6, false>,
    qmpc_solve_warm_kernel<0, true>, qmpc_solve_warm_kernel<1, true>, qmpc_solve_warm_kernel<2, true>,
    qmpc_solve_warm_kernel<3, true>, qmpc_solve_warm_kernel<5, true>, qmpc_solve_warm_kernel<6, true>};
static_assert(sizeof kFused / sizeof kFused[0] == kFusedSlots && sizeof kWarm / sizeof kWarm[0] == kWarmSlots, "qmpc_kernel_slots.h");

// called from qmpc_hip.hip (declared there); hidden: not part of the C ABI
__attribute__((visibility("hidden"))) hipError_t qmpc_loop_fused_set_lds() { return set_max_lds(kFused, kWarm); }

// var: 0 everything in LDS, 1 gains in the workspace, 2 gains and slack arrays there (converged mode only),
// 3 / 5 / 6 the same three of the wrench form (the reference mode: 3 / 5)
__attribute__((visibility("hidden"))) hipError_t qmpc_fused_launch(int var, int reference_mode, int convex, int batch, size_t lds,
                                                                   hipStream_t s,
                                                                   const void* dev_params, size_t dev_params_size,
                                                                   const qmpc_loop_params* lp, qmpc_loop_state* st,
                                                                   qmpc_input* rec, double* forces, qmpc_info* info,
                                                                   double* trace_f, double* trace_c, int ticks, double* gws,
                                                                   const qmpc_leg_geometry* geom, double* joint_pos,
                                                                   qmpc_joint_command* cmd, qmpc_joint_command* trace_cmd) {
  if (dev_params_size != sizeof(DevParams)) return hipErrorInvalidValue;
  DevParams P;
  std::memcpy(&P, dev_params, sizeof P);
  const qmpc_loop_params LP = *lp;
  FusedJoint JL;
  std::memset(&JL, 0, sizeof JL);
  if (geom) {
    static_assert(sizeof(LegGeom) == sizeof(qmpc_leg_geometry), "kernel argument mirrors the ABI struct");
    std::memcpy(&JL.G, geom, sizeof JL.G);
    JL.joint_pos = joint_pos;
    JL.cmd = cmd;
    JL.trace = trace_cmd;
  }
  const int k = fused_slot(var, reference_mode != 0, convex != 0, geom != nullptr);
  if (k < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kFused[k], dim3((unsigned)batch), dim3(kWave), lds, s, P, LP, st, rec, forces, info, trace_f, trace_c, ticks, batch,
                     gws, JL);
  return hipGetLastError();
}

__attribute__((visibility("hidden"))) hipError_t qmpc_warm_launch(int var, int convex, int batch, size_t lds, hipStream_t s,
                                                                  const void* dev_params, size_t dev_params_size,
                                                                  const qmpc_input* in, const double* u_init, double* forces,
                                                                  qmpc_info* info, double* traj_u, double* gws, int check_prev) {
  if (dev_params_size != sizeof(DevParams)) return hipErrorInvalidValue;
  DevParams P;
  std::memcpy(&P, dev_params, sizeof P);
  const int k = warm_slot(var, convex != 0);
  if (k < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kWarm[k], dim3((unsigned)batch), dim3(kWave), lds, s, P, in, u_init, forces, info, traj_u, batch, gws, check_prev);
  return hipGetLastError();
}
