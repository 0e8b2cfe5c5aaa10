// qmpc_wform_cinst.hip -- a translation unit of libqmpc_hip.so of its own: ConvexMpc's solve with per-instance robot and cost
// parameters (qmpc_convex_solve_instances*; include/qmpc.h).  qmpc_solve_cw_kernel (qmpc_wform.hip: the wrench-form body with
// QMPC_WMODEL WM_CONVEX) with P bound to the instance's expanded block and the rejected record's early exit, as
// qmpc_solve_w_inst_kernel has them for QuatMpc's problem.  The blocks and verdicts are those of qmpc_expand_instances_kernel
// (qmpc_wform.hip): the record's fields go into the handle's DevParams whatever the model.  Same sources, same flags as
// qmpc_wform.hip; a unit of its own so that the kernels of every other unit keep their code to the byte (qmpc_kernel_slots.h).
#define QMPC_FUSED_TU 1
#define qmpc qmpc_wcinst_tu
#include "qmpc_kernels.hip"
#include "qmpc_ref.hip"
#include "qmpc_wform.h"

namespace qmpc {

// Pi[b]: instance b's parameters, pstatus[b]: its record's verdict.  The block address depends on blockIdx.x only and both
// pointers are const __restrict__, so the body's reads through P stay scalar loads, as those of the by-value kernel argument.
// ConvexMpc's state has 12 entries (world-frame forces, Euler angles): trajectory rows of 12.
template <int WVAR>
__global__ __launch_bounds__(64, (WVAR == 5 || WVAR == 6) ? 2 : 1) void qmpc_solve_cw_inst_kernel(
    const DevParams* __restrict__ Pi, const qmpc_input* __restrict__ in_, double* __restrict__ forces, qmpc_info* __restrict__ info,
    double* __restrict__ traj_u, double* __restrict__ traj_x, int batch, double* __restrict__ gws, const int* __restrict__ pstatus) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int b = blockIdx.x;
  if (b >= batch) return;
  const int wslot = b;
  const int lane = threadIdx.x;
  constexpr bool PROF = false;
  long long* prof_out = nullptr;
  constexpr int warm_t = 0;
  constexpr const double* resume = nullptr;
  if (pstatus[b] != QMPC_OK) {      // a rejected record: zero forces and trajectory rows, no iteration
    const int N = Pi[b].N;
    if (lane < 12) forces[12 * (size_t)b + lane] = 0.0;
    if (lane == 0 && info) {
      qmpc_info r = {QMPC_BAD_PARAMS, 0, 0.0, 0.0, 0.0, 0.0};
      info[b] = r;
    }
    if (traj_u) for (int i = lane; i < N * 12; i += kWave) traj_u[(size_t)b * N * 12 + i] = 0.0;
    if (traj_x) for (int i = lane; i < (N + 1) * 12; i += kWave) traj_x[(size_t)b * (N + 1) * 12 + i] = 0.0;
    return;
  }
  const DevParams& P = Pi[b];
#define QMPC_WMODEL WM_CONVEX
#include "qmpc_wform_body.inc"
#undef QMPC_WMODEL
}

}  // namespace qmpc
#undef qmpc

#include "qmpc_kernel_slots.h"

using namespace qmpc_wcinst_tu;
using namespace qmpc;

static decltype(&qmpc_solve_cw_inst_kernel<3>) const kWformConvexInst[] = {
    qmpc_solve_cw_inst_kernel<3>, qmpc_solve_cw_inst_kernel<5>, qmpc_solve_cw_inst_kernel<6>};
static_assert(sizeof kWformConvexInst / sizeof kWformConvexInst[0] == kWformConvexInstSlots, "qmpc_kernel_slots.h");

// called from qmpc_hip.hip (declared there); hidden: not part of the C ABI
__attribute__((visibility("hidden"))) hipError_t qmpc_wform_cinst_set_lds() { return set_max_lds(kWformConvexInst); }
// variant var (3 / 5 / 6) on the expanded blocks and verdicts (dev_blocks / status) of qmpc_wform_inst_expand_launch
__attribute__((visibility("hidden"))) hipError_t qmpc_wform_cinst_solve_launch(int var, int batch, size_t lds, hipStream_t s, const void* dev_blocks,
                                                                               const int* status, const qmpc_input* in, double* forces,
                                                                               qmpc_info* info, double* traj_u, double* traj_x, double* gws) {
  const int k = wform_convex_inst_slot(var);
  if (k < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kWformConvexInst[k], dim3((unsigned)batch), dim3(kWave), lds, s, static_cast<const DevParams*>(dev_blocks), in, forces,
                     info, traj_u, traj_x, batch, gws, status);
  return hipGetLastError();
}
