// qmpc_wform_cinst_warm.hip -- a translation unit of libqmpc_hip.so of its own: ConvexMpc's warm-started solve with per-instance
// robot and cost parameters, the tick a closed loop with controller records repeats under lp->warm_start in the per-tick form on
// a ConvexMpc handle (qmpc_set_convex_records with qmpc_set_convex_warm_records; include/qmpc.h).  qmpc_solve_cw_inst_kernel
// (qmpc_wform_cinst.hip: P bound to the instance's expanded block, the rejected record's early exit) with the front of
// qmpc_solve_w_inst_warm_kernel (qmpc_wform_inst_warm.hip: the previous solution into sm[L.U], warm_t) -- which is that of the
// plain qmpc_solve_warm_kernel<VAR, true> (qmpc_loop.hip), so uniform records give the plain warm tick's bits.  Same sources,
// same flags as qmpc_wform.hip; a unit of its own so that the kernels of every other unit keep their code to the byte
// (qmpc_kernel_slots.h).
#define QMPC_FUSED_TU 1
#define qmpc qmpc_wcinstw_tu
#include "qmpc_kernels.hip"
#include "qmpc_ref.hip"
#include "qmpc_wform.h"

namespace qmpc {

// u_init: the previous solutions [batch][N][12] (it may be the buffer traj_u is written to); nullptr: a cold solve.
// check_prev: info[b] still holds the record of the robot's previous solve; a failed one left no usable solution behind, so
// this one starts cold -- the rule of qmpc_solve_warm_kernel and of the persistent kernel.
template <int WVAR>
__global__ __launch_bounds__(64, (WVAR == 5 || WVAR == 6) ? 2 : 1) void qmpc_solve_cw_inst_warm_kernel(
    const DevParams* __restrict__ Pi, const qmpc_input* __restrict__ in_, const double* u_init, double* __restrict__ forces,
    qmpc_info* __restrict__ info, double* traj_u, int batch, double* __restrict__ gws, const int* __restrict__ pstatus, int check_prev) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int b = blockIdx.x;
  if (b >= batch) return;
  const int wslot = b;
  const int lane = threadIdx.x;
  constexpr bool PROF = false;
  double* traj_x = nullptr;
  long long* prof_out = nullptr;
  constexpr const double* resume = nullptr;
  if (pstatus[b] != QMPC_OK) {      // a rejected record: zero forces and trajectory rows, no iteration
    const int N = Pi[b].N;
    if (lane < 12) forces[12 * (size_t)b + lane] = 0.0;
    if (lane == 0 && info) {
      qmpc_info r = {QMPC_BAD_PARAMS, 0, 0.0, 0.0, 0.0, 0.0};
      info[b] = r;
    }
    if (traj_u) for (int i = lane; i < N * 12; i += kWave) traj_u[(size_t)b * N * 12 + i] = 0.0;
    return;
  }
  const DevParams& P = Pi[b];
  const bool usable = u_init && (!check_prev || info[b].status == QMPC_OK || info[b].status == QMPC_MAX_ITER);
  const int warm_t = usable ? 1 : 0;
  if (usable) {
    LayoutW LWw;
    const Layout Lw = make_layout_w(P.N, &LWw, WVAR == 5 || WVAR == 6, WVAR == 6);
    for (int i = lane; i < P.N * 12; i += kWave) sm[Lw.U + i] = u_init[(size_t)b * P.N * 12 + i];
    __syncthreads();
  }
#define QMPC_WMODEL WM_CONVEX
#include "qmpc_wform_body.inc"
#undef QMPC_WMODEL
}

}  // namespace qmpc
#undef qmpc

#include "qmpc_kernel_slots.h"

using namespace qmpc_wcinstw_tu;
using namespace qmpc;

static decltype(&qmpc_solve_cw_inst_warm_kernel<3>) const kWformConvexInstWarm[] = {
    qmpc_solve_cw_inst_warm_kernel<3>, qmpc_solve_cw_inst_warm_kernel<5>, qmpc_solve_cw_inst_warm_kernel<6>};
static_assert(sizeof kWformConvexInstWarm / sizeof kWformConvexInstWarm[0] == kWformConvexInstWarmSlots, "qmpc_kernel_slots.h");

// called from qmpc_hip.hip (declared there); hidden: not part of the C ABI
__attribute__((visibility("hidden"))) hipError_t qmpc_wform_cinst_warm_set_lds() { return set_max_lds(kWformConvexInstWarm); }
// variant var (3 / 5 / 6) on the expanded blocks and verdicts (dev_blocks / status) of qmpc_wform_inst_expand_launch
__attribute__((visibility("hidden"))) hipError_t qmpc_wform_cinst_warm_launch(int var, int batch, size_t lds, hipStream_t s, const void* dev_blocks,
                                                                              const int* status, const qmpc_input* in, const double* u_init,
                                                                              double* forces, qmpc_info* info, double* traj_u, double* gws,
                                                                              int check_prev) {
  const int k = wform_convex_inst_warm_slot(var);
  if (k < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kWformConvexInstWarm[k], dim3((unsigned)batch), dim3(kWave), lds, s, static_cast<const DevParams*>(dev_blocks), in, u_init,
                     forces, info, traj_u, batch, gws, status, check_prev);
  return hipGetLastError();
}
