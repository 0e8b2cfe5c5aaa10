// qmpc_wform_inst_kernel.inc -- the wave-per-instance solve with per-instance robot and cost parameters in the units beside
// qmpc_wform.hip, defined once (DESIGN.md section 3t): the front of qmpc_solve_w_inst_kernel (qmpc_wform.hip: P bound to the
// instance's expanded block, the rejected record's early exit), for a warm unit with the front of qmpc_solve_warm_kernel
// (qmpc_loop.hip: the previous solution into sm[L.U], warm_t), then the wrench-form body; the instantiation table and the two hidden
// launchers.  Included at file scope, after qmpc_wform.h and inside the unit's `#define qmpc QMPC_WINST_TU`, by a unit that has set
//   QMPC_WINST_TU        the unit's namespace (it tells the kernels apart in a trace)
//   QMPC_WINST_KERNEL    the kernel template's name
//   QMPC_WINST_CONVEX    1: ConvexMpc's problem (the body with QMPC_WMODEL WM_CONVEX; trajectory rows of 12), 0: QuatMpc's
//   QMPC_WINST_WARM      1: the kernel takes previous solutions (u_init, check_prev) and writes no traj_x; 0: the cold kernel
//   QMPC_WINST_SLOT, QMPC_WINST_SLOTS    the unit's entries in qmpc_kernel_slots.h
//   QMPC_WINST_SET_LDS, QMPC_WINST_LAUNCH    the names qmpc_hip.hip declares
// qmpc_wform_inst_warm.hip (QuatMpc, warm), qmpc_wform_cinst.hip (ConvexMpc, cold), qmpc_wform_cinst_warm.hip (ConvexMpc, warm).
// Textual inclusion, as qmpc_wform_body.inc: every unit keeps its code object (tools/isa_same.py states it against a revision).
#if !defined(QMPC_WINST_TU) || !defined(QMPC_WINST_KERNEL) || !defined(QMPC_WINST_CONVEX) || !defined(QMPC_WINST_WARM) || \
    !defined(QMPC_WINST_SLOT) || !defined(QMPC_WINST_SLOTS) || !defined(QMPC_WINST_SET_LDS) || !defined(QMPC_WINST_LAUNCH)
#error "qmpc_wform_inst_kernel.inc: the including unit sets QMPC_WINST_TU, _KERNEL, _CONVEX, _WARM, _SLOT, _SLOTS, _SET_LDS, _LAUNCH"
#endif
// ... expand to their arguments or to nothing: the parameters and arguments only one start has
#if QMPC_WINST_WARM
#define QMPC_WINST_IF_WARM(...) __VA_ARGS__
#define QMPC_WINST_IF_COLD(...)
#else
#define QMPC_WINST_IF_WARM(...)
#define QMPC_WINST_IF_COLD(...) __VA_ARGS__
#endif

namespace qmpc {

// Pi[b]: instance b's parameters, pstatus[b]: its record's verdict.  The block address depends on blockIdx.x only and both
// pointers are const __restrict__, so the body's reads through P stay scalar loads, as those of the by-value kernel argument.
// A warm unit: u_init -- the previous solutions [batch][N][12] (it may be the buffer traj_u is written to); nullptr: a cold solve.
// check_prev: info[b] still holds the record of the robot's previous solve; a failed one left no usable solution behind, so
// this one starts cold -- the rule of qmpc_solve_warm_kernel and of the persistent kernel.
template <int WVAR>
__global__ __launch_bounds__(64, (WVAR == 5 || WVAR == 6) ? 2 : 1) void QMPC_WINST_KERNEL(
    const DevParams* __restrict__ Pi, const qmpc_input* __restrict__ in_, QMPC_WINST_IF_WARM(const double* u_init,)
    double* __restrict__ forces, qmpc_info* __restrict__ info, QMPC_WINST_IF_WARM(double* traj_u,)
    QMPC_WINST_IF_COLD(double* __restrict__ traj_u, double* __restrict__ traj_x,) int batch, double* __restrict__ gws,
    const int* __restrict__ pstatus QMPC_WINST_IF_WARM(, int check_prev)) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int b = blockIdx.x;
  if (b >= batch) return;
  const int wslot = b;
  const int lane = threadIdx.x;
  constexpr bool PROF = false;
  QMPC_WINST_IF_WARM(double* traj_x = nullptr;)
  long long* prof_out = nullptr;
  QMPC_WINST_IF_COLD(constexpr int warm_t = 0;)
  constexpr const double* resume = nullptr;
  if (pstatus[b] != QMPC_OK) {      // a rejected record: zero forces and trajectory rows, no iteration
    const int N = Pi[b].N;
    if (lane < 12) forces[12 * (size_t)b + lane] = 0.0;
    if (lane == 0 && info) {
      qmpc_info r = {QMPC_BAD_PARAMS, 0, 0.0, 0.0, 0.0, 0.0};
      info[b] = r;
    }
    if (traj_u) for (int i = lane; i < N * 12; i += kWave) traj_u[(size_t)b * N * 12 + i] = 0.0;
    QMPC_WINST_IF_COLD(if (traj_x) for (int i = lane; i < (N + 1) * (QMPC_WINST_CONVEX ? 12 : 13); i += kWave)
                         traj_x[(size_t)b * (N + 1) * (QMPC_WINST_CONVEX ? 12 : 13) + i] = 0.0;)
    return;
  }
  const DevParams& P = Pi[b];
#if QMPC_WINST_WARM
  const bool usable = u_init && (!check_prev || info[b].status == QMPC_OK || info[b].status == QMPC_MAX_ITER);
  const int warm_t = usable ? 1 : 0;
  if (usable) {
    LayoutW LWw;
    const Layout Lw = make_layout_w(P.N, &LWw, WVAR == 5 || WVAR == 6, WVAR == 6);
    for (int i = lane; i < P.N * 12; i += kWave) sm[Lw.U + i] = u_init[(size_t)b * P.N * 12 + i];
    __syncthreads();
  }
#endif
#if QMPC_WINST_CONVEX
#define QMPC_WMODEL WM_CONVEX
#endif
#include "qmpc_wform_body.inc"
#undef QMPC_WMODEL
}

}  // namespace qmpc
#undef qmpc

#include "qmpc_kernel_slots.h"

using namespace QMPC_WINST_TU;
using namespace qmpc;

static decltype(&QMPC_WINST_KERNEL<3>) const kWformInstTable[] = {QMPC_WINST_KERNEL<3>, QMPC_WINST_KERNEL<5>, QMPC_WINST_KERNEL<6>};
static_assert(sizeof kWformInstTable / sizeof kWformInstTable[0] == QMPC_WINST_SLOTS, "qmpc_kernel_slots.h");

// called from qmpc_hip.hip (declared there); hidden: not part of the C ABI
__attribute__((visibility("hidden"))) hipError_t QMPC_WINST_SET_LDS() { return set_max_lds(kWformInstTable); }
// variant var (3 / 5 / 6) on the expanded blocks and verdicts (dev_blocks / status) of qmpc_wform_inst_expand_launch
__attribute__((visibility("hidden"))) hipError_t QMPC_WINST_LAUNCH(int var, int batch, size_t lds, hipStream_t s, const void* dev_blocks,
                                                                   const int* status, const qmpc_input* in,
                                                                   QMPC_WINST_IF_WARM(const double* u_init,) double* forces, qmpc_info* info,
                                                                   double* traj_u, QMPC_WINST_IF_COLD(double* traj_x,) double* gws
                                                                   QMPC_WINST_IF_WARM(, int check_prev)) {
  const int k = QMPC_WINST_SLOT(var);
  if (k < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kWformInstTable[k], dim3((unsigned)batch), dim3(kWave), lds, s, static_cast<const DevParams*>(dev_blocks), in,
                     QMPC_WINST_IF_WARM(u_init,) forces, info, traj_u, QMPC_WINST_IF_COLD(traj_x,) batch, gws, status
                     QMPC_WINST_IF_WARM(, check_prev));
  return hipGetLastError();
}
