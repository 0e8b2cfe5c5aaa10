// qmpc_wform_inst_list.hip -- a translation unit of libqmpc_hip.so of its own: the straggler hand-off of
// qmpc_solve_instances* on the lane kernel (QMPC_INSTANCES_AUTO; qmpc_lane_inst.hip).  qmpc_solve_w_list_kernel
// (qmpc_wform.hip) with P bound to the drawn instance's expanded block, as qmpc_solve_w_inst_kernel binds it: the instance
// index is wave-uniform, so the reads stay scalar loads.  Same sources, same flags as qmpc_wform.hip; a unit of its own so
// that the kernels of that unit keep their code to the byte (qmpc_kernel_slots.h).
#define QMPC_FUSED_TU 1
#define qmpc qmpc_winst_tu
#include "qmpc_kernels.hip"
#include "qmpc_ref.hip"
#include "qmpc_wform.h"

namespace qmpc {

// sel[0 .. *sel_count): the instances the capped launch of qmpc_lane_inst_kernel left; hstate: their state records (8 + 84 N
// doubles each, the format of qmpc_lane_kernel's).  A listed instance has a valid record: rejected ones never join the list.
template <int WVAR>
__global__ __launch_bounds__(64, 1) void qmpc_solve_w_list_inst_kernel(
    const DevParams* __restrict__ Pi, const qmpc_input* __restrict__ in_, double* __restrict__ forces, qmpc_info* __restrict__ info,
    double* __restrict__ traj_u, double* __restrict__ traj_x, const int* __restrict__ sel, const int* __restrict__ sel_count,
    double* __restrict__ gws, const double* __restrict__ hstate, int hcap) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int lane = threadIdx.x;
  constexpr bool PROF = false;
  constexpr int warm_t = 0;
  long long* prof_out = nullptr;
  const int wslot = blockIdx.x;
  const int count = sel_count[0];
  int* cursor = const_cast<int*>(sel_count) + 1;      // the workgroups draw their instances (qmpc_solve_w_list_kernel)
  for (;;) {
    int i = 0;
    if (lane == 0) i = atomicAdd(cursor, 1);
    i = __builtin_amdgcn_readfirstlane(i);
    if (i >= count) break;
    const int b = __builtin_amdgcn_readfirstlane(sel[i]);
    const DevParams& P = Pi[b];
    const double* resume = (hstate && i < hcap) ? hstate + (size_t)i * (8 + 84 * (size_t)P.N) : nullptr;
    [&]() {                            // `return` in the body (rejected input) ends this instance only
#include "qmpc_wform_body.inc"
    }();
    __syncthreads();
  }
}

}  // namespace qmpc
#undef qmpc

#include "qmpc_kernel_slots.h"

using namespace qmpc_winst_tu;
using namespace qmpc;

static decltype(&qmpc_solve_w_list_inst_kernel<3>) const kWformListInst[] = {qmpc_solve_w_list_inst_kernel<3>,
                                                                             qmpc_solve_w_list_inst_kernel<5>};
static_assert(sizeof kWformListInst / sizeof kWformListInst[0] == kWformListInstSlots, "qmpc_kernel_slots.h");

// called from qmpc_hip.hip (declared there); hidden: not part of the C ABI
__attribute__((visibility("hidden"))) hipError_t qmpc_wform_inst_list_set_lds() { return set_max_lds(kWformListInst); }
// the instances sel[0 .. *sel_count) (device memory) with the expanded blocks dev_blocks, `grid` workgroups walking the list
__attribute__((visibility("hidden"))) hipError_t qmpc_wform_inst_list_launch(int var, int grid, size_t lds, hipStream_t s, const void* dev_blocks,
                                                                             const qmpc_input* in, double* forces, qmpc_info* info,
                                                                             double* traj_u, double* traj_x, const int* sel,
                                                                             const int* sel_count, double* gws, const double* hstate,
                                                                             int hcap) {
  const int k = wform_list_inst_slot(var);
  if (k < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kWformListInst[k], dim3((unsigned)grid), dim3(kWave), lds, s, static_cast<const DevParams*>(dev_blocks), in, forces, info,
                     traj_u, traj_x, sel, sel_count, gws, hstate, hcap);
  return hipGetLastError();
}
