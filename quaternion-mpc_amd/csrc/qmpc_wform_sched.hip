// qmpc_wform_sched.hip -- a translation unit of libqmpc_hip.so of its own: QuatMpc's solve with a CONTACT SCHEDULE over the
// horizon (qmpc_solve_schedule*; include/qmpc.h).  qmpc_solve_w_inst_kernel (qmpc_wform.hip: P bound to the
// instance's expanded block, the rejected record's early exit) with one more argument, the schedule: one byte per knot, bit l
// set where leg l stands during that knot.  The body is qmpc_wform_body.inc and the functions of qmpc_wform.h, compiled here
// with QMPC_WSCHED: every place that asks "is leg l in stance?" asks it for the knot at hand, the input reference is the knot's
// (c_kl mass 9.81 / nc_k), cone rows exist per (knot, stance leg).  A constant schedule gives qmpc_solve_w_inst_kernel's bits.
// The schedule is wave-uniform and at most 32 x 4 bits: two 64-bit words in scalar registers (qmpc_device.h: WSched), nothing
// in LDS -- the layout, its size and the workspace slice are those of the per-instance kernel.
// Same sources, same flags as qmpc_wform.hip; a unit of its own so that the kernels of every other unit keep their code to the
// byte (qmpc_kernel_slots.h).
#define QMPC_FUSED_TU 1
#define QMPC_WSCHED 1
#define qmpc qmpc_wsched_tu
#include "qmpc_kernels.hip"
#include "qmpc_ref.hip"
#include "qmpc_wform.h"

namespace qmpc {

// Pi[b], pstatus[b]: instance b's expanded parameters and its record's verdict (qmpc_expand_instances_kernel); sched[b][N].
// Verdicts of the schedule, per instance: a byte above 15 -- QMPC_BAD_PARAMS; a knot without a stance leg -- QMPC_NO_CONTACT
// (flight phases are out of scope); either gives zero forces and trajectory rows and no iteration, like a rejected record.
template <int WVAR>
__global__ __launch_bounds__(64, (WVAR == 5 || WVAR == 6) ? 2 : 1) void qmpc_solve_w_sched_kernel(
    const DevParams* __restrict__ Pi, const qmpc_input* __restrict__ in_, double* __restrict__ forces, qmpc_info* __restrict__ info,
    double* __restrict__ traj_u, double* __restrict__ traj_x, int batch, double* __restrict__ gws, const int* __restrict__ pstatus,
    const unsigned char* __restrict__ sched) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int b = blockIdx.x;
  if (b >= batch) return;
  const int wslot = b;
  const int lane = threadIdx.x;
  constexpr bool PROF = false;
  long long* prof_out = nullptr;
  constexpr int warm_t = 0;
  constexpr const double* resume = nullptr;
  const DevParams& P = Pi[b];
  const int Nk = P.N;      // (1 ... QMPC_MAX_HORIZON = 32 on every handle; an expanded block carries the handle's horizon)
  WSched wsched;
  int verdict = pstatus[b] != QMPC_OK ? QMPC_BAD_PARAMS : QMPC_OK;
  {
    // lane k reads knot k's byte; the words are assembled from wave-uniform values
    const unsigned mine = (lane < Nk) ? (unsigned)sched[(size_t)b * Nk + lane] : 1u;
    const unsigned long long high = __ballot(mine > 15u), empty = __ballot(mine == 0u);
    if (verdict == QMPC_OK) verdict = high ? QMPC_BAD_PARAMS : (empty ? QMPC_NO_CONTACT : QMPC_OK);
    unsigned long long w0 = 0, w1 = 0;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const unsigned long long bits = __ballot((mine >> l) & 1u);      // bit k: leg l stands at knot k
      for (int k = 0; k < Nk; ++k) {
        const unsigned long long bit = (bits >> k) & 1ull;
        if (k < 16) w0 |= bit << (4 * k + l);
        else w1 |= bit << (4 * (k - 16) + l);
      }
    }
    wsched.w0 = w0;
    wsched.w1 = w1;
    wsched.uz1 = 1.0 * P.mass * 9.81 / (double)1;      // (the set-up's c mass 9.81 / (double)nc with c = 1)
    wsched.uz2 = 1.0 * P.mass * 9.81 / (double)2;
    wsched.uz3 = 1.0 * P.mass * 9.81 / (double)3;
    wsched.uz4 = 1.0 * P.mass * 9.81 / (double)4;
  }
  if (verdict != QMPC_OK) {      // zero forces and trajectory rows, no iteration
    if (lane < 12) forces[12 * (size_t)b + lane] = 0.0;
    if (lane == 0 && info) {
      qmpc_info r = {verdict, 0, 0.0, 0.0, 0.0, 0.0};
      info[b] = r;
    }
    if (traj_u) for (int i = lane; i < Nk * 12; i += kWave) traj_u[(size_t)b * Nk * 12 + i] = 0.0;
    if (traj_x) for (int i = lane; i < (Nk + 1) * 13; i += kWave) traj_x[(size_t)b * (Nk + 1) * 13 + i] = 0.0;
    return;
  }
#include "qmpc_wform_body.inc"
}

// iparams == NULL: the handle's own values for every instance -- ONE record (qmpc_instance_params_from of the handle's
// parameters) through apply_instance_params, the arithmetic of qmpc_expand_instances_kernel on `batch` copies of it
__global__ __launch_bounds__(256) void qmpc_expand_uniform_kernel(DevParams base, qmpc_instance_params rec, DevParams* __restrict__ out,
                                                                  int* __restrict__ status, int batch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch) return;
  DevParams d;
  status[i] = apply_instance_params(base, rec, &d);
  out[i] = d;
}

}  // namespace qmpc
#undef qmpc

#include "qmpc_kernel_slots.h"

using namespace qmpc_wsched_tu;
using namespace qmpc;

static decltype(&qmpc_solve_w_sched_kernel<3>) const kWformSched[] = {qmpc_solve_w_sched_kernel<3>, qmpc_solve_w_sched_kernel<5>,
                                                                      qmpc_solve_w_sched_kernel<6>};
static_assert(sizeof kWformSched / sizeof kWformSched[0] == kWformSchedSlots, "qmpc_kernel_slots.h");

// called from qmpc_hip.hip (declared there); hidden: not part of the C ABI
__attribute__((visibility("hidden"))) hipError_t qmpc_wform_sched_set_lds() { return set_max_lds(kWformSched); }
// variant var (3 / 5 / 6) on the expanded blocks and verdicts (dev_blocks / status) of qmpc_wform_inst_expand_launch
__attribute__((visibility("hidden"))) hipError_t qmpc_wform_sched_launch(int var, int batch, size_t lds, hipStream_t s, const void* dev_blocks,
                                                                         const int* status, const qmpc_input* in, const unsigned char* sched,
                                                                         double* forces, qmpc_info* info, double* traj_u, double* traj_x,
                                                                         double* gws) {
  const int k = wform_sched_slot(var);
  if (k < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kWformSched[k], dim3((unsigned)batch), dim3(kWave), lds, s, static_cast<const DevParams*>(dev_blocks), in, forces, info,
                     traj_u, traj_x, batch, gws, status, sched);
  return hipGetLastError();
}
// the expansion of a call without records: the handle's values (`rec`, a host record) into every block
__attribute__((visibility("hidden"))) hipError_t qmpc_wform_sched_expand_uniform_launch(int batch, hipStream_t s, const void* dev_params,
                                                                                        size_t dev_params_size, const qmpc_instance_params* rec,
                                                                                        void* dev_out, int* status_out) {
  if (dev_params_size != sizeof(DevParams)) return hipErrorInvalidValue;
  DevParams P;
  std::memcpy(&P, dev_params, sizeof P);
  hipLaunchKernelGGL(qmpc_expand_uniform_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, s, P, *rec,
                     static_cast<DevParams*>(dev_out), status_out, batch);
  return hipGetLastError();
}
