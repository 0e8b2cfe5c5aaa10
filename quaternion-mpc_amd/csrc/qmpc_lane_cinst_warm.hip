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

namespace qmpc {
namespace lane {

#define QL_INST_MD MD_CONVEX
#include "qmpc_lane_inst_calls.inc"

// pi: the instance's expanded block (its instance fields become the lane's rows first, in every tick: which lane a robot takes
// changes with the sort); u_prev: the robot's previous inputs, or 0 for a cold start of this lane
__device__ __noinline__ void call_setup_cinstw(InstArgs a, unsigned long long rec, unsigned long long pi, unsigned long long u_prev,
                                               QL_PRIV_AS LaneK<4>* Kp, QL_PRIV_AS LaneState* sp) {
  QL_INST_PARAMS(a);
  const Ctx c = pass_ctx<4>(a.a);
  const WsOff O = make_wsoff<4>(U.N);
  lane_params_store(*reinterpret_cast<const DevParams*>(pi), const_cast<QL_GLOBAL_AS double*>(inst_prm(a)), 8u * kLaneWave, a.a.lane8);
  LaneK<4> K;
  LaneState st;
  lane_setup<4, MD_CONVEX>(P, c, O, reinterpret_cast<const double*>(rec), K, st, __builtin_amdgcn_readfirstlane(a.a.warm) != 0,
                           reinterpret_cast<const double*>(u_prev));
  priv_store(Kp, K);
  priv_store(sp, st);
}
// qmpc_lane_kernel<4, MD_CONVEX>'s launch with previous solutions (u_init [batch][N][12]; it may be the buffer traj_u is written to;
// check_prev: info[b] still holds the record of robot b's previous solve) on Pi[b] / pstatus[b] and prm as in
// qmpc_lane_cinst_kernel.  lanes: 64 or 32.  A lane whose record was rejected runs no iteration: zero forces and trajectory rows,
// {QMPC_BAD_PARAMS, 0, ...}.
__global__ __launch_bounds__(kLaneWave) void qmpc_lane_cinst_warm_kernel(int pslot, const double* __restrict__ in, const DevParams* __restrict__ Pi,
                                                                         const int* __restrict__ pstatus, double* __restrict__ forces,
                                                                         qmpc_info* __restrict__ info, int batch, double* __restrict__ ws,
                                                                         double* __restrict__ prm, unsigned slots, int lanes,
                                                                         const int* __restrict__ perm, const double* u_init, double* traj_u,
                                                                         int check_prev) {
  typedef LDim<4> D;
  const int lane = threadIdx.x;
  const DevParams& P = ql_params[pslot];
  const int itmax = P.iterations_max;
  const size_t block_elems = (size_t)make_wsoff<4>(P.N).total * kLaneWave;
  const unsigned long long wsb = reinterpret_cast<unsigned long long>(ws + (size_t)blockIdx.x * block_elems);
  const unsigned long long prb = reinterpret_cast<unsigned long long>(prm + (size_t)blockIdx.x * LPR_ROWS * kLaneWave);
  const InstArgs a = {{pslot, (unsigned)wsb, (unsigned)(wsb >> 32), 8u * (unsigned)lane, u_init ? 1u : 0u, 0u, 0x1F8u}, (unsigned)prb,
                      (unsigned)(prb >> 32)};
  const bool warm = u_init != nullptr;      // kernel argument: scalar
  const size_t tstride = (size_t)P.N * D::NU;
  LaneK<4> K;
  LaneState st;
  QL_PRIV_AS LaneK<4>* Kp = (QL_PRIV_AS LaneK<4>*)&K;
  QL_PRIV_AS LaneState* sp = (QL_PRIV_AS LaneState*)&st;
  for (long long base = (long long)blockIdx.x * lanes; base < batch; base += slots) {
    const long long pos = base + lane;
    const bool valid = lane < lanes && pos < batch;
    const int b = valid ? (perm ? perm[pos] : (int)pos) : 0;
    const bool rejected = valid && pstatus[b] != QMPC_OK;
    bool active = false;
    st.status = QMPC_BAD_PARAMS;
    if (valid && !rejected) {
      // the previous solution of this robot is usable unless its last solve failed (the rule of qmpc_lane_kernel)
      const bool usable = u_init && (!check_prev || info[b].status == QMPC_OK || info[b].status == QMPC_MAX_ITER);
      call_setup_cinstw(a, reinterpret_cast<unsigned long long>(in + (size_t)b * D::REC), reinterpret_cast<unsigned long long>(Pi + b),
                        usable ? reinterpret_cast<unsigned long long>(u_init + (size_t)b * tstride) : 0ull, Kp, sp);
      active = st.active;
    }
    while (__any(active)) {
      if (active) {
        // one interior-point iteration: the control flow of qmpc_lane_kernel's rounds with previous solutions -- the warm
        // instantiations of the passes while some lane still carries a slack residual (rho is exactly 0 after a lane's first
        // full step), the cold ones after
        if (warm && __any(st.rho != 0.0)) call_A_inst<true, false>(a, Kp, sp);
        else call_A_inst<false, false>(a, Kp, sp);
        const double resid = st.rho * st.rcmax;
        if (st.mu <= P.mu_final && resid <= P.tol_feas && st.last_step <= P.tol_step) { st.status = QMPC_OK; active = false; }
        else if (st.it > itmax) { st.status = QMPC_MAX_ITER; active = false; }
        else {
          double sg = P.sigma;
          const double amin = fmin(st.last_ap, st.last_ad);
          if (st.it > 1 && amin >= 0.99) sg = P.sigma_fast;
          else if (st.it > 1 && amin < 0.2) sg = fmax(sg, 0.8);
          else if (st.it > 1 && amin < 0.5) sg = fmax(sg, 0.5);
          st.target = sg * st.mu;
          const bool wrows = warm && __any(st.rho != 0.0);
          const bool okB = wrows ? call_B_inst<true, false>(a, Kp, sp) : call_B_inst<false, false>(a, Kp, sp);
          if (!okB) { st.status = QMPC_NOT_PD; active = false; }
          else {
            if (wrows) call_C_inst<true, false>(a, Kp, sp);
            else call_C_inst<false, false>(a, Kp, sp);
            if (st.bad_step) { st.status = QMPC_NOT_PD; active = false; }
          }
        }
      }
    }
    if (valid && !rejected)
      call_finish_inst(a, Kp, sp, reinterpret_cast<unsigned long long>(forces + (size_t)b * D::NU),
                       info ? reinterpret_cast<unsigned long long>(info + b) : 0ull,
                       traj_u ? reinterpret_cast<unsigned long long>(traj_u + (size_t)b * tstride) : 0ull, 0ull);
    if (rejected) {
      for (int j = 0; j < D::NU; ++j) forces[(size_t)b * D::NU + j] = 0.0;
      if (info) {
        const qmpc_info r = {QMPC_BAD_PARAMS, 0, 0.0, 0.0, 0.0, 0.0};
        info[b] = r;
      }
      if (traj_u) for (size_t i = 0; i < tstride; ++i) traj_u[(size_t)b * tstride + i] = 0.0;
    }
  }
}

}  // namespace lane
}  // namespace qmpc

// The handle's block into this unit's table (once per closed-loop call, outside its capture) ...
__attribute__((visibility("hidden"))) hipError_t qmpc_lane_cinst_warm_upload_params(int pslot, hipStream_t s, const void* dev_params,
                                                                                     size_t dev_params_size) {
  if (dev_params_size != sizeof(DevParams) || pslot < 0 || pslot >= kParamSlots) return hipErrorInvalidValue;
  return hipMemcpyToSymbolAsync(HIP_SYMBOL(ql_params), dev_params, sizeof(DevParams), sizeof(DevParams) * (size_t)pslot,
                                hipMemcpyHostToDevice, s);
}
// ... and the launch (one kernel: capturable), the arguments of qmpc_lane_cinst_launch_only with the previous solutions u_init, the
// buffer traj_u this tick's go to (it may be u_init) and check_prev.
__attribute__((visibility("hidden"))) hipError_t qmpc_lane_cinst_warm_launch_only(int pslot, int batch, hipStream_t s, const void* in,
                                                                                   const void* dev_blocks, const int* status, double* forces,
                                                                                   qmpc_info* info, double* ws, double* prm, unsigned slots,
                                                                                   const int* perm, const double* u_init, double* traj_u,
                                                                                   int check_prev) {
  if (slots % kLaneWave || pslot < 0 || pslot >= kParamSlots || batch < 1) return hipErrorInvalidValue;
  const int lanes = (size_t)batch * 2 <= slots ? 32 : 64;
  const unsigned need = (unsigned)(((size_t)batch + lanes - 1) / lanes);
  const unsigned waves = need < slots / kLaneWave ? need : slots / kLaneWave;
  const unsigned used = waves * (unsigned)lanes;
  const size_t lds = sizeof(double) * kLaneWave * LDim<4>::PLDS;
  hipLaunchKernelGGL(qmpc_lane_cinst_warm_kernel, dim3(waves), dim3(kLaneWave), lds, s, pslot, static_cast<const double*>(in),
                     static_cast<const DevParams*>(dev_blocks), status, forces, info, batch, ws, prm, used, lanes, perm, u_init, traj_u,
                     check_prev);
  return hipGetLastError();
}
