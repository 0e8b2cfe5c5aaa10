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

namespace qmpc {
namespace lane {

#define QL_INST_MD MD_CONVEX
#include "qmpc_lane_inst_calls.inc"

// pi: the instance's expanded block (qmpc_expand_instances_kernel); its instance fields become the lane's rows first
__device__ __noinline__ void call_setup_cinst(InstArgs a, unsigned long long rec, unsigned long long pi, QL_PRIV_AS LaneK<4>* Kp,
                                              QL_PRIV_AS LaneState* sp) {
  QL_INST_PARAMS(a);
  const Ctx c = pass_ctx<4>(a.a);
  const WsOff O = make_wsoff<4>(U.N);
  lane_params_store(*reinterpret_cast<const DevParams*>(pi), const_cast<QL_GLOBAL_AS double*>(inst_prm(a)), 8u * kLaneWave, a.a.lane8);
  LaneK<4> K;
  LaneState st;
  lane_setup<4, MD_CONVEX>(P, c, O, reinterpret_cast<const double*>(rec), K, st, false, nullptr);
  priv_store(Kp, K);
  priv_store(sp, st);
}
// qmpc_lane_kernel<4, MD_CONVEX>'s cold launch with Pi[b] / pstatus[b] (the expanded block and the verdict of instance b) and prm,
// the parameter blocks of the resident wavefronts (LPR_ROWS rows of 64 lanes each).  Same persistent wavefronts, same sort
// (perm maps a position to b: the parameters are indexed by b), 32 or 64 lanes of a wavefront take instances.  A lane whose record
// was rejected runs no iteration: zero forces and trajectory rows (traj_x: (N + 1) * 12 per instance), {QMPC_BAD_PARAMS, 0, ...}.
__global__ __launch_bounds__(kLaneWave) void qmpc_lane_cinst_kernel(int pslot, const double* __restrict__ in, const DevParams* __restrict__ Pi,
                                                                    const int* __restrict__ pstatus, double* __restrict__ forces,
                                                                    qmpc_info* __restrict__ info, int batch, double* __restrict__ ws,
                                                                    double* __restrict__ prm, unsigned slots, int lanes,
                                                                    const int* __restrict__ perm, double* traj_u, double* traj_x) {
  typedef LDim<4> D;
  const int lane = threadIdx.x;
  const DevParams& P = ql_params[pslot];
  const int itmax = P.iterations_max;
  const size_t block_elems = (size_t)make_wsoff<4>(P.N).total * kLaneWave;
  const unsigned long long wsb = reinterpret_cast<unsigned long long>(ws + (size_t)blockIdx.x * block_elems);
  const unsigned long long prb = reinterpret_cast<unsigned long long>(prm + (size_t)blockIdx.x * LPR_ROWS * kLaneWave);
  const InstArgs a = {{pslot, (unsigned)wsb, (unsigned)(wsb >> 32), 8u * (unsigned)lane, 0u, 0u, 0x1F8u}, (unsigned)prb, (unsigned)(prb >> 32)};
  const size_t tstride = (size_t)P.N * D::NU;
  const size_t xstride = (size_t)(P.N + 1) * 12;
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
      call_setup_cinst(a, reinterpret_cast<unsigned long long>(in + (size_t)b * D::REC), reinterpret_cast<unsigned long long>(Pi + b), Kp, sp);
      active = st.active;
    }
    while (__any(active)) {
      if (active) {
        // one interior-point iteration: the control flow of qmpc_lane_kernel's cold rounds
        call_A_inst<false, false>(a, Kp, sp);
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
          if (!call_B_inst<false, false>(a, Kp, sp)) { st.status = QMPC_NOT_PD; active = false; }
          else {
            call_C_inst<false, false>(a, Kp, sp);
            if (st.bad_step) { st.status = QMPC_NOT_PD; active = false; }
          }
        }
      }
    }
    if (valid && !rejected)
      call_finish_inst(a, Kp, sp, reinterpret_cast<unsigned long long>(forces + (size_t)b * D::NU),
                       info ? reinterpret_cast<unsigned long long>(info + b) : 0ull,
                       traj_u ? reinterpret_cast<unsigned long long>(traj_u + (size_t)b * tstride) : 0ull,
                       traj_x ? reinterpret_cast<unsigned long long>(traj_x + (size_t)b * xstride) : 0ull);
    if (rejected) {
      for (int j = 0; j < D::NU; ++j) forces[(size_t)b * D::NU + j] = 0.0;
      if (info) {
        const qmpc_info r = {QMPC_BAD_PARAMS, 0, 0.0, 0.0, 0.0, 0.0};
        info[b] = r;
      }
      if (traj_u) for (size_t i = 0; i < tstride; ++i) traj_u[(size_t)b * tstride + i] = 0.0;
      if (traj_x) for (size_t i = 0; i < xstride; ++i) traj_x[(size_t)b * xstride + i] = 0.0;
    }
  }
}

// ---- the sort ------------------------------------------------------------------------------------------------------------------
// ConvexMpc's records carry their contacts at offset 24 (con_off of qmpc_lane_launch).  The plain call: the keys of
// qmpc_lane_sort_count / scatter<4> with that offset (prev = null, idle_last = 0).  A closed-loop tick with controller records: the
// plain tick's keys (the stance mask and 16 classes of the previous record's iteration count, 256 keys) and one class more, ordered
// after all of them: robots that will NOT solve in this tick -- a rejected record (status[b] != QMPC_OK) or the non-finite
// euler[0] the convex front kernel gives frozen and halted robots (word 0 of the record).  scratch as for qmpc_lane_sort_*:
// hist[256] | cursor[256] | perm[batch]; the last class is not counted: after the scan nothing reads hist any more, and hist[0]
// becomes its cursor (it begins where the counted keys end).
constexpr unsigned kKeyIdle = 256;
constexpr int kConvexConOff = 24;
__device__ __forceinline__ unsigned cinst_sort_key(const double* __restrict__ in, int b, const qmpc_info* __restrict__ prev,
                                                   const int* __restrict__ status, int idle_last) {
  if (idle_last && (status[b] != QMPC_OK || !isfinite(in[(size_t)b * LDim<4>::REC]))) return kKeyIdle;
  return stance_key<4>(in, b, kConvexConOff, prev);
}
__global__ __launch_bounds__(256) void qmpc_lane_cinst_sort_count(const double* __restrict__ in, int batch, int* __restrict__ scratch,
                                                                  const qmpc_info* __restrict__ prev, const int* __restrict__ status,
                                                                  int idle_last) {
  __shared__ int hist[256];
  hist[threadIdx.x] = 0;
  __syncthreads();
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < batch) {
    const unsigned key = cinst_sort_key(in, b, prev, status, idle_last);
    if (key < kKeyIdle) atomicAdd(&hist[key], 1);
  }
  __syncthreads();
  if (hist[threadIdx.x]) atomicAdd(&scratch[threadIdx.x], hist[threadIdx.x]);
}
__global__ __launch_bounds__(64) void qmpc_lane_cinst_sort_scan(int* __restrict__ scratch) {
  if (threadIdx.x != 0) return;
  int run = 0;
  for (int k = 0; k < 256; ++k) {
    const int n = scratch[k];
    scratch[256 + k] = run;
    run += n;
  }
  scratch[0] = run;      // the cursor of the class that will not solve
}
__global__ __launch_bounds__(256) void qmpc_lane_cinst_sort_scatter(const double* __restrict__ in, int batch, int* __restrict__ scratch,
                                                                    const qmpc_info* __restrict__ prev, const int* __restrict__ status,
                                                                    int idle_last) {
  __shared__ int hist[257], base[257];
  hist[threadIdx.x] = 0;
  if (threadIdx.x == 0) hist[kKeyIdle] = 0;
  __syncthreads();
  const int b = blockIdx.x * 256 + threadIdx.x;
  unsigned key = 0;
  int rank = 0;
  if (b < batch) {
    key = cinst_sort_key(in, b, prev, status, idle_last);
    rank = atomicAdd(&hist[key], 1);
  }
  __syncthreads();
  if (hist[threadIdx.x]) base[threadIdx.x] = atomicAdd(&scratch[256 + threadIdx.x], hist[threadIdx.x]);
  if (threadIdx.x == 0 && hist[kKeyIdle]) base[kKeyIdle] = atomicAdd(&scratch[0], hist[kKeyIdle]);
  __syncthreads();
  if (b < batch) scratch[512 + base[key] + rank] = b;
}

}  // namespace lane
}  // namespace qmpc

// The launch of qmpc_lane_kernel<4, MD_CONVEX> (qmpc_lane_launch, nl = -4) for per-instance records in two parts.  The upload: the
// handle's block into this unit's table (once per closed-loop call, outside its capture; before every launch of
// qmpc_convex_solve_instances*).
__attribute__((visibility("hidden"))) hipError_t qmpc_lane_cinst_upload_params(int pslot, hipStream_t s, const void* dev_params,
                                                                                size_t dev_params_size) {
  if (dev_params_size != sizeof(DevParams) || pslot < 0 || pslot >= kParamSlots) return hipErrorInvalidValue;
  return hipMemcpyToSymbolAsync(HIP_SYMBOL(ql_params), dev_params, sizeof(DevParams), sizeof(DevParams) * (size_t)pslot,
                                hipMemcpyHostToDevice, s);
}
// ... and the launch (one kernel: capturable): dev_blocks / status are the expansion kernel's outputs, prm
// qmpc_lane_inst_param_bytes(slots) bytes, perm the sort's permutation (qmpc_lane_cinst_sort_launch) or null.
__attribute__((visibility("hidden"))) hipError_t qmpc_lane_cinst_launch_only(int pslot, int batch, hipStream_t s, const void* in,
                                                                              const void* dev_blocks, const int* status, double* forces,
                                                                              qmpc_info* info, double* ws, double* prm, unsigned slots,
                                                                              const int* perm, double* traj_u, double* traj_x) {
  if (slots % kLaneWave || pslot < 0 || pslot >= kParamSlots || batch < 1) return hipErrorInvalidValue;
  // (the rule of qmpc_lane_launch) batches that would occupy at most half of the chip's SIMDs with full wavefronts run with 32
  // lanes per wavefront, the other half masked
  const int lanes = (size_t)batch * 2 <= slots ? 32 : 64;
  const unsigned need = (unsigned)(((size_t)batch + lanes - 1) / lanes);
  const unsigned waves = need < slots / kLaneWave ? need : slots / kLaneWave;
  const unsigned used = waves * (unsigned)lanes;
  const size_t lds = sizeof(double) * kLaneWave * LDim<4>::PLDS;
  hipLaunchKernelGGL(qmpc_lane_cinst_kernel, dim3(waves), dim3(kLaneWave), lds, s, pslot, static_cast<const double*>(in),
                     static_cast<const DevParams*>(dev_blocks), status, forces, info, batch, ws, prm, used, lanes, perm, traj_u, traj_x);
  return hipGetLastError();
}
// both parts: a launch of qmpc_convex_solve_instances*
__attribute__((visibility("hidden"))) hipError_t qmpc_lane_cinst_launch(int pslot, int batch, hipStream_t s, const void* dev_params,
                                                                         size_t dev_params_size, const void* in, const void* dev_blocks,
                                                                         const int* status, double* forces, qmpc_info* info, double* ws,
                                                                         double* prm, unsigned slots, const int* perm, double* traj_u,
                                                                         double* traj_x) {
  const hipError_t e = qmpc_lane_cinst_upload_params(pslot, s, dev_params, dev_params_size);
  if (e != hipSuccess) return e;
  return qmpc_lane_cinst_launch_only(pslot, batch, s, in, dev_blocks, status, forces, info, ws, prm, slots, perm, traj_u, traj_x);
}
// The sort (scratch: qmpc_lane_scratch_bytes(batch) bytes; the permutation is left at scratch + 512).  The plain call: prev = null,
// idle_last = 0 (status is not read).  A closed-loop tick with controller records: prev the previous solves' records (the handle's
// output buffer) or null, status the expansion's verdicts, idle_last = 1 unless QMPC_LANE_SORT_IDLE=0.
__attribute__((visibility("hidden"))) hipError_t qmpc_lane_cinst_sort_launch(int batch, hipStream_t s, const void* in, const qmpc_info* prev,
                                                                              const int* status, int idle_last, int* scratch) {
  const double* rec = static_cast<const double*>(in);
  const hipError_t e = hipMemsetAsync(scratch, 0, sizeof(int) * 512, s);
  if (e != hipSuccess) return e;
  const unsigned blocks = (unsigned)((batch + 255) / 256);
  hipLaunchKernelGGL(qmpc_lane_cinst_sort_count, dim3(blocks), dim3(256), 0, s, rec, batch, scratch, prev, status, idle_last);
  hipLaunchKernelGGL(qmpc_lane_cinst_sort_scan, dim3(1), dim3(64), 0, s, scratch);
  hipLaunchKernelGGL(qmpc_lane_cinst_sort_scatter, dim3(blocks), dim3(256), 0, s, rec, batch, scratch, prev, status, idle_last);
  return hipGetLastError();
}
