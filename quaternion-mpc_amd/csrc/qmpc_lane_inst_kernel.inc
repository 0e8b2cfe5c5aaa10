// qmpc_lane_inst_kernel.inc -- the lane units with per-lane robot and cost parameters, defined once (DESIGN.md section 3t): the
// passes of qmpc_lane_kernel<4, QL_INST_MD> instantiated on LaneParams (qmpc_lane_core.h) as separate functions with the arguments
// they are called with, the set-up, the kernel, the idle-last sort of the cold units, and the hidden launchers.  Included after
// qmpc_lane.hip, at file scope, by a unit that has set
//   QL_INST_NAME   the prefix of what the unit exports: <name>_kernel, <name>_upload_params, <name>_launch_only, <name>_sort_launch
//   QL_INST_MD     the model: MD_QUAT or MD_CONVEX
//   QL_INST_WARM   1: the kernel takes previous solutions (u_init, check_prev) and writes no traj_x; 0: the cold kernel, which
//                  also defines the sort of its model's ticks (the warm unit's ticks run behind the same sort)
//   QL_INST_PAIRS  1: lane pairs, the iteration cap and the hand-off records (QuatMpc: the three go together); 0: none of them
//   QL_INST_CON_OFF  (cold units) where a record carries its contacts: the sort's key
// qmpc_lane_inst.hip (QL_UNIT 3: qmpc_lane_inst, MD_QUAT, cold, pairs), qmpc_lane_inst_warm.hip (4: ... warm),
// qmpc_lane_cinst.hip (5: qmpc_lane_cinst, MD_CONVEX, cold, no pairs), qmpc_lane_cinst_warm.hip (6: ... warm).
// Textual inclusion: each unit instantiates what it calls and keeps its own code object with its own parameter table, and a
// kernel's parameter list is the one its flavour needs (kernarg offsets are in the code).  What a flavour's list lacks is a
// constant in the kernel's prologue, so the body below is one text and the compiler drops what the constant rules out
// (tools/isa_same.py states every function against a revision).
#if !defined(QL_INST_NAME) || !defined(QL_INST_MD) || !defined(QL_INST_WARM) || !defined(QL_INST_PAIRS)
#error "QL_INST_NAME, QL_INST_MD (MD_QUAT or MD_CONVEX), QL_INST_WARM (0/1), QL_INST_PAIRS (0/1): set by the including unit"
#endif
#define QL_INST_CAT2(a, b) a##b
#define QL_INST_CAT(a, b) QL_INST_CAT2(a, b)
#define QL_INST_FN(suffix) QL_INST_CAT(QL_INST_NAME, suffix)
// ... expand to their arguments or to nothing: the parameters and arguments only some flavours have
#if QL_INST_WARM
#define QL_INST_IF_WARM(...) __VA_ARGS__
#define QL_INST_IF_COLD(...)
#else
#define QL_INST_IF_WARM(...)
#define QL_INST_IF_COLD(...) __VA_ARGS__
#endif
#if QL_INST_PAIRS
#define QL_INST_IF_PAIRS(...) __VA_ARGS__
#else
#define QL_INST_IF_PAIRS(...)
#endif

namespace qmpc {
namespace lane {

struct InstArgs {
  PassArgs a;
  unsigned pr_lo, pr_hi;     // this wave's parameter block
};
__device__ __forceinline__ QL_GLOBAL_AS const double* inst_prm(const InstArgs& a) {
  const unsigned lo = __builtin_amdgcn_readfirstlane(a.pr_lo), hi = __builtin_amdgcn_readfirstlane(a.pr_hi);
  return reinterpret_cast<QL_GLOBAL_AS const double*>(((unsigned long long)hi << 32) | lo);
}
// U: the handle's block (scalar loads); P: the passes' parameter source
#define QL_INST_PARAMS(a)                                                         \
  const DevParams& U = ql_params[__builtin_amdgcn_readfirstlane((a).a.pslot)];    \
  const LaneParams P(U, inst_prm(a), 8u * kLaneWave, (a).a.lane8)

template <bool WARM, bool PAIR>
__device__ __noinline__ void call_A_inst(InstArgs a, QL_PRIV_AS const LaneK<4>* Kp, QL_PRIV_AS LaneState* sp) {
  QL_INST_PARAMS(a);
  const Ctx c = pass_ctx<4>(a.a);
  const WsOff O = make_wsoff<4>(U.N);
  LaneK<4> K;
  priv_load(K, Kp);
  LaneState st;
  priv_load(st, (QL_PRIV_AS const LaneState*)sp);
  st.it += 1;
  pass_A<4, WARM, QL_INST_MD, PAIR>(P, c, O, K, st, st.it == 1, (FootPtr)Kp->foot);
  priv_store(sp, st);
}
template <bool WARM, bool PAIR>
__device__ __noinline__ bool call_B_inst(InstArgs a, QL_PRIV_AS const LaneK<4>* Kp, QL_PRIV_AS LaneState* sp) {
  QL_INST_PARAMS(a);
  const Ctx c = pass_ctx<4>(a.a);
  const WsOff O = make_wsoff<4>(U.N);
  LaneK<4> K;
  priv_load(K, Kp);
  LaneState st;
  priv_load(st, (QL_PRIV_AS const LaneState*)sp);
  const bool ok = pass_B<4, WARM, QL_INST_MD, false, PAIR>(P, c, O, K, st, (FootPtr)Kp->foot);
#if defined(QL_PROFILE)
  priv_store(sp, st);
#endif
  return ok;
}
template <bool WARM, bool PAIR>
__device__ __noinline__ void call_C_inst(InstArgs a, QL_PRIV_AS const LaneK<4>* Kp, QL_PRIV_AS LaneState* sp) {
  QL_INST_PARAMS(a);
  const Ctx c = pass_ctx<4>(a.a);
  const WsOff O = make_wsoff<4>(U.N);
  LaneK<4> K;
  priv_load(K, Kp);
  LaneState st;
  priv_load(st, (QL_PRIV_AS const LaneState*)sp);
  pass_C<4, WARM, QL_INST_MD, PAIR>(P, c, O, K, st, (FootPtr)Kp->foot);
  if (!st.bad_step) st.iters = st.it;
  priv_store(sp, st);
}
__device__ __noinline__ void call_finish_inst(InstArgs a, QL_PRIV_AS const LaneK<4>* Kp, QL_PRIV_AS const LaneState* sp,
                                              unsigned long long forces, unsigned long long info, unsigned long long traj_u,
                                              unsigned long long traj_x) {
  QL_INST_PARAMS(a);
  const Ctx c = pass_ctx<4>(a.a);
  const WsOff O = make_wsoff<4>(U.N);
  LaneK<4> K;
  priv_load(K, Kp);
  LaneState st;
  priv_load(st, sp);
  lane_finish<4, QL_INST_MD>(P, c, O, K, st, reinterpret_cast<double*>(forces), reinterpret_cast<qmpc_info*>(info),
                          reinterpret_cast<double*>(traj_u), reinterpret_cast<double*>(traj_x));
}
// pi: the instance's expanded block (qmpc_expand_instances_kernel); its instance fields become the lane's rows first (in every
// tick: which lane a robot takes changes with the sort); u_prev (warm units): the robot's previous inputs, or 0 for a cold start
// of this lane
__device__ __noinline__ void call_setup_inst(InstArgs a, unsigned long long rec, unsigned long long pi,
                                             QL_INST_IF_WARM(unsigned long long u_prev,) QL_PRIV_AS LaneK<4>* Kp,
                                             QL_PRIV_AS LaneState* sp) {
  QL_INST_PARAMS(a);
  const Ctx c = pass_ctx<4>(a.a);
  const WsOff O = make_wsoff<4>(U.N);
  lane_params_store(*reinterpret_cast<const DevParams*>(pi), const_cast<QL_GLOBAL_AS double*>(inst_prm(a)), 8u * kLaneWave, a.a.lane8);
  LaneK<4> K;
  LaneState st;
  lane_setup<4, QL_INST_MD>(P, c, O, reinterpret_cast<const double*>(rec), K, st,
                            QL_INST_IF_WARM(__builtin_amdgcn_readfirstlane(a.a.warm) != 0, reinterpret_cast<const double*>(u_prev))
                            QL_INST_IF_COLD(false, nullptr));
  priv_store(Kp, K);
  priv_store(sp, st);
}
// a pass, split across the lane pair where `pair` says so (the pair instantiations exist for the four-point quaternion model only)
#if QL_INST_PAIRS
#define QL_INST_PASS(fn, W, pair) ((pair) ? fn<W, true>(a, Kp, sp) : fn<W, false>(a, Kp, sp))
#else
#define QL_INST_PASS(fn, W, pair) fn<W, false>(a, Kp, sp)
#endif

// qmpc_lane_kernel<4, QL_INST_MD>'s launch with Pi[b] / pstatus[b] (the expanded block and the verdict of instance b) and prm, the
// parameter blocks of the resident wavefronts (LPR_ROWS rows of 64 lanes each).  Same persistent wavefronts, same sort (perm maps a
// position to b: the parameters are indexed by b), 32 or 64 lanes of a wavefront take instances.  A warm unit's kernel takes the
// previous solutions (u_init [batch][N][12]; it may be the buffer traj_u is written to; check_prev: info[b] still holds the record
// of robot b's previous solve) and follows the control flow of qmpc_lane_kernel with previous solutions: the per-lane `usable` rule,
// the WARM instantiations of the passes while some lane of the wavefront still carries a slack residual (rho is exactly 0 after a
// lane's first full step), the cold ones after.  A cold unit's writes traj_x ((N + 1) * 13 per instance, ConvexMpc 12).  With
// pairs: lanes < 0 for lane pairs (half-filled wavefronts; without pairs they run 32 lanes masked) -- -34 every pass split across
// the pair (the cold kernel's only form), -33 the trial pass of the cold rounds only, -32 the cold rounds only --, the iteration
// cap and the hand-off records (a warm launch's carry the rows' initial residuals).  A lane whose record was rejected runs no
// iteration: zero forces and trajectory rows, {QMPC_BAD_PARAMS, 0, ...}, never on the hand-off list.
__global__ __launch_bounds__(kLaneWave) void QL_INST_FN(_kernel)(int pslot, const double* __restrict__ in, const DevParams* __restrict__ Pi,
                                                                const int* __restrict__ pstatus, double* __restrict__ forces,
                                                                qmpc_info* __restrict__ info, int batch, double* __restrict__ ws,
                                                                double* __restrict__ prm, unsigned slots, int lanes,
                                                                const int* __restrict__ perm, QL_INST_IF_WARM(const double* u_init,)
                                                                double* traj_u QL_INST_IF_COLD(, double* traj_x)
                                                                QL_INST_IF_WARM(, int check_prev)
                                                                QL_INST_IF_PAIRS(, int iter_cap, int* __restrict__ hcount,
                                                                                 int* __restrict__ hsel, double* __restrict__ hstate,
                                                                                 int hcap)) {
  // what this flavour's parameter list lacks
#if QL_INST_WARM
  constexpr double* traj_x = nullptr;
#else
  constexpr const double* u_init = nullptr;
#endif
#if !QL_INST_PAIRS
  constexpr int iter_cap = 0, hcap = 0;
  constexpr int *hcount = nullptr, *hsel = nullptr;
  constexpr double* hstate = nullptr;
#endif
  typedef LDim<4> D;
  const int lane = threadIdx.x;
  const DevParams& P = ql_params[pslot];
  const int itmax = (iter_cap > 0 && iter_cap < P.iterations_max) ? iter_cap : P.iterations_max;
  const size_t block_elems = (size_t)make_wsoff<4>(P.N).total * kLaneWave;
  const unsigned long long wsb = reinterpret_cast<unsigned long long>(ws + (size_t)blockIdx.x * block_elems);
  const unsigned long long prb = reinterpret_cast<unsigned long long>(prm + (size_t)blockIdx.x * LPR_ROWS * kLaneWave);
  // the pair forms: pairm -- lane pairs at all; pair_b -- in the cold rounds' factorisation pass too; pair_w -- in the warm rounds
  // (declared here, not with the constants above: moved up, the warm pair kernel gets another register assignment; DESIGN.md 3t)
#if !QL_INST_PAIRS
  constexpr bool pairm = false, pair_b = false, pair_w = false;
#elif QL_INST_WARM
  const bool pairm = lanes <= -32;
  const bool pair_b = lanes == -32 || lanes == -34;
  const bool pair_w = lanes == -34;
#else
  const bool pairm = lanes < 0;      // (the launcher passes -34: a cold launch splits every pass)
  constexpr bool pair_b = true, pair_w = true;
#endif
  QL_INST_IF_PAIRS(if (lanes < 0) lanes = 32;)
  const int lane_i = pairm ? (lane & 31) : lane;
  const InstArgs a = {{pslot, (unsigned)wsb, (unsigned)(wsb >> 32), 8u * (unsigned)lane_i, u_init ? 1u : 0u,
                       pairm ? (unsigned)(lane >> 5) : 0u, pairm ? 0xF8u : 0x1F8u},
                      (unsigned)prb, (unsigned)(prb >> 32)};
  const bool warm = u_init != nullptr;      // kernel argument: scalar
  const size_t tstride = (size_t)P.N * D::NU;
  const size_t xstride = (size_t)(P.N + 1) * (QL_INST_MD == MD_CONVEX ? 12 : 13);
  LaneK<4> K;
  LaneState st;
  QL_PRIV_AS LaneK<4>* Kp = (QL_PRIV_AS LaneK<4>*)&K;
  QL_PRIV_AS LaneState* sp = (QL_PRIV_AS LaneState*)&st;
  for (long long base = (long long)blockIdx.x * lanes; base < batch; base += slots) {
    const long long pos = base + lane_i;
    const bool valid = (pairm || lane < lanes) && pos < batch;
    const int b = valid ? (perm ? perm[pos] : (int)pos) : 0;
    const bool rejected = valid && pstatus[b] != QMPC_OK;
    bool active = false;
    st.status = QMPC_BAD_PARAMS;
    if (valid && !rejected) {
      // the previous solution of this robot is usable unless its last solve failed (the rule of qmpc_lane_kernel)
      QL_INST_IF_WARM(const bool usable = u_init && (!check_prev || info[b].status == QMPC_OK || info[b].status == QMPC_MAX_ITER);)
      call_setup_inst(a, reinterpret_cast<unsigned long long>(in + (size_t)b * D::REC), reinterpret_cast<unsigned long long>(Pi + b),
                      QL_INST_IF_WARM(usable ? reinterpret_cast<unsigned long long>(u_init + (size_t)b * tstride) : 0ull,) Kp, sp);
      active = st.active;
    }
    while (__any(active)) {
      if (active) {
        // one interior-point iteration: the control flow of qmpc_lane_kernel's rounds
        if (warm && __any(st.rho != 0.0)) QL_INST_PASS(call_A_inst, true, pairm && pair_b && pair_w);
        else QL_INST_PASS(call_A_inst, false, pairm && pair_b);
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
          const bool pb = pairm && pair_b;
          const bool okB = wrows ? QL_INST_PASS(call_B_inst, true, pb && pair_w) : QL_INST_PASS(call_B_inst, false, pb);
          if (!okB) { st.status = QMPC_NOT_PD; active = false; }
          else {
            if (wrows) QL_INST_PASS(call_C_inst, true, pairm && pair_w);
            else QL_INST_PASS(call_C_inst, false, pairm);
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
    if (rejected && (!pairm || lane < 32)) {
      for (int j = 0; j < D::NU; ++j) forces[(size_t)b * D::NU + j] = 0.0;
      if (info) {
        const qmpc_info r = {QMPC_BAD_PARAMS, 0, 0.0, 0.0, 0.0, 0.0};
        info[b] = r;
      }
      if (traj_u) for (size_t i = 0; i < tstride; ++i) traj_u[(size_t)b * tstride + i] = 0.0;
      if (traj_x) for (size_t i = 0; i < xstride; ++i) traj_x[(size_t)b * xstride + i] = 0.0;
    }
    if (hcount && valid && !rejected && (!pairm || lane < 32) && itmax < P.iterations_max && st.status == QMPC_MAX_ITER) {
      const int ord = atomicAdd(hcount, 1);
      hsel[ord] = b;
      if (ord < hcap) call_dump<4>(a.a, sp, reinterpret_cast<unsigned long long>(hstate + (size_t)ord * (8 + 84 * (size_t)P.N)), warm ? 1 : 0);
    }
  }
}

#if !QL_INST_WARM
// ---- the sort of a closed-loop tick with controller records ---------------------------------------------------------------------
// The plain loop tick's keys (stance_key with the previous records, contacts at QL_INST_CON_OFF: the stance mask and 16 classes of
// the last iteration count, 256 keys) and one class more, ordered after all of them: robots that will NOT solve in this tick -- a
// rejected record (status[b] != QMPC_OK) or the non-finite word 0 of the record the front kernels give frozen and halted robots.
// Spread over the wavefronts by their stance masks they would shorten none; at the end of the order they fill whole wavefronts,
// which leave after the set-up.  scratch as for qmpc_lane_sort_*: hist[256] | cursor[256] | perm[batch]; the last class is not
// counted: after the scan nothing reads hist any more, and hist[0] becomes its cursor (it begins where the counted keys end).
constexpr unsigned kKeyIdle = 256;
__device__ __forceinline__ unsigned inst_sort_key(const double* __restrict__ in, int b, const qmpc_info* __restrict__ prev,
                                                  const int* __restrict__ status, int idle_last) {
  if (idle_last && (status[b] != QMPC_OK || !isfinite(in[(size_t)b * LDim<4>::REC]))) return kKeyIdle;
  return stance_key<4>(in, b, QL_INST_CON_OFF, prev);
}
__global__ __launch_bounds__(256) void QL_INST_FN(_sort_count)(const double* __restrict__ in, int batch, int* __restrict__ scratch,
                                                              const qmpc_info* __restrict__ prev, const int* __restrict__ status,
                                                              int idle_last) {
  __shared__ int hist[256];
  hist[threadIdx.x] = 0;
  __syncthreads();
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < batch) {
    const unsigned key = inst_sort_key(in, b, prev, status, idle_last);
    if (key < kKeyIdle) atomicAdd(&hist[key], 1);
  }
  __syncthreads();
  if (hist[threadIdx.x]) atomicAdd(&scratch[threadIdx.x], hist[threadIdx.x]);
}
__global__ __launch_bounds__(64) void QL_INST_FN(_sort_scan)(int* __restrict__ scratch) {
  if (threadIdx.x != 0) return;
  int run = 0;
  for (int k = 0; k < 256; ++k) {
    const int n = scratch[k];
    scratch[256 + k] = run;
    run += n;
  }
  scratch[0] = run;      // the cursor of the class that will not solve
}
__global__ __launch_bounds__(256) void QL_INST_FN(_sort_scatter)(const double* __restrict__ in, int batch, int* __restrict__ scratch,
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
    key = inst_sort_key(in, b, prev, status, idle_last);
    rank = atomicAdd(&hist[key], 1);
  }
  __syncthreads();
  if (hist[threadIdx.x]) base[threadIdx.x] = atomicAdd(&scratch[256 + threadIdx.x], hist[threadIdx.x]);
  if (threadIdx.x == 0 && hist[kKeyIdle]) base[kKeyIdle] = atomicAdd(&scratch[0], hist[kKeyIdle]);
  __syncthreads();
  if (b < batch) scratch[512 + base[key] + rank] = b;
}
#endif

}  // namespace lane
}  // namespace qmpc

// ---- the hidden launchers: one signature in every unit (qmpc_hip.hip keeps them in a table); a unit ignores the trailing
// arguments its kernel does not take ------------------------------------------------------------------------------------------
#if QL_UNIT == 3
__attribute__((visibility("hidden"))) size_t qmpc_lane_inst_param_bytes(unsigned slots) {
  return sizeof(double) * (size_t)LPR_ROWS * (size_t)slots;
}
#endif
// The launch of qmpc_lane_kernel<4, QL_INST_MD> (qmpc_lane_launch) for per-instance records in two parts.  The upload: the handle's
// block into this unit's table (once per closed-loop call, outside its capture; before every launch of a solve call).
__attribute__((visibility("hidden"))) hipError_t QL_INST_FN(_upload_params)(int pslot, hipStream_t s, const void* dev_params,
                                                                           size_t dev_params_size) {
  if (dev_params_size != sizeof(DevParams) || pslot < 0 || pslot >= kParamSlots) return hipErrorInvalidValue;
  return hipMemcpyToSymbolAsync(HIP_SYMBOL(ql_params), dev_params, sizeof(DevParams), sizeof(DevParams) * (size_t)pslot,
                                hipMemcpyHostToDevice, s);
}
// ... and the launch (with pairs the hand-off counter's memset, then the kernel: capturable): dev_blocks / status are the expansion
// kernel's outputs, prm qmpc_lane_inst_param_bytes(slots) bytes, perm the sort's permutation (qmpc_lane_sort_launch, <name>_sort_launch)
// or null; u_init: the previous solutions, traj_u the buffer this launch's go to (it may be u_init); pair: QMPC_LANE_PAIR, with the
// meaning it has for the plain tick of the same start (qmpc_lane_launch).
__attribute__((visibility("hidden"))) hipError_t QL_INST_FN(_launch_only)(int pslot, int batch, hipStream_t s, const void* in,
                                                                         const void* dev_blocks, const int* status, double* forces,
                                                                         qmpc_info* info, double* ws, double* prm, unsigned slots,
                                                                         const int* perm, const double* u_init, double* traj_u,
                                                                         double* traj_x, int check_prev, int iter_cap, int* hcount,
                                                                         int* hsel, double* hstate, int hcap, int pair) {
  if (slots % kLaneWave || pslot < 0 || pslot >= kParamSlots) return hipErrorInvalidValue;
#if QL_INST_PAIRS
  if (hcount) {
    const hipError_t e = hipMemsetAsync(hcount, 0, 2 * sizeof(int), s);      // the list's length and the list kernel's cursor
    if (e != hipSuccess) return e;
  }
#else
  if (batch < 1) return hipErrorInvalidValue;
#endif
  // (the rule of qmpc_lane_launch) batches that would occupy at most half of the chip's SIMDs with full wavefronts run with 32
  // lanes per wavefront: as lane pairs unless QMPC_LANE_PAIR=0, without pairs the other half masked
  const int lanes = (size_t)batch * 2 <= slots ? 32 : 64;
  const unsigned need = (unsigned)(((size_t)batch + lanes - 1) / lanes);
  const unsigned waves = need < slots / kLaneWave ? need : slots / kLaneWave;
  const unsigned used = waves * (unsigned)lanes;
  const size_t lds = sizeof(double) * kLaneWave * LDim<4>::PLDS;
#if !QL_INST_PAIRS
  const int lanes_arg = lanes;
#elif QL_INST_WARM
  const int lanes_arg = (lanes == 32 && pair) ? (pair == 2 ? -33 : (pair == 4 ? -32 : -34)) : lanes;
#else
  const int lanes_arg = (lanes == 32 && pair) ? -34 : lanes;
#endif
  hipLaunchKernelGGL(QL_INST_FN(_kernel), dim3(waves), dim3(kLaneWave), lds, s, pslot, static_cast<const double*>(in),
                     static_cast<const DevParams*>(dev_blocks), status, forces, info, batch, ws, prm, used, lanes_arg, perm,
                     QL_INST_IF_WARM(u_init,) traj_u QL_INST_IF_COLD(, traj_x) QL_INST_IF_WARM(, check_prev)
                     QL_INST_IF_PAIRS(, iter_cap, hcount, hsel, hstate, hcap));
  return hipGetLastError();
}
#if !QL_INST_WARM
// The sort of a tick (scratch: qmpc_lane_scratch_bytes(batch) bytes; the permutation is left at scratch + 512).  prev: the previous
// solves' records (the handle's output buffer) or null; status: the expansion's verdicts; idle_last = 0: the plain tick's keys for
// every robot (status is not read) -- ConvexMpc's plain call, or QMPC_LANE_SORT_IDLE=0.
__attribute__((visibility("hidden"))) hipError_t QL_INST_FN(_sort_launch)(int batch, hipStream_t s, const void* in, const qmpc_info* prev,
                                                                         const int* status, int idle_last, int* scratch) {
  const double* rec = static_cast<const double*>(in);
  const hipError_t e = hipMemsetAsync(scratch, 0, sizeof(int) * 512, s);
  if (e != hipSuccess) return e;
  const unsigned blocks = (unsigned)((batch + 255) / 256);
  hipLaunchKernelGGL(QL_INST_FN(_sort_count), dim3(blocks), dim3(256), 0, s, rec, batch, scratch, prev, status, idle_last);
  hipLaunchKernelGGL(QL_INST_FN(_sort_scan), dim3(1), dim3(64), 0, s, scratch);
  hipLaunchKernelGGL(QL_INST_FN(_sort_scatter), dim3(blocks), dim3(256), 0, s, rec, batch, scratch, prev, status, idle_last);
  return hipGetLastError();
}
#endif
