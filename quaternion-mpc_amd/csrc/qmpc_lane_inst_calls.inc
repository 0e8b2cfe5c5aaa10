// qmpc_lane_inst_calls.inc -- what the lane units with per-lane robot and cost parameters share, defined once: the passes of
// qmpc_lane_kernel<4, QL_INST_MD> instantiated on LaneParams (qmpc_lane_core.h) as separate functions, and the arguments they are
// called with.  QL_INST_MD is the including unit's model: MD_QUAT in qmpc_lane_inst.hip (QL_UNIT 3: the cold kernel, WARM = false
// throughout) and qmpc_lane_inst_warm.hip (QL_UNIT 4), MD_CONVEX in qmpc_lane_cinst.hip (QL_UNIT 5: ConvexMpc's cold kernel, which
// has no pair forms) and qmpc_lane_cinst_warm.hip (QL_UNIT 6: that kernel warm-started).  Included inside namespace qmpc::lane, after qmpc_lane.hip.  Textual inclusion: each unit instantiates what
// it calls and keeps its own code object (tools/isa_same.py states unit 3's against a revision).  The set-up differs between the
// units (cold: no previous solution) and stays with its unit.
#if !defined(QL_INST_MD)
#error "QL_INST_MD: the model of the including unit (MD_QUAT or MD_CONVEX)"
#endif
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
