// lane_cinst_warm_host.cpp -- TEST INFRASTRUCTURE: g++ build of the lane-per-instance solver core of ConvexMpc's problem with
// PER-LANE parameters, WARM-STARTED (quaternion-mpc_amd/csrc/qmpc_lane_core.h: the LaneParams / MD_CONVEX instantiation of the
// passes with warm = true, the text hipcc compiles into qmpc_lane_cinst_warm_kernel), one instance after the other with unit
// strides, in the pattern of lane_cinst_host.cpp.  u_init / traj_u: [batch][N][12], u_init null for a cold solve; check_prev: info
// holds the records of the instances' previous solves, and a failed one starts cold (the kernels' `usable` rule).  It also exports
// the plain warm core (DevParams instantiation) for the byte comparison of tests/test_convex_warm_records_cpu.py; nothing in the
// product loads it.
#include <cstring>
#include <vector>

#include "../../quaternion-mpc_amd/csrc/qmpc_lane_core.h"

using namespace qmpc;
using namespace qmpc::lane;

template <class PT>
static void solve_one(const PT& P, int N, std::vector<double>& ws, std::vector<double>& pl, const double* rec, const double* u_prev,
                      double* forces, qmpc_info* info, double* traj_u) {
  const WsOff O = make_wsoff<4>(N);
  Ctx c = {ws.data(), 8, 0, pl.data(), 8, 0};
  LaneK<4> K;
  LaneState st;
  const bool warm = u_prev != nullptr;
  lane_setup<4, MD_CONVEX>(P, c, O, rec, K, st, warm, u_prev);
  if (st.active)
    while (lane_iteration<4, MD_CONVEX>(P, c, O, K, st, warm)) {}
  lane_finish<4, MD_CONVEX>(P, c, O, K, st, forces, info, traj_u);
}

static bool usable(const double* u_init, int check_prev, const qmpc_info* info, int b) {
  return u_init && (!check_prev || info[b].status == QMPC_OK || info[b].status == QMPC_MAX_ITER);
}

// the plain core, warm-started, one instance after the other (ConvexMpc's problem in the converged mode)
extern "C" int lane_host_convex_solve_warm(const qmpc_params* p, int batch, const double* rec, const double* u_init, int check_prev,
                                           double* forces, qmpc_info* info, double* traj_u) {
  DevParams P;
  const int st = fill_dev_params(p, &P);
  if (st != QMPC_OK) return st;
  if (p->model != QMPC_MODEL_CONVEX || p->mode != QMPC_MODE_CONVERGED || !info || !traj_u) return QMPC_BAD_ARGUMENT;
  const size_t ts = (size_t)P.N * 12;
  std::vector<double> ws((size_t)make_wsoff<4>(P.N).total), pl((size_t)LDim<4>::PLDS);
  for (int b = 0; b < batch; ++b)
    solve_one(P, P.N, ws, pl, rec + (size_t)b * LDim<4>::REC, usable(u_init, check_prev, info, b) ? u_init + b * ts : nullptr,
              forces + (size_t)b * 12, info + b, traj_u + b * ts);
  return QMPC_OK;
}

// per-instance records on the per-lane-parameter instantiation, warm-started
extern "C" int lane_host_convex_solve_instances_warm(const qmpc_params* p, int batch, const double* rec, const qmpc_instance_params* iparams,
                                                     const double* u_init, int check_prev, double* forces, qmpc_info* info,
                                                     double* traj_u) {
  DevParams P;
  const int st = fill_dev_params(p, &P);
  if (st != QMPC_OK) return st;
  if (p->model != QMPC_MODEL_CONVEX || p->mode != QMPC_MODE_CONVERGED || !info || !traj_u) return QMPC_BAD_ARGUMENT;
  const size_t ts = (size_t)P.N * 12;
  std::vector<double> ws((size_t)make_wsoff<4>(P.N).total), pl((size_t)LDim<4>::PLDS), prm((size_t)LPR_ROWS);
  for (int b = 0; b < batch; ++b) {
    DevParams Pi;
    if (apply_instance_params(P, iparams[b], &Pi) != QMPC_OK) {      // a rejected record: no iteration (qmpc_lane_cinst_warm_kernel)
      for (int i = 0; i < 12; ++i) forces[(size_t)b * 12 + i] = 0.0;
      const qmpc_info r = {QMPC_BAD_PARAMS, 0, 0.0, 0.0, 0.0, 0.0};
      info[b] = r;
      for (size_t i = 0; i < ts; ++i) traj_u[b * ts + i] = 0.0;
      continue;
    }
    lane_params_store(Pi, prm.data(), 8, 0);
    // the uniform block is the HANDLE's: an instance field read from it instead of the lane's rows shows as a difference
    const LaneParams LP(P, prm.data(), 8, 0);
    solve_one(LP, P.N, ws, pl, rec + (size_t)b * LDim<4>::REC, usable(u_init, check_prev, info, b) ? u_init + b * ts : nullptr,
              forces + (size_t)b * 12, info + b, traj_u + b * ts);
  }
  return QMPC_OK;
}
