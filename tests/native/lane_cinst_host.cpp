// lane_cinst_host.cpp -- TEST INFRASTRUCTURE: g++ build of the lane-per-instance solver core of ConvexMpc's problem with PER-LANE
// parameters (quaternion-mpc_amd/csrc/qmpc_lane_core.h: the LaneParams / MD_CONVEX instantiation of the passes, the text hipcc
// compiles into qmpc_lane_cinst_kernel), one instance after the other with unit strides.  The records are expanded with
// apply_instance_params, as qmpc_expand_instances_kernel does, and the instance fields go through the parameter block, as on
// the device.  It also exports the plain core (DevParams instantiation) for the byte comparison of
// tests/test_convex_instance_lane_cpu.py; nothing in the product loads it.
#include <cstring>
#include <vector>

#include "../../quaternion-mpc_amd/csrc/qmpc_lane_core.h"

using namespace qmpc;
using namespace qmpc::lane;

template <class PT>
static void solve_one(const PT& P, int N, std::vector<double>& ws, std::vector<double>& pl, const double* rec, double* forces,
                      qmpc_info* info) {
  const WsOff O = make_wsoff<4>(N);
  Ctx c = {ws.data(), 8, 0, pl.data(), 8, 0};
  LaneK<4> K;
  LaneState st;
  lane_setup<4, MD_CONVEX>(P, c, O, rec, K, st);
  if (st.active)
    while (lane_iteration<4, MD_CONVEX>(P, c, O, K, st)) {}
  lane_finish<4, MD_CONVEX>(P, c, O, K, st, forces, info, nullptr);
}

// the plain core, one instance after the other (ConvexMpc's problem in the converged mode)
extern "C" int lane_host_convex_solve(const qmpc_params* p, int batch, const double* rec, double* forces, qmpc_info* info) {
  DevParams P;
  const int st = fill_dev_params(p, &P);
  if (st != QMPC_OK) return st;
  if (p->model != QMPC_MODEL_CONVEX || p->mode != QMPC_MODE_CONVERGED) return QMPC_BAD_ARGUMENT;
  std::vector<double> ws((size_t)make_wsoff<4>(P.N).total), pl((size_t)LDim<4>::PLDS);
  for (int b = 0; b < batch; ++b) solve_one(P, P.N, ws, pl, rec + (size_t)b * LDim<4>::REC, forces + (size_t)b * 12, info ? info + b : nullptr);
  return QMPC_OK;
}

// per-instance records on the per-lane-parameter instantiation
extern "C" int lane_host_convex_solve_instances(const qmpc_params* p, int batch, const double* rec, const qmpc_instance_params* iparams,
                                                double* forces, qmpc_info* info) {
  DevParams P;
  const int st = fill_dev_params(p, &P);
  if (st != QMPC_OK) return st;
  if (p->model != QMPC_MODEL_CONVEX || p->mode != QMPC_MODE_CONVERGED) return QMPC_BAD_ARGUMENT;
  std::vector<double> ws((size_t)make_wsoff<4>(P.N).total), pl((size_t)LDim<4>::PLDS), prm((size_t)LPR_ROWS);
  for (int b = 0; b < batch; ++b) {
    DevParams Pi;
    if (apply_instance_params(P, iparams[b], &Pi) != QMPC_OK) {      // a rejected record: no iteration (qmpc_lane_cinst_kernel)
      for (int i = 0; i < 12; ++i) forces[(size_t)b * 12 + i] = 0.0;
      if (info) {
        const qmpc_info r = {QMPC_BAD_PARAMS, 0, 0.0, 0.0, 0.0, 0.0};
        info[b] = r;
      }
      continue;
    }
    lane_params_store(Pi, prm.data(), 8, 0);
    // the uniform block is the HANDLE's: an instance field read from it instead of the lane's rows shows as a difference
    const LaneParams LP(P, prm.data(), 8, 0);
    solve_one(LP, P.N, ws, pl, rec + (size_t)b * LDim<4>::REC, forces + (size_t)b * 12, info ? info + b : nullptr);
  }
  return QMPC_OK;
}
