// qmpc_params_dev.h -- DevParams: the kernels' by-value copy of qmpc_params plus derived constants.
// No HIP dependency: the lane-per-instance core (qmpc_lane_core.h) is also compiled by g++ for its CPU numerics
// test, which needs the same structure.
#pragma once

#include <cmath>
#include <cstring>

#include "../../include/qmpc.h"

// the helpers the expansion kernel of qmpc_solve_instances (qmpc_wform.hip) shares with the host: one source for both
#if defined(__HIPCC__)
#define QP_HD __host__ __device__
#else
#define QP_HD
#endif

namespace qmpc {

// Device copy of qmpc_params plus derived constants (host fills it).
struct DevParams {
  int N;
  int mode;
  int iterations_max;
  int drop_ang_vel;
  double h;        // (double)(float h)
  double hh;       // (double)(h/2) with h float
  double h_ref;
  double mass;
  double inv_mass;
  double Iinv[9];
  double Q[13];
  double R[12];
  double w;
  double mu;
  double fz_max;
  double tol_feas, tol_step, mu0, mu_final, sigma, sigma_fast, tau;
  // reference mode (AL-iLQR, QuatMpc.cpp:21-26 + upstream ALTRO defaults)
  double penalty_initial, penalty_scaling, penalty_max, tol_stat, tol_cost_int;
  int linesearch_max;
};

// 1 / mass and the cofactor inverse of the 3x3 inertia (Eigen's fixed-size inverse(), AltroUtils.cpp:391); false: singular.
// Contraction off: the host (fill_dev_params) and the device (qmpc_expand_instances_kernel) round every product alike.
QP_HD inline bool derive_inertial(double mass, const double* A, double* inv_mass, double* Iinv) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  *inv_mass = 1.0 / mass;
  const double c00 = A[4] * A[8] - A[5] * A[7], c01 = A[5] * A[6] - A[3] * A[8], c02 = A[3] * A[7] - A[4] * A[6];
  const double det = A[0] * c00 + A[1] * c01 + A[2] * c02;
  if (!(__builtin_fabs(det) > 0.0)) return false;
  const double id = 1.0 / det;
  Iinv[0] = c00 * id; Iinv[1] = (A[2] * A[7] - A[1] * A[8]) * id; Iinv[2] = (A[1] * A[5] - A[2] * A[4]) * id;
  Iinv[3] = c01 * id; Iinv[4] = (A[0] * A[8] - A[2] * A[6]) * id; Iinv[5] = (A[2] * A[3] - A[0] * A[5]) * id;
  Iinv[6] = c02 * id; Iinv[7] = (A[1] * A[6] - A[0] * A[7]) * id; Iinv[8] = (A[0] * A[4] - A[1] * A[3]) * id;
  return true;
}

// The handle's DevParams with the seven fields of a per-instance record (qmpc_solve_instances) in place, and the record's
// verdict: QMPC_OK, or QMPC_BAD_PARAMS for a non-finite field, mass <= 0, a singular inertia, an r_weight <= 0, a negative
// q_weight or w, mu <= 0 or fz_max <= 0 (*d is written either way).
QP_HD inline int apply_instance_params(const DevParams& base, const qmpc_instance_params& r, DevParams* d) {
  *d = base;
  const double* v = &r.mass;      // the record is 38 doubles
  bool ok = true;
  for (int i = 0; i < (int)(sizeof r / sizeof(double)); ++i) ok = ok && __builtin_isfinite(v[i]);
  d->mass = r.mass;
  ok = derive_inertial(r.mass, r.inertia, &d->inv_mass, d->Iinv) && ok;
  ok = ok && r.mass > 0.0 && r.mu > 0.0 && r.fz_max > 0.0 && r.w >= 0.0;
  for (int j = 0; j < 13; ++j) { d->Q[j] = r.q_weights[j]; ok = ok && r.q_weights[j] >= 0.0; }
  for (int j = 0; j < 12; ++j) { d->R[j] = r.r_weights[j]; ok = ok && r.r_weights[j] > 0.0; }
  d->w = r.w;
  d->mu = r.mu;
  d->fz_max = r.fz_max;
  return ok ? QMPC_OK : QMPC_BAD_PARAMS;
}

// One robot's TRUE plant in the closed loop with per-robot records (qmpc_loop_run_instances*), as the kernels read it: the mass,
// the inverse inertia (derive_inertial: bit-identical to DevParams::Iinv for the same inertia), the constant disturbance
// wrench and the robot's verdict (QMPC_OK, or QMPC_BAD_PARAMS: the robot is frozen).  136 B.
struct PlantDev {
  double mass;
  double Iinv[9];
  double force[3];     // world frame, at the CoM [N]
  double torque[3];    // body frame [N m]
  int status;
  int pad_;
};

// A plant record -> PlantDev (*d is written either way) and its verdict: QMPC_OK, or QMPC_BAD_PARAMS for a non-finite
// field, mass <= 0 or a singular inertia.
QP_HD inline int apply_plant_params(const qmpc_plant_params& r, PlantDev* d) {
  const double* v = &r.mass;      // the record is 16 doubles
  bool ok = true;
  for (int i = 0; i < (int)(sizeof r / sizeof(double)); ++i) ok = ok && __builtin_isfinite(v[i]);
  double inv_mass;
  d->mass = r.mass;
  ok = derive_inertial(r.mass, r.inertia, &inv_mass, d->Iinv) && ok;
  ok = ok && r.mass > 0.0;
  for (int a = 0; a < 3; ++a) { d->force[a] = r.ext_force_world[a]; d->torque[a] = r.ext_torque_body[a]; }
  d->status = ok ? QMPC_OK : QMPC_BAD_PARAMS;
  d->pad_ = 0;
  return d->status;
}

// qmpc_params -> DevParams; QMPC_OK or QMPC_BAD_ARGUMENT
inline int fill_dev_params(const qmpc_params* p, DevParams* d) {
  if (!p || p->horizon < 1 || p->horizon > QMPC_MAX_HORIZON) return QMPC_BAD_ARGUMENT;
  if (p->mode != QMPC_MODE_CONVERGED && p->mode != QMPC_MODE_REFERENCE) return QMPC_BAD_ARGUMENT;
  if (p->mode == QMPC_MODE_REFERENCE && !(p->penalty_initial > 0.0 && p->penalty_scaling >= 1.0)) return QMPC_BAD_ARGUMENT;
  if (p->model != QMPC_MODEL_QUAT && p->model != QMPC_MODEL_CONVEX && p->model != QMPC_MODEL_QUAT8)
    return QMPC_BAD_ARGUMENT;
  if (!(p->mass > 0.0) || !(p->h > 0.0f)) return QMPC_BAD_ARGUMENT;
  if (p->mode == QMPC_MODE_CONVERGED && !(p->ipm_mu0 > 0.0)) return QMPC_BAD_ARGUMENT;
  std::memset(d, 0, sizeof *d);
  d->N = p->horizon;
  d->mode = p->mode;
  d->iterations_max = p->iterations_max;
  d->drop_ang_vel = p->drop_ang_vel;
  d->h = (double)p->h;
  d->hh = (double)(p->h / 2);  // float division, as `h / 2` in AltroUtils.cpp:16,94
  d->h_ref = p->h_ref;
  d->mass = p->mass;
  if (!derive_inertial(p->mass, p->inertia, &d->inv_mass, d->Iinv)) return QMPC_BAD_ARGUMENT;
  std::memcpy(d->Q, p->q_weights, sizeof d->Q);
  std::memcpy(d->R, p->r_weights, sizeof d->R);
  for (int j = 0; j < 12; ++j) if (!(d->R[j] > 0.0)) return QMPC_BAD_ARGUMENT;
  d->w = p->w;
  d->mu = p->mu;
  d->fz_max = p->fz_max;
  d->tol_feas = p->tol_feasibility;
  d->tol_step = p->tol_step;
  d->mu0 = p->ipm_mu0;
  d->mu_final = p->ipm_mu_final;
  d->sigma = p->ipm_sigma;
  d->sigma_fast = p->ipm_sigma_fast;
  d->tau = p->ipm_tau;
  d->penalty_initial = p->penalty_initial;
  d->penalty_scaling = p->penalty_scaling;
  d->penalty_max = p->penalty_max;
  d->tol_stat = p->tol_stationarity;
  d->tol_cost_int = p->tol_cost_intermediate;
  d->linesearch_max = p->linesearch_max;
  return QMPC_OK;
}

}  // namespace qmpc
