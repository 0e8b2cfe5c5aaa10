// qmpc_ref_body.inc -- the body of one reference-mode solve (AL-iLQR, qmpc_ref.hip), textually included by
// qmpc_ref_kernel and, inside a lambda, by the closed loop's persistent kernel (qmpc_loop.hip) -- like
// qmpc_solve_body.inc.  Names expected in scope: template parameters MD, VAR;  DevParams P;  const qmpc_input* in_;
// double* forces;  qmpc_info* info;  double* traj_u, * traj_x;  double* gws;  int b, lane;  double sm[].
  typedef typename MD::D D;
  constexpr int NU = D::NU, NC = D::NC;
  const int N = P.N;
  constexpr bool KDG = VAR >= 1;
  constexpr bool LEAN = KDG || MD::NL != 4;
  const Layout L = make_layout(N, KDG, MD::NL, false);
  const size_t slice = (size_t)N * (D::KD + D::ROT);
  double* KD = KDG ? gws + (size_t)b * slice : sm + L.KD;
  double* ROT = KDG ? KD + N * D::KD : sm + L.ROT;
  double* sl = sm;
  const void* in = reinterpret_cast<const double*>(in_) + (size_t)b * ((MD::NX == 13) ? D::REC : 48);
  int status = QMPC_OK;
  Prof<false> prof;
  setup_instance<MD>(P, L, sm, in, lane, &status);
  if (status != QMPC_OK) {
    if (lane < NU) forces[NU * (size_t)b + lane] = 0.0;
    if (lane == 0 && info) {
      qmpc_info r = {status, 0, 0.0, 0.0, 0.0, 0.0};
      info[b] = r;
    }
    if (traj_u) for (int i = lane; i < N * NU; i += kWave) traj_u[(size_t)b * N * NU + i] = 0.0;
    if (traj_x) for (int i = lane; i < (N + 1) * MD::NX; i += kWave) traj_x[(size_t)b * (N + 1) * MD::NX + i] = 0.0;
    return;
  }
  unsigned conmask = 0;
  for (int l = 0; l < MD::NL; ++l) conmask |= (sm[L.cst + D::C_CON + l] != 0.0) ? (1u << l) : 0u;
  conmask = __builtin_amdgcn_readfirstlane(conmask);
  // QuatMpc's four-point problem: the stationarity test runs the row-parallel costate sweep of qmpc_wform.h (its 0.0
  // operand slots behind the instance constants, the input weights and the per-knot 6-vectors in the unused DLAM / DS slots)
  constexpr bool WSTAT = MD::NL == 4 && MD::NX == 13;
  // four contact points (QuatMpc and ConvexMpc): the line search tries three step lengths per rollout (rollout_trials_dense)
  constexpr bool WLS = MD::NL == 4;
  if (WSTAT && lane < 10) sm[L.cst + kZeroSlots + lane] = 0.0;
  if (WLS && lane < 12) sl[L.DLAM + N * NC - 12 + lane] = P.R[lane];
  const double* Rl = sl + L.DLAM + N * NC - 12;
  for (int i = lane; i < N * NU; i += kWave) sm[L.U + i] = sm[L.uref + (i % NU)];
  for (int i = lane; i < N * NC; i += kWave) sl[L.LAM + i] = 0.0;
  QSYNC();
  rollout_open<MD, LEAN>(P, L, sm, lane);
  expansions<MD>(P, L, sm, lane);
  ref_cone_refresh<D>(P, L, sm, sl, conmask, lane);
  QSYNC();
  double rho = P.penalty_initial;
  double Jplain = 0.0, viol = 0.0;
  double J = ref_merit<MD, false>(P, L, sm, sl, rho, conmask, lane, &Jplain, &viol);
  int iter = 0;
  double last_step = 0.0;
  status = QMPC_MAX_ITER;
  for (iter = 1; iter <= P.iterations_max; ++iter) {
    rotation_prepass<D, true>(P, L, sm, sl, ROT, rho, lane);
    if (KDG) __syncthreads();
    double dV1 = 0.0;
    if (backward_pass<MD, false, !KDG, (D::TU > 1)>(P, L, sm, KD, ROT, lane, conmask, prof, &dV1)) {
      status = QMPC_NOT_PD;
      --iter;
      break;
    }
    if (KDG) __syncthreads();
    // forward pass: backtracking line search on the AL merit
    double alpha = 1.0, Jn = J, Jn_plain = Jplain, vn = viol;
    bool accepted = false;
    if constexpr (WLS) {
      // three trial step lengths per rollout (rollout_trials_dense), tested in the order of the backtracking sequence
      int gacc = 0;
      for (int ls = 0; ls <= P.linesearch_max && !accepted; ls += 3) {
        const int grp = (lane >> 4) < 2 ? (lane >> 4) : 2;
        const double ag = alpha * (grp == 0 ? 1.0 : (grp == 1 ? 0.5 : 0.25));
        const double Jx = rollout_trials_dense<MD, LEAN>(P, L, sm, KD, ROT, ag, lane);
        double Ju[3], mer[3], vi[3];
        trial_inputs_dense<D>(P, L, sm, sl, Rl, rho, lane, Ju, mer, vi);
#pragma unroll
        for (int g = 0; g < 3; ++g) {
          if (accepted || ls + g > P.linesearch_max) continue;
          const double a_g = alpha * (g == 0 ? 1.0 : (g == 1 ? 0.5 : 0.25));
          const double Jxg = read_lane(Jx, 16 * g);
          const double Jg = Jxg + wave_sum(mer[g]);
          const double expected = a_g * dV1;
          const double slack = 1e-12 * fmax(1.0, fabs(J));
          if (isfinite(Jg) && Jg - J <= 1e-4 * expected + slack) {
            accepted = true; gacc = g; Jn = Jg; Jn_plain = Jxg + wave_sum(Ju[g]); vn = wave_max(vi[g]);
          }
        }
        if (accepted) {
          alpha *= (gacc == 0 ? 1.0 : (gacc == 1 ? 0.5 : 0.25));
          if (gacc != 0) {      // the accepted group's increments and states into dU / Xc (group 0 rolled there directly)
            const double* ds = sm + trial_du_slot(L, gacc);
            const double* xs = sm + trial_x_slot(L, gacc);
            for (int i = lane; i < NU * N; i += kWave) sm[L.dU + i] = ds[i];
            for (int i = lane; i < 13 * N; i += kWave) sm[L.Xc + 13 + i] = xs[i];
            QSYNC();
          }
        } else {
          alpha *= 0.125;
        }
      }
    } else {
    for (int ls = 0; ls <= P.linesearch_max; ++ls) {
      rollout_closed<MD, !KDG, LEAN, false>(P, L, sm, KD, ROT, alpha, lane, prof);
      Jn = ref_merit<MD, true>(P, L, sm, sl, rho, conmask, lane, &Jn_plain, &vn);
      const double expected = alpha * dV1;
      const double slack = 1e-12 * fmax(1.0, fabs(J));
      if (isfinite(Jn) && Jn - J <= 1e-4 * expected + slack) { accepted = true; break; }
      alpha *= 0.5;
    }
    }
    if (!accepted) {
      status = QMPC_LINESEARCH_FAIL;
      --iter;
      break;
    }
    double step = 0.0;
    for (int i = lane; i < N * NU; i += kWave) {
      step = fmax(step, fabs(sm[L.dU + i]));
      sm[L.U + i] += sm[L.dU + i];
    }
    for (int i = lane; i < (N + 1) * 13; i += kWave) sm[L.X + i] = sm[L.Xc + i];
    last_step = wave_max(step);
    QSYNC();
    const double dJ = J - Jn;
    J = Jn; Jplain = Jn_plain; viol = vn;
    expansions<MD>(P, L, sm, lane);
    ref_cone_refresh<D>(P, L, sm, sl, conmask, lane);
    QSYNC();
    double stat;
    if constexpr (WSTAT) stat = stationarity_w(P, L, sm, sl, sl + L.DS, Rl, rho, conmask, lane);
    else stat = ref_stationarity<MD>(P, L, sm, sl, rho, conmask, lane);
    if (stat < P.tol_stat && viol < P.tol_feas) {
      status = QMPC_OK;
      break;
    }
    if (stat < P.tol_stat || fabs(dJ) < P.tol_cost_int) {
      for (int i = lane; i < N * NC; i += kWave) {       // lambda <- max(lambda + rho c, 0)
        const double z = sl[L.LAM + i] + rho * sl[L.RC + i];
        sl[L.LAM + i] = (z > 0.0) ? z : 0.0;
      }
      rho = fmin(rho * P.penalty_scaling, P.penalty_max);
      QSYNC();
      J = ref_merit<MD, false>(P, L, sm, sl, rho, conmask, lane, &Jplain, &viol);
    }
  }
  if (iter > P.iterations_max) iter = P.iterations_max;
  if (lane < NU) forces[NU * (size_t)b + lane] = sm[L.U + lane];
  if (traj_u) for (int i = lane; i < N * NU; i += kWave) traj_u[(size_t)b * N * NU + i] = sm[L.U + i];
  if (traj_x)
    for (int i = lane; i < (N + 1) * MD::NX; i += kWave) {
      const int k = i / MD::NX, j = i - MD::NX * k;
      traj_x[(size_t)b * (N + 1) * MD::NX + i] = sm[L.X + 13 * k + j];
    }
  if (info && lane == 0) {
    qmpc_info r = {status, iter, Jplain, viol, last_step, rho};
    info[b] = r;
  }
