// qmpc_wform_ref_body.inc -- the body of one REFERENCE-MODE solve (the reference's own AL-iLQR scheme: iterations_max = 10,
// penalty_scaling = 20, backtracking line search, status ignored; QuatMpc.cpp:21-26,256; qmpc_ref.hip has the scheme) on the
// wrench-form algebra of qmpc_wform.h: the counterpart of qmpc_ref_body.inc for QuatMpc's problem with four contact points.
// Same control flow and the same helper routines (ref_cone_refresh, ref_merit, ref_stationarity of qmpc_ref.hip); the
// backward pass, the rollouts of the line search and the input recovery are the wrench-form ones, with augmented-Lagrangian
// weights in the per-point pre-pass and the step length alpha scaling the feed-forward parts.  Names expected in scope:
//   WVAR (3: everything in LDS; 5: gains / per-point records / per-knot blocks in the workspace);  DevParams P;
//   const qmpc_input* in_;  double* forces;  qmpc_info* info;  double* traj_u, * traj_x;  double* gws;  int wslot, b, lane;
//   double sm[].  Slot use: LAM = lambda, RC = c(U), S = candidate inputs (scratch), DS = y0 of the backward pass (6 per knot).
#ifndef QMPC_WMODEL
#define QMPC_WMODEL WM_QUAT      // WM_CONVEX: ConvexMpc's problem (its own mode: five AL-iLQR iterations, ConvexMpc.cpp:36-38)
#define QMPC_WMODEL_DEFAULTED 1
#endif
#ifndef QMPC_WNL
#define QMPC_WNL 4               // 8: the eight-contact-point model (full layout: the direction slots hold y0 / costates / trial states here)
#define QMPC_WNL_DEFAULTED 1
#endif
  constexpr int WMT = QMPC_WMODEL;
  constexpr int WNL = QMPC_WNL;
  typedef typename std::conditional<WMT == WM_CONVEX, ConvexModel, typename std::conditional<WNL == 8, Quat8Model, QuatModel>::type>::type WMD;
  typedef Dim<WNL> WD;
  constexpr int NU = WD::NU, NC = WD::NC;
  const int N = P.N;
  constexpr bool KDG = WVAR == 5;
  LayoutW LW;
  const Layout L = make_layout_w<WNL>(N, &LW, KDG, false, WMT == WM_CONVEX, true);
  double* wsb = KDG ? gws + (size_t)wslot * wform_slice<WNL>(N) : sm;
  double* KD = wsb + L.KD;
  double* ROT = wsb + L.ROT;
  double* GK = wsb + LW.GK;
  double* sl = sm;
  double* Y0 = sm + L.DS;
  const void* in = reinterpret_cast<const double*>(in_) + (size_t)b * WD::REC;
  int status = QMPC_OK;
  Prof<false> prof;
  setup_instance<WMD>(P, L, sm, in, lane, &status);
  if (status != QMPC_OK) {
    if (lane < NU) forces[NU * (size_t)b + lane] = 0.0;
    if (lane == 0 && info) {
      qmpc_info r = {status, 0, 0.0, 0.0, 0.0, 0.0};
      info[b] = r;
    }
    if (traj_u) for (int i = lane; i < N * NU; i += kWave) traj_u[(size_t)b * N * NU + i] = 0.0;
    if (traj_x) for (int i = lane; i < (N + 1) * WMD::NX; i += kWave) traj_x[(size_t)b * (N + 1) * WMD::NX + i] = 0.0;
    return;
  }
  unsigned conmask = 0;
  for (int l = 0; l < WMD::NL; ++l) conmask |= (sm[L.cst + WD::C_CON + l] != 0.0) ? (1u << l) : 0u;
  conmask = __builtin_amdgcn_readfirstlane(conmask);
  double* Rl = sm + L.DLAM + 13 * N;      // the input weights R (one per input), behind the trial states kept in this slot
  if (lane < NU) Rl[lane] = P.R[lane % 12];
  if (lane < 10) sm[L.cst + kZeroSlotsT<WNL>() + lane] = 0.0;
  if (lane == 0) GK[kGK * N] = 0.0;
  BwPat bp;
  if (!KDG) bp.init<WNL, WMT>(P, L, lane);
  for (int i = lane; i < N * NU; i += kWave) sm[L.U + i] = sm[L.uref + (i % NU)];
  for (int i = lane; i < N * NC; i += kWave) sl[L.LAM + i] = 0.0;
  QSYNC();
  rollout_open<WMD, false>(P, L, sm, lane);
  wrench_from_inputs<false, WNL>(P, L, LW, sm, lane);
  expansions_w<WNL, WMT>(P, L, LW, sm, lane);
  ref_cone_refresh<WD>(P, L, sm, sl, conmask, lane);
  QSYNC();
  double rho = P.penalty_initial;
  double Jplain = 0.0, viol = 0.0;
  double J = ref_merit<WMD, false>(P, L, sm, sl, rho, conmask, lane, &Jplain, &viol);
  int iter = 0;
  double last_step = 0.0;
  status = QMPC_MAX_ITER;
#ifdef QMPC_REF_PROF
  long long rp_t0 = clock64(), rp_ls = 0, rp_st = 0, rp_bw = 0, rp_tr = 0, rp_a, rp_ro = 0, rp_ma = 0, rp_b;
#define RP_BEGIN() rp_a = clock64()
#define RP_END(acc) acc += clock64() - rp_a
#else
#define RP_BEGIN() do { } while (0)
#define RP_END(acc) do { } while (0)
#endif
  for (iter = 1; iter <= P.iterations_max; ++iter) {
    RP_BEGIN();
    prepass_w<true, WNL, WMT>(P, L, sm, sl, ROT, GK, rho, lane);
    if (KDG) bp.init<WNL, WMT>(P, L, lane);
    // horizons beyond kRefineMinN: the 6 x 6 stage solves with one step of iterative refinement (qmpc_wform.h: REFINE; truncated
    // iterates keep their rounding); up to there the plain elimination already agrees with the oracle to 4e-8 N and is 10 %
    // faster (wave-uniform branch) (ConvexMpc's problem: at every horizon -- with 5 ms knots only R = 1e-6 sees the force directions)
    constexpr int kRefineMinN = 12;
    const int bp_fail = (N > kRefineMinN || WMT == WM_CONVEX)
                            ? backward_pass_w<false, true, WMT>(P, L, bp, sm, KD, GK, lane, prof, Y0)
                            : backward_pass_w<false, false, WMT>(P, L, bp, sm, KD, GK, lane, prof, Y0);
    if (bp_fail) {
      status = QMPC_NOT_PD;
      --iter;
      break;
    }
    QSYNC();
    const double dV1 = expected_decrease_w<WMT, WNL>(P, L, sm, KD, ROT, Y0, lane);
    RP_END(rp_bw);
    RP_BEGIN();
    // forward pass: backtracking line search on the AL merit
    // four trial step lengths per rollout (rollout_trials_w), tested in the order of the backtracking sequence
    double alpha = 1.0, Jn = J, Jn_plain = Jplain, vn = viol;
    bool accepted = false;
    double* ZG = sm + L.DS;        // costates of the four trials (y0 is dead after expected_decrease_w)
    int gacc = 0;
    for (int ls = 0; ls <= P.linesearch_max && !accepted; ls += 4) {
      const int grp = lane >> 4;
      const double ag = alpha * (grp == 0 ? 1.0 : (grp == 1 ? 0.5 : (grp == 2 ? 0.25 : 0.125)));
      const double Jx = rollout_trials_w<WMT, WNL>(P, L, LW, sm, KD, ZG, ag, lane);
      double Ju[4], mer[4], vi[4];
      trial_inputs_w<WMT, WNL>(P, L, sm, sl, ROT, ZG, Rl, alpha, rho, lane, Ju, mer, vi);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        if (accepted || ls + g > P.linesearch_max) continue;
        const double a_g = alpha * (g == 0 ? 1.0 : (g == 1 ? 0.5 : (g == 2 ? 0.25 : 0.125)));
        const double Jxg = read_lane(Jx, 16 * g);
        const double Jg = Jxg + wave_sum(mer[g]);
        const double expected = a_g * dV1;
        const double slack = 1e-12 * fmax(1.0, fabs(J));
        if (isfinite(Jg) && Jg - J <= 1e-4 * expected + slack) {
          accepted = true; gacc = g; Jn = Jg; Jn_plain = Jxg + wave_sum(Ju[g]); vn = wave_max(vi[g]);
        }
#ifdef QMPC_REF_PROF
        if (!accepted) ++rp_tr;
#endif
      }
      if (accepted) {
        alpha *= (gacc == 0 ? 1.0 : (gacc == 1 ? 0.5 : (gacc == 2 ? 0.25 : 0.125)));
#ifdef QMPC_REF_PROF
        rp_b = clock64();
#endif
        if (gacc != 0) {      // the accepted group's states into Xc (group 0 rolled there directly)
          const double* xs = sm + trial_states_slot(L, gacc);
          for (int i = lane; i < 13 * N; i += kWave) sm[L.Xc + 13 + i] = xs[i];
        }
        (void)recover_inputs_w<WNL, WMT>(P, L, sm, ROT, lane, alpha, ZG + 6 * N * gacc);
#ifdef QMPC_REF_PROF
        rp_ma += clock64() - rp_b;
#endif
      } else {
        alpha *= 0.0625;
      }
    }
    RP_END(rp_ls);
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
    wrench_from_inputs<false, WNL>(P, L, LW, sm, lane);
    expansions_w<WNL, WMT>(P, L, LW, sm, lane);
    ref_cone_refresh<WD>(P, L, sm, sl, conmask, lane);
    QSYNC();
    RP_BEGIN();
    const double stat = stationarity_w<WMT, WNL>(P, L, sm, sl, Y0, Rl, rho, conmask, lane);
    RP_END(rp_st);
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
      J = ref_merit<WMD, false>(P, L, sm, sl, rho, conmask, lane, &Jplain, &viol);
    }
  }
  if (iter > P.iterations_max) iter = P.iterations_max;
  if (lane < NU) forces[NU * (size_t)b + lane] = sm[L.U + lane];
  if (traj_u) for (int i = lane; i < N * NU; i += kWave) traj_u[(size_t)b * N * NU + i] = sm[L.U + i];
  if (traj_x)
    for (int i = lane; i < (N + 1) * WMD::NX; i += kWave) {
      if (WMD::NX == 13) {
        traj_x[(size_t)b * (N + 1) * WMD::NX + i] = sm[L.X + i];
      } else {      // (states are 13 doubles apart in LDS for either model)
        const int k_ = i / WMD::NX, j_ = i - WMD::NX * k_;
        traj_x[(size_t)b * (N + 1) * WMD::NX + i] = sm[L.X + 13 * k_ + j_];
      }
    }
#ifdef QMPC_REF_PROF
  Jplain = (double)(clock64() - rp_t0); viol = (double)rp_ls; last_step = (double)(QMPC_REF_PROF == 2 ? rp_ro : rp_bw); rho = (double)(QMPC_REF_PROF == 2 ? rp_ma : rp_st) + 1e-3 * (double)rp_tr;
#endif
  if (info && lane == 0) {
    qmpc_info r = {status, iter, Jplain, viol, last_step, rho};
    info[b] = r;
  }
#undef RP_BEGIN
#undef RP_END
#ifdef QMPC_WMODEL_DEFAULTED
#undef QMPC_WMODEL
#undef QMPC_WMODEL_DEFAULTED
#endif
#ifdef QMPC_WNL_DEFAULTED
#undef QMPC_WNL
#undef QMPC_WNL_DEFAULTED
#endif
