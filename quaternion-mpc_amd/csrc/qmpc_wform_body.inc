// qmpc_wform_body.inc -- the body of one solve in the wrench form (qmpc_wform.h), instance `b` of the batch, by the calling
// wave: the counterpart of qmpc_solve_body.inc (same interior-point iteration, same control flow) for QuatMpc's problem
// with four contact points and everything in LDS.  Textually included by qmpc_solve_w_kernel (qmpc_wform.hip) and, in
// qmpc_loop.hip, by the closed loop's persistent kernel and the warm-started solve (VAR == 3).  Names expected in scope:
//   PROF;  DevParams P;  const qmpc_input* in_;  double* forces;  qmpc_info* info;  double* traj_u, * traj_x;
//   WVAR (3: everything in LDS; 5: gains / per-point records / per-knot blocks in the workspace gws, one slice per
//   instance);  double* gws;  int wslot (the slice: the instance index b, or the workgroup's);  long long* prof_out;  int b, lane;  double sm[] (the dynamic LDS block, make_layout_w);
//   int warm_t (> 0: sm[L.U] holds a previous solution to start from);  const double* resume (the state record of a
//   straggler hand-off to continue from, or null)
// In a unit compiled with QMPC_WSCHED (qmpc_wform.h; qmpc_wform_sched.hip): also  WSched wsched  -- the instance's contact schedule,
// every knot's stance set non-empty.  A cold solve of QuatMpc's problem only: no warm start, no hand-off record.
// `return` leaves the including function (early exits on rejected inputs).
#ifndef QMPC_WNL
#define QMPC_WNL 4      // contact points: 4 (QuatMpc's problem on Go1) unless the including kernel says 8 (the biped of config 5)
#define QMPC_WNL_DEFAULTED 1
#endif
#ifndef QMPC_WMODEL
#define QMPC_WMODEL WM_QUAT      // WM_CONVEX: ConvexMpc's problem (four contact points; qmpc_wform.h)
#define QMPC_WMODEL_DEFAULTED 1
#endif
  constexpr int WNL = QMPC_WNL;
  constexpr int WMT = QMPC_WMODEL;
  typedef typename std::conditional<WMT == WM_CONVEX, ConvexModel, QuatModelT<WNL>>::type WMD;
  typedef Dim<WNL> WD;
  constexpr int NU = WD::NU, NC = WD::NC;
  const int N = P.N;
  constexpr bool KDG = WVAR == 5 || WVAR == 6;      // gains, per-point records and per-knot blocks in the global workspace slice
  constexpr bool SLG = WVAR == 6;                   // ... and the slack / multiplier / residual arrays (round 5: long horizons)
  constexpr bool LEAN = WNL == 8 || SLG;            // no direction arrays, weakly-active flags in a register (qmpc_wform.h)
  LayoutW LW;
#ifdef QMPC_WSCHED
  static_assert(WNL == 4 && WMT == WM_QUAT, "the contact schedule: QuatMpc's problem with four contact points");
  Layout Lsc_ = make_layout_w<WNL>(N, &LW, KDG, SLG, WMT == WM_CONVEX);
  Lsc_.sc = wsched;
  const Layout L = Lsc_;
#else
  const Layout L = make_layout_w<WNL>(N, &LW, KDG, SLG, WMT == WM_CONVEX);
#endif
  double* wsb = KDG ? gws + (size_t)wslot * wform_slice<WNL>(N, SLG) : sm;
  double* KD = wsb + L.KD;
  double* ROT = wsb + L.ROT;
  double* GK = wsb + LW.GK;
  double* sl = SLG ? wsb + LW.SLW : sm;
  const void* in = reinterpret_cast<const double*>(in_) + (size_t)b * WD::REC;
  int status = QMPC_OK;
  Prof<PROF> prof;
  prof.start();
#ifdef QMPC_WSCHED
  {
    unsigned any_ = 0;      // every leg that stands at some knot
    for (int k = 0; k < N; ++k) any_ |= L.sc.mask(k);
    setup_instance_sched<WMD>(P, L, sm, in, lane, any_, &status);
  }
#else
  setup_instance<WMD>(P, L, sm, in, lane, &status);
#endif
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
  if (lane < 10) sm[L.cst + kZeroSlotsT<WNL>() + lane] = 0.0;      // the zeros the masked operand reads of the backward pass point at
  if (lane == 0) GK[kGK * N] = 0.0;
  BwPat bp;      // lane patterns of the backward pass: once per solve where a wave owns its SIMD's registers
  if (!KDG) bp.init<WNL, WMT>(P, L, lane);
  // initial guess U = u_ref (QuatMpc.cpp:253), or the warm start of qmpc_solve_body.inc: the previous solution, still in
  // LDS, shifted by one knot (the last knot repeats); swing legs pinned to 0, a leg that has just landed starts from u_ref
  if (resume) {
    // straggler hand-off: the inputs of the lane kernel's iterate at its iteration cap (qmpc_lane.hip: call_dump)
    for (int i = lane; i < N * NU; i += kWave) sm[L.U + i] = resume[8 + i];
  } else if (warm_t > 0) {
    if (lane < NU) {
      const bool stance = (conmask >> (lane / 3)) & 1u;
      for (int k = 0; k < N; ++k) {
        const double prev = sm[L.U + ((k + 1 < N) ? k + 1 : k) * NU + lane];
        sm[L.U + k * NU + lane] = !stance ? 0.0 : (prev != 0.0 ? prev : sm[L.uref + lane]);
      }
    }
  } else {
#ifdef QMPC_WSCHED
    for (int i = lane; i < N * NU; i += kWave) sm[L.U + i] = ((i % NU) % 3 == 2) ? L.sc.uref_z(i / NU, (i % NU) / 3) : 0.0;      // u_ref of the knot
#else
    for (int i = lane; i < N * NU; i += kWave) sm[L.U + i] = sm[L.uref + (i % NU)];
#endif
  }
  QSYNC();
  rollout_open<WMD, false>(P, L, sm, lane);
  wrench_from_inputs<false, WNL, !KDG>(P, L, LW, sm, lane);
  expansions_w<WNL, WMT>(P, L, LW, sm, lane);
  double sl_part = 0.0, rc_part = 0.0;
  unsigned kapbits = 0;
  if (resume) {
    // ... and its slacks, multipliers, weakly-active flags (the sign of a stored slack) and slack residuals: the lane kernel
    // carries rc_i = rho rc0_i with rc0_i the residual at the initial guess u_ref, the same number this kernel starts from
    const double rho = resume[0];
    int j = 0;
    for (int i = lane; i < N * NC; i += kWave, ++j) {
      const int row = i % NC, l = row / 6, r = row - 6 * l;
      const double* cr = sm + L.cst + WD::C_CR + 3 * r;
      const double* ur = sm + L.uref + 3 * l;
      double c0 = cr[0] * ur[0] + cr[1] * ur[1] + cr[2] * ur[2];
      if (r == 4) c0 += -P.fz_max * sm[L.cst + WD::C_CON + l];
      const double s0 = fmax(-c0, 1.0);
      const double sraw = resume[8 + N * NU + i], lam = resume[8 + N * NU + N * NC + i];
      // (a warm-started lane launch: the row's own initial residual, from the record)
      const double sv = fabs(sraw), rc = rho * ((resume[5] != 0.0) ? resume[8 + N * NU + 2 * N * NC + i] : (c0 + s0));
      const bool flag = sraw < 0.0;
      sl[L.S + i] = sv;
      sl[L.RC + i] = rc;
      sl[L.LAM + i] = lam;
      if (!LEAN) sl[L.DS + i] = flag ? 1.0 : 0.0;
      if (conmask & (1u << l)) {
        sl_part += sv * lam;
        rc_part = fmax(rc_part, fabs(rc));
        kapbits |= flag ? (1u << j) : 0u;
      }
    }
  } else
  for (int i = lane; i < N * NC; i += kWave) {
    const double c0 = cone_value<WD>(P, L, sm, i);
    const double s0 = fmax(-c0, 1.0);
    const double lam0 = P.mu0 / s0;
    sl[L.S + i] = s0;
    sl[L.RC + i] = c0 + s0;
    sl[L.LAM + i] = lam0;
    if (!LEAN) sl[L.DS + i] = 0.0;
    if (QMPC_STANCE_AT(L, i / NC, (i % NC) / 6, conmask & (1u << ((i % NC) / 6)))) {
      sl_part += s0 * lam0;
      rc_part = fmax(rc_part, fabs(c0 + s0));
    }
  }
  QSYNC();
  prof.tick(PH_SETUP);
#ifdef QMPC_WSCHED
  int rows_ = 0;      // the cone rows that exist: six per (knot, stance leg)
  for (int k = 0; k < N; ++k) rows_ += __popc(L.sc.mask(k));
  const double inv_rows = 1.0 / (double)(6 * rows_);
#else
  const double inv_rows = 1.0 / (double)(6 * N * __popc(conmask));
#endif
  const int it_start = resume ? (int)resume[4] + 1 : 1;      // a handed-over instance continues where the lane kernel stopped
  int it = 0, iters = it_start - 1;
  double mu = 0.0, resid = 0.0, last_step = resume ? resume[3] : 1e300, last_ap = resume ? resume[1] : 0.0,
         last_ad = resume ? resume[2] : 0.0;
  status = QMPC_MAX_ITER;
  mu = wave_sum(sl_part) * inv_rows;
  resid = wave_max(rc_part);
  for (it = it_start; it <= P.iterations_max + 1; ++it) {
    if (mu <= P.mu_final && resid <= P.tol_feas && last_step <= P.tol_step) { status = QMPC_OK; break; }
    if (it > P.iterations_max) break;
    double sg = P.sigma;
    const double amin = fmin(last_ap, last_ad);
    if (it > 1 && amin >= 0.99) sg = P.sigma_fast;
    else if (it > 1 && amin < 0.2) sg = fmax(sg, 0.8);
    else if (it > 1 && amin < 0.5) sg = fmax(sg, 0.5);
    const double target = sg * mu;
    prof.tick(PH_MISC);
    prepass_w<false, WNL, WMT, LEAN>(P, L, sm, sl, ROT, GK, target, lane, kapbits);
    prof.tick(PH_PREPASS);
    if (KDG) bp.init<WNL, WMT>(P, L, lane);
    if (backward_pass_w<PROF, false, WMT>(P, L, bp, sm, KD, GK, lane, prof)) { status = QMPC_NOT_PD; break; }
    QSYNC();
    double ap, ad;
    rollout_closed_w<PROF, !KDG, WNL, WMT, !KDG, !KDG>(P, L, LW, sm, KD, ROT, lane, prof);      // trial step
    prof.tick(PH_ROLL);
    {      // input recovery + directions, one lane per (knot, contact point)
      double stp_;      // a non-finite trial step is not applied and must not become the reported step
      if (recover_directions_w<WNL, WMT, LEAN, !KDG>(P, L, sm, sl, ROT, target, lane, &ap, &ad, &stp_, kapbits)) { status = QMPC_NOT_PD; break; }
      last_step = stp_;
    }
    last_ap = ap; last_ad = ad;
    prof.tick(PH_DIRS);
    if (LEAN) apply_w<WNL, true>(P, L, sl, ap, ad, conmask, lane, kapbits, sl_part, rc_part, sm, target);   // (before dU is scaled)
    if (ap < 1.0) rollout_scaled_w<WNL, WMT, !KDG>(P, L, LW, sm, ap, lane);    // shortened primal step
    prof.tick(PH_ROLL);
    if (!LEAN) apply_w<WNL, false>(P, L, sl, ap, ad, conmask, lane, kapbits, sl_part, rc_part);
    prof.tick(PH_APPLY);
    for (int i = lane; i < N * NU; i += kWave) sm[L.U + i] += sm[L.dU + i];
    for (int i = lane; i < (N + 1) * 13; i += kWave) sm[L.X + i] = sm[L.Xc + i];
    QSYNC();
    iters = it;
    // everything the test at the head of the next pass reads is known here: a pass that ends the solve (converged, or
    // the cap reached) leaves without the wrenches and expansions at the new iterate, which nothing reads any more
    mu = wave_sum(sl_part) * inv_rows;
    resid = wave_max(rc_part);
    if ((mu <= P.mu_final && resid <= P.tol_feas && last_step <= P.tol_step) || it >= P.iterations_max) continue;
    // after a shortened step rollout_scaled_w has left the wrenches of U + dU in place: the same numbers as those of the
    // stored sum (every sum of wrench_from_inputs starts from +0.0, which absorbs a zero of either sign: the u + 0.0
    // of this form and the u + du of that one cannot give different wrenches)
    if (!(ap < 1.0)) wrench_from_inputs<false, WNL, !KDG>(P, L, LW, sm, lane);
    prof.tick(PH_MISC);
    expansions_w<WNL, WMT>(P, L, LW, sm, lane);
    prof.tick(PH_EXPAND);
  }
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
  if (info) {
#ifdef QMPC_WSCHED
    const double J = cost_sched_w<WMD>(P, L, sm, lane);
#else
    const double J = cost_plain<WMD>(P, L, sm, lane);
#endif
    double viol = 0.0;
    for (int i = lane; i < N * NC; i += kWave) {
      const int l = (i % NC) / 6;
      if (QMPC_STANCE_AT(L, i / NC, l, conmask & (1u << l))) viol = fmax(viol, fmax(cone_value<WD>(P, L, sm, i), 0.0));
    }
    viol = wave_max(viol);
    if (lane == 0) {
      qmpc_info r = {status, iters, J, viol, last_step, mu};
      info[b] = r;
    }
  }
  if (PROF && prof_out && lane == 0) {
    prof.tick(PH_MISC);
#pragma unroll
    for (int i = 0; i < PH_COUNT; ++i) prof_out[16 * (size_t)b + i] = prof.t[i];
    prof_out[16 * (size_t)b + 15] = iters;
  }
#ifdef QMPC_WMODEL_DEFAULTED
#undef QMPC_WMODEL
#undef QMPC_WMODEL_DEFAULTED
#endif
#ifdef QMPC_WNL_DEFAULTED
#undef QMPC_WNL
#undef QMPC_WNL_DEFAULTED
#endif
