// qmpc_solve_body.inc -- the body of one solve (instance `b` of the batch, by the calling wave).  Textually included by
// qmpc_solve_kernel (qmpc_kernels.hip) and, inside a lambda, by the closed loop's persistent kernel (qmpc_loop.hip), so
// that the solve kernel's code generation does not depend on the second user.  Names expected in scope:
//   template parameters MD, PROF, VAR;  DevParams P;  const qmpc_input* in_;  double* forces;  qmpc_info* info;
//   double* traj_u, * traj_x;  long long* prof_out;  double* gws;  int b, lane;  double sm[] (the dynamic LDS block);
//   int warm_t (> 0: this is a later tick of a warm-started closed loop and sm[L.U] still holds the last solution)
// `return` leaves the including function (early exits on rejected inputs).
  typedef typename MD::D D;
  constexpr int NU = D::NU, NC = D::NC;
  const int N = P.N;
  constexpr bool KDG = VAR >= 1, SLG = VAR == 2;
  constexpr bool LEAN = KDG || MD::NL != 4;     // register-lean model constants where registers bound the occupancy
  const Layout L = make_layout(N, KDG, MD::NL, SLG);
  const size_t slice = (size_t)N * (D::KD + D::ROT + (SLG ? 5 * NC : 0));
  double* KD = KDG ? gws + (size_t)b * slice : sm + L.KD;
  double* ROT = KDG ? KD + N * D::KD : sm + L.ROT;
  double* sl = SLG ? ROT + N * D::ROT : sm;      // base of the slack arrays (offsets L.S .. L.RC)
  // records are 8 * D::REC bytes apart (48 doubles; 64 for the 8-contact-point model)
  const void* in = reinterpret_cast<const double*>(in_) + (size_t)b * ((MD::NX == 13) ? D::REC : 48);
  int status = QMPC_OK;
  Prof<PROF> prof;
  prof.start();
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
  // initial guess U = u_ref (QuatMpc.cpp:253), slacks and multipliers
  if (warm_t > 0) {
    // closed loop, warm start (qmpc_loop_params.warm_start): the previous tick's solution, still in LDS, shifted by one
    // knot (the last knot repeats); swing legs are pinned to 0, a leg that has just landed starts from u_ref.
    // Lane j owns input j of every knot, so the in-place shift has no hazard.
    if (lane < NU) {
      const bool stance = (conmask >> (lane / 3)) & 1u;
      for (int k = 0; k < N; ++k) {
        const double prev = sm[L.U + ((k + 1 < N) ? k + 1 : k) * NU + lane];
        sm[L.U + k * NU + lane] = !stance ? 0.0 : (prev != 0.0 ? prev : sm[L.uref + lane]);
      }
    }
  } else {
    for (int i = lane; i < N * NU; i += kWave) sm[L.U + i] = sm[L.uref + (i % NU)];
  }
  QSYNC();
  rollout_open<MD, LEAN>(P, L, sm, lane);
  expansions<MD>(P, L, sm, lane);
  double sl_part = 0.0, rc_part = 0.0;     // per-lane shares of sum s*lambda / max |rc| over the enabled rows
  for (int i = lane; i < N * NC; i += kWave) {
    const double c0 = cone_value<D>(P, L, sm, i);
    const double s0 = fmax(-c0, 1.0);
    const double lam0 = P.mu0 / s0;
    sl[L.S + i] = s0;
    sl[L.RC + i] = c0 + s0;
    sl[L.LAM + i] = lam0;
    sl[L.DS + i] = 0.0;
    if (conmask & (1u << ((i % NC) / 6))) {
      sl_part += s0 * lam0;
      rc_part = fmax(rc_part, fabs(c0 + s0));
    }
  }
  QSYNC();
  prof.tick(PH_SETUP);
  const double inv_rows = 1.0 / (double)(6 * N * __popc(conmask));
  int it = 0, iters = 0;
  unsigned kapbits = 0;
  double mu = 0.0, resid = 0.0, last_step = 1e300, last_ap = 0.0, last_ad = 0.0;
  status = QMPC_MAX_ITER;
  for (it = 1; it <= P.iterations_max + 1; ++it) {
    // barrier parameter and slack residual over the enabled rows (shares left by the set-up / the last apply)
    mu = wave_sum(sl_part) * inv_rows;
    resid = wave_max(rc_part);
    if (mu <= P.mu_final && resid <= P.tol_feas && last_step <= P.tol_step) { status = QMPC_OK; break; }
    if (it > P.iterations_max) break;
    // centering: sigma until full steps are taken, then the fast value; short steps
    // (jamming near the boundary) call for more centering
    double sg = P.sigma;
    const double amin = fmin(last_ap, last_ad);
    if (it > 1 && amin >= 0.99) sg = P.sigma_fast;
    else if (it > 1 && amin < 0.2) sg = fmax(sg, 0.8);
    else if (it > 1 && amin < 0.5) sg = fmax(sg, 0.5);
    const double target = sg * mu;
    prof.tick(PH_MISC);
    rotation_prepass<D>(P, L, sm, sl, ROT, target, lane);
    if (KDG) __syncthreads();
    prof.tick(PH_PREPASS);
    if (backward_pass<MD, PROF, !KDG, (SLG || D::TU > 1), KDG>(P, L, sm, KD, ROT, lane, conmask, prof)) { status = QMPC_NOT_PD; break; }
    if (KDG) __syncthreads();
    double ap, ad;
    rollout_closed<MD, !KDG, LEAN, PROF>(P, L, sm, KD, ROT, 1.0, lane, prof);  // trial step
    prof.tick(PH_ROLL);
    ipm_directions<D>(P, L, sm, sl, target, lane, &ap, &ad, &last_step);
    last_ap = ap; last_ad = ad;
    prof.tick(PH_DIRS);
    if (ap < 1.0) rollout_scaled<MD, LEAN>(P, L, sm, ap, lane);    // shortened primal step
    prof.tick(PH_ROLL);
    prof.tick(PH_MISC);
    ipm_apply<D>(P, L, sl, ap, ad, conmask, lane, kapbits, sl_part, rc_part);
    if (SLG) __syncthreads();
    prof.tick(PH_APPLY);
    // accept the candidate
    for (int i = lane; i < N * NU; i += kWave) sm[L.U + i] += sm[L.dU + i];
    for (int i = lane; i < (N + 1) * 13; i += kWave) sm[L.X + i] = sm[L.Xc + i];
    QSYNC();
    prof.tick(PH_MISC);
    expansions<MD>(P, L, sm, lane);
    prof.tick(PH_EXPAND);
    iters = it;
  }
  // outputs: GetInput(u, 0) (QuatMpc.cpp:264-265)
  if (lane < NU) forces[NU * (size_t)b + lane] = sm[L.U + lane];
  if (traj_u) for (int i = lane; i < N * NU; i += kWave) traj_u[(size_t)b * N * NU + i] = sm[L.U + i];
  if (traj_x)
    for (int i = lane; i < (N + 1) * MD::NX; i += kWave) {
      const int k = i / MD::NX, j = i - MD::NX * k;
      traj_x[(size_t)b * (N + 1) * MD::NX + i] = sm[L.X + 13 * k + j];
    }
  if (info) {
    const double J = cost_plain<MD>(P, L, sm, lane);
    double viol = 0.0;
    for (int i = lane; i < N * NC; i += kWave) {
      const int l = (i % NC) / 6;
      if (conmask & (1u << l)) viol = fmax(viol, fmax(cone_value<D>(P, L, sm, i), 0.0));
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
