// qmpc_plan.h -- which kernel a launch of the library takes: the handle's selection state (filled once in qmpc_create,
// qmpc_plan_fill.h), the facts of one call, and the plan of that call.  Pure host C++: no HIP call, nothing read from the
// environment, so the choice can be enumerated and checked without a device (tests/native/plan_host.cpp; the planners of the
// calls with per-instance records, which also read the handle's qmpc_opts: tests/native/records_plan_host.cpp).
//
// Every launch form of a model (plain solve, warm-started solve, per-tick and persistent closed loop) includes the same body, so
// ONE rule names the variant for all of them -- they are bit-identical only then.
#pragma once

#include <cstddef>

#include "../../include/qmpc.h"

namespace qmpc {

// What the choice of kernel depends on, fixed at qmpc_create (qmpc_set_params keeps mode and iterations_max current).
// The tuning knobs, read from the environment there and nowhere else (qmpc_plan_fill.h):
//   QMPC_VARIANT          0 auto; 1 / 2 / 3 the round-1 kernel with everything in LDS / gains / + slack arrays in the workspace
//                         (the wrench form takes the same positions), 4 the lane-per-instance kernel at every batch size
//   QMPC_WFORM            1 (default) the wrench-form kernels where they apply, 0 the round-1 family only, 3 its all-LDS form only
//   QMPC_LANE_MIN         the converged mode's switch-over to the lane kernel (plain solves, warm starts and loops alike)
//   QMPC_LANE_REF_MIN     ... the reference mode's (its closed loop included)
//   QMPC_LANE_INST_MIN    ... of qmpc_solve_instances* under QMPC_INSTANCES_AUTO (per-instance parameters on the lane kernel); the
//                         ticks of qmpc_loop_run_instances* / qmpc_loop_run_outcomes* with controller records switch over at the
//                         larger of this and the cold-started loop's own switch-over (QMPC_LANE_MIN moves that one)
//   QMPC_LANE_CINST_MIN   ... of qmpc_convex_solve_instances* under QMPC_INSTANCES_AUTO on a handle that opted in with
//                         qmpc_set_convex_lane_records (ConvexMpc's lane kernel with per-lane parameters); the ticks of its record
//                         loops with controller records switch over at the larger of this and the cold-started loop's own
//                         (warm-started, on a handle that opted in with qmpc_set_convex_warm_records: the warm-started loop's own)
//   QMPC_LANE_CAP, QMPC_LANE_CAP_LOOP, QMPC_LANE_CAP_WARM
//                         iteration cap of the lane kernel before the straggler hand-off: cold plain solves, cold-started
//                         loops, warm-started loop ticks (0: no hand-off)
//   QMPC_HANDOFF_RESTART  1: the hand-off's wave kernel ignores the state records and solves the list from scratch
//   QMPC_LANE_SORT        0: the lane kernel takes the batch in its own order (default 1: sorted by stance mask)
//   QMPC_LANE_SORT_IDLE   0: the sort of a loop tick with controller records on the lane kernel keeps robots that will not solve
//                         (rejected record, frozen, halted) among the others (diagnostic; default 1: a class of their own, last)
//   QMPC_LANE_PAIR        0: half-filled lane wavefronts run with half their lanes masked, not as lane pairs (2, 4: partial splits)
//   QMPC_LOOP_FUSED       0 / 1: the closed loop's per-tick launches / persistent kernel at every batch size
//   QMPC_REF_WFORM_MAXN   the longest horizon the reference mode takes the wrench form on (default: all)
//   QMPC_ZERO_COPY        0: host-buffer calls copy explicitly instead of solving zero-copy
struct qmpc_select {
  int model, mode, horizon, iterations_max;
  // dynamic LDS of a wave-per-instance kernel, [mode][variant]: 0 everything in LDS, 1 gains in the global workspace,
  // 2 gains and slack arrays there (the round-1 family); 3 / 5 / 6 the same three of the wrench-form kernel (qmpc_wform.hip;
  // the reference mode's body has layouts of its own, which differ for eight contact points only); [4] unused
  size_t lds[2][7];
  bool lane_slot;         // a slot of the lane kernel's parameter table was left for the handle (none: wave kernels only)
  int variant, wform;
  int lane_min_batch;     // batches from this size on take the lane-per-instance kernel
  int lane_min_loop_cold; // ... in the ticks of a cold-started closed loop
  int lane_min_warm;      // ... in warm-started solves and loop ticks (their lane passes are not pair-split)
  int lane_min_inst;      // ... in qmpc_solve_instances* under QMPC_INSTANCES_AUTO (the lane kernel with per-lane parameters)
  int lane_ref_min;       // reference-mode batches from this size on take the lane kernel
  bool lane_ref_min_env;  // ... set by QMPC_LANE_REF_MIN (then the closed loop's own switch-over does not apply)
  int lane_cap, lane_cap_loop, lane_cap_warm;
  bool handoff_restart;
  int lane_sort, lane_pair, loop_fused, ref_wform_maxn, zero_copy;
  int lane_sort_idle;     // loop ticks with controller records on the lane kernel: robots that will not solve sort last
  int lane_min_cinst;     // ... in qmpc_convex_solve_instances* under QMPC_INSTANCES_AUTO on a handle that opted in (qmpc_opts::convex_lane)
};

static inline int model_nl(int model) { return model == QMPC_MODEL_QUAT8 ? 8 : 4; }

// Reference-mode batches of Monte-Carlo scale take the AL variant of the lane passes (qmpc_lane_core.h: lane_solve_ref;
// qmpc_lane.hip: qmpc_lane_ref_kernel): QuatMpc's problem (four or eight contact points) and ConvexMpc's (its own mode: five iterations)
// In a closed loop the in-gait states need 1.8 iterations on average (plain solves of the benchmark states: 8.6) and the
// lane kernel's fixed costs weigh more: N=10 32768 robots wave kernels 12.7 vs lane 9.2 M robot-ticks/s, 65536: 13.2 vs 16.4 M
// (49152: 12.7 vs 10.1 M; ConvexMpc: 12.9 vs 8.9 M at 32768, 13.6 vs 16.6 M at 65536; N=20 65536 robots: 4.28 vs 4.99 M,
// ConvexMpc 4.73 vs 8.37 M; tools/loop_bench.py --mode 1)
constexpr int kLaneRefMinLoop = 61440;

enum qmpc_call {
  QMPC_CALL_PLAIN,            // a plain solve (qmpc_solve*, qmpc_*_device)
  QMPC_CALL_WARM,             // a warm-started solve (qmpc_solve_warm*)
  QMPC_CALL_LOOP_TICK,        // a tick of a cold-started closed loop in the per-tick form
  QMPC_CALL_WARM_LOOP_FIRST,  // the first (cold) tick of a warm-started closed loop in the per-tick form
  QMPC_CALL_WARM_LOOP_TICK,   // ... and its later ticks
  QMPC_CALL_LOOP,             // a cold-started closed loop: persistent kernel or per-tick form
  QMPC_CALL_WARM_LOOP,        // ... a warm-started one
  QMPC_CALL_PROFILE,          // qmpc_debug_profile
  QMPC_CALL_COUNT
};

struct qmpc_plan {
  int family = QMPC_KERNEL_NONE;  // QMPC_KERNEL_*; NONE: the handle refuses this kind of call
  int variant = 0;                // 0 / 1 / 2 dense (round-1) kernels, 3 / 5 / 6 wrench form, 4 lane per instance
  size_t lds = 0;                 // dynamic LDS of the wave kernel launched (lane per instance: of the hand-off's list kernel)
  bool gws = false;               // ... which is passed the gains workspace
  int handoff_variant = 0;        // hand-off: the wave kernel continuing the capped lane launch (3 / 5; 0: none)
  int iter_cap = 0;               // ... the lane kernel's iteration cap
  int handoff_grid = 0;           // ... the workgroups walking the list
  bool upload_params = false;     // lane kernel: upload the parameter block before the launch (the closed loop uploads it once)
  bool order_prev = false;        // lane kernel: order the batch by the previous records' iteration counts too (closed loop)
  bool fused = false;             // closed loop: ONE persistent launch for all ticks (variant / lds / gws are its kernel's)
};

// Straggler hand-off (qmpc_plan_fill.h): the lane kernel's iteration cap in this kind of call (0: none) and, in *wv, the wave
// kernel that CONTINUES what the capped launch leaves -- 3 (everything in LDS), 5 (gains in the workspace; up to 80 KB of LDS,
// i.e. every horizon the handle accepts: two workgroups per CU instead of four).  Only where the library chooses the lane
// kernel by itself (QMPC_VARIANT=4 forces the pure lane kernel), for QuatMpc's problem in the converged mode, and not on a
// handle whose hand-off records could not be allocated.
static inline int lane_cap(const qmpc_select& s, qmpc_call kind, bool handoff_failed, int* wv = nullptr) {
  const size_t* lds = s.lds[0];
  const int hv = (s.variant != 0 || !s.wform || s.model != QMPC_MODEL_QUAT || s.mode != QMPC_MODE_CONVERGED || handoff_failed) ? 0
                 : lds[3] <= 40 * 1024 ? 3 : (lds[5] <= 80 * 1024 ? 5 : 0);
  const int cap = kind == QMPC_CALL_PLAIN ? s.lane_cap
                  : kind == QMPC_CALL_LOOP_TICK ? s.lane_cap_loop : (kind == QMPC_CALL_WARM_LOOP_TICK ? s.lane_cap_warm : 0);
  if (wv) *wv = hv;
  return (cap > 0 && cap < s.iterations_max && hv) ? cap : 0;
}

// The plan of one call: `batch` instances, `has_info`: the call passes status records, `handoff_failed`: the handle's
// hand-off records could not be allocated.
static inline qmpc_plan plan(const qmpc_select& s, int batch, qmpc_call kind, bool has_info, bool handoff_failed) {
  qmpc_plan p;
  const bool quat = s.model == QMPC_MODEL_QUAT, convex = s.model == QMPC_MODEL_CONVEX, quat8 = s.model == QMPC_MODEL_QUAT8;
  const bool ref = s.mode == QMPC_MODE_REFERENCE;
  const bool warm = kind == QMPC_CALL_WARM || kind == QMPC_CALL_WARM_LOOP_FIRST || kind == QMPC_CALL_WARM_LOOP_TICK ||
                    kind == QMPC_CALL_WARM_LOOP;
  const bool loop = kind != QMPC_CALL_PLAIN && kind != QMPC_CALL_WARM && kind != QMPC_CALL_PROFILE;
  const bool cold_loop = kind == QMPC_CALL_LOOP_TICK || kind == QMPC_CALL_LOOP;
  // the warm start and the profile exist for QuatMpc's problem in the converged mode, the closed loop for four contact points
  if (((kind == QMPC_CALL_WARM || kind == QMPC_CALL_PROFILE) && !quat) || (warm && ref) || (kind == QMPC_CALL_PROFILE && ref) ||
      (loop && quat8))
    return p;
  const int N = s.horizon;
  const size_t* lds = s.lds[ref ? 1 : 0];
  // everything in LDS while every instance of the batch finds a CU with room (256 CUs of 160 KB)
  auto resident = [&](size_t bytes) { return bytes <= 160 * 1024 && batch <= 256 * (int)((160 * 1024) / bytes); };

  // The round-1 family (0: all LDS, 1: gains in the workspace, 2: gains and slack arrays in the workspace).
  // With everything in LDS an instance needs 39.6 KB (N=10) / 75 KB (N=20): 4 / 2 instances per CU.  Small
  // batches (<= one instance per SIMD) keep everything in LDS (lowest latency); long horizons and large batches
  // move the gains (N=10: 19 KB, two waves per SIMD) and, when that is still more than 20 KB, the slack arrays
  // (N=20: 36 KB -> 17 KB) to the workspace to raise the number of resident instances.
  auto dense = [&]() {
    // one instance per SIMD (1024 on the chip) is the break-even: beyond it a second resident wave per SIMD
    // (x1.6 throughput) beats a second round of one-wave instances (measured at B = 2048 / 4096)
    const bool big = batch > 1024;
    // QMPC_VARIANT override (experiments).  Only the instantiations that exist may be named: the 8-point model has no
    // all-LDS kernel, and an all-LDS request that does not fit the CU falls back to the workspace
    const bool no_lds_variant = quat8 || lds[0] > 160 * 1024;
    if (s.variant == 1) return no_lds_variant ? 1 : 0;
    if (s.variant == 2) return 1;
    // variant 2's set-up scratch (one record) aliases X..U..Xc: it needs (N + 1) * 13 >= the record length, or a warm start
    // loaded into U before the set-up would be overwritten
    if (s.variant == 3) return ((N + 1) * 13 >= 32 + 4 * model_nl(s.model)) ? 2 : 1;
    if (quat8) return (batch > 768 && lds[1] > 40 * 1024) ? 2 : 1;  // 3 per CU in LDS
    if (lds[0] > 40 * 1024) return (big && lds[1] > 20 * 1024) ? 2 : 1;   // < 4 instances per CU otherwise
    return big ? 1 : 0;
  };

  // The converged mode takes the wrench-form kernels (qmpc_wform.hip): with everything in LDS (3) where the round-1 family
  // would keep everything in LDS (one instance per SIMD at most) and four instances fit a CU with its layout, with the gains
  // in the workspace (5) for the mid-size batches below the lane kernel's threshold; 0: the round-1 family.
  // QMPC_WFORM=0 keeps the round-1 kernels (A/B runs); QMPC_WFORM=3 restricts QuatMpc's problem to the all-LDS form.
  auto wform = [&]() {
    if (!s.wform || ref) return 0;
    // WVAR 6 (slack arrays in the workspace too): from four knots on, where its layout leaves two waves per SIMD
    const bool w6 = N >= 4 && lds[6] <= 80 * 1024;
    if (convex) {
      if (s.variant >= 2) return 0;
      // the same rule as QuatMpc's problem at its horizon (N=20: 75 KB per instance): everything in LDS while every instance
      // finds a CU with room, the workspace form (two waves per SIMD) beyond
      if (resident(lds[3])) return 3;
      // ... as long as the batch is ONE round of resident instances (N=20: 37 KB, four per CU = 1024): beyond that the round-1
      // kernel with its slack arrays in the workspace too (17 KB: two waves per SIMD) wins -- measured at N=20, 8192 instances:
      // 0.87 M (round-1) against 0.68 M solves/s
      if (lds[5] <= 80 * 1024 && resident(lds[5])) return 5;
      return (w6 && lds[5] > 20 * 1024) ? 6 : 0;      // (short horizons: the round-1 kernel, 1.60 against 1.61 M at N=10)
    }
    if (quat8) {
      // eight contact points (round 5): 94 KB (everything in LDS) / 49 KB (workspace form) per instance at N=16, one wave per
      // SIMD either way -- everything in LDS while every instance finds a CU with room, the workspace form (three per CU) beyond
      if (s.variant >= 2 && s.variant != 3) return lds[5] <= 160 * 1024 ? 5 : 0;
      if (resident(lds[3])) return 3;
      // beyond one resident round of the workspace form: the slack arrays out as well (WVAR 6: 18 KB at N=16, two waves per SIMD)
      if (w6 && lds[5] <= 160 * 1024 && !resident(lds[5])) return 6;
      return lds[5] <= 160 * 1024 ? 5 : (lds[3] <= 160 * 1024 ? 3 : 0);
    }
    if (dense() == 0) return lds[3] <= 40 * 1024 ? 3 : 0;
    // Longer horizons (N=20, the reference's own configuration: 75 KB per instance): everything in LDS as long as every
    // instance of the batch finds a CU with room -- two per CU up to N=21 (512 instances), one per CU beyond (256) -- i.e. for
    // the single robot and small fleets; the workspace form (two waves per SIMD) from there on.  Round 5, tools/latency_b1.py.
    if (s.variant == 0 && resident(lds[3])) return 3;
    // Long horizons, mid-size batches (round 5): with 37 KB of LDS (N=20) the workspace form leaves a SIMD ONE wave, and the
    // round-1 kernel with its slack arrays in the workspace (two waves per SIMD) was faster -- N=20: 8192 instances 1.12 M against
    // 0.97 M solves/s.  WVAR 6 moves the wrench form's slack arrays out as well (18 KB); every launch form of QuatMpc's problem
    // (plain, warm-started, the closed loop's two forms) is instantiated on it, so they stay bit-identical.
    if (s.wform != 3 && w6 && lds[5] > 20 * 1024 && !resident(lds[5])) return 6;
    return (s.wform != 3 && lds[5] <= 80 * 1024) ? 5 : 0;
  };

  // The reference mode: the wrench-form kernels (3: everything in LDS, one instance per SIMD; 5: gains in the workspace),
  // with the rule of the round-1 reference kernels for which of the two; 0: keep the round-1 kernels.
  // QuatMpc's problem was first taken to horizons up to 12 only: a TRUNCATED iterate does not damp the rounding of its Newton
  // systems, and the 6 x 6 wrench-space system (condition ~1e7, growing with the horizon) is solved to ~1e-9 of the step where
  // the rotated 12 x 12 elimination keeps every direction to its own scale.  Measured against the round-1 kernels
  // (tools/refmode_bench.py): N=10 all status words and iteration counts equal, forces within 4e-8 N; with four trial step
  // lengths per rollout and the costate sweep in row-parallel form 0.91 -> 1.95 M solves/s at 1024 instances, 1.24 -> 2.9 M at
  // 8192.  N=20 (first version): status words and iteration counts equal but only 65 % of the forces within 1e-6 N (median
  // 6e-7); against the ORACLE the N=20 workload of tests/test_gpu_parity.py agrees on 354 of 512 instances (median 4.9e-7 N)
  // where the round-1 kernels agree on 499 (median 1.1e-8 N): W' = S6 (I + G S6) carries cond(S6) twice.  N=16: all within
  // 1e-6 N of the round-1 kernels (median 2.5e-8, worst 8.7e-7).  QMPC_REF_WFORM_MAXN limits the horizon (experiments).
  auto ref_wform = [&]() {
    if (!s.wform || !ref) return 0;
    if (N > s.ref_wform_maxn || N < 2) return 0;      // (one knot: the input weights would not fit behind the trial states)
    if (quat8) {      // eight points (round 5): one wave per SIMD in either form; everything in LDS while every instance finds a CU
      if (s.variant == 0 && resident(lds[3])) return 3;
      return lds[5] <= 160 * 1024 ? 5 : 0;
    }
    if (s.variant < 2) {
      if (batch <= 1024 && lds[3] <= 40 * 1024) return 3;
      // longer horizons: everything in LDS while every instance finds a CU with room (the converged mode's rule)
      if (s.variant == 0 && resident(lds[3])) return 3;
    }
    return lds[5] <= 80 * 1024 ? 5 : 0;
  };
  // the round-1 reference kernels: everything in LDS (0) or the gains in the workspace (1)
  auto ref_dense = [&]() { return (batch > 1024 || lds[0] > 40 * 1024 || s.variant >= 2 || quat8) ? 1 : 0; };
  // the variant of the bodies every launch form of the converged mode shares: the wrench form where it applies
  auto body = [&]() { const int wv = wform(); return wv ? wv : dense(); };
  auto wave = [&](int var) {
    p.family = var >= 3 ? (var >= 5 ? QMPC_KERNEL_WFORM_WS : QMPC_KERNEL_WFORM_LDS) : (var >= 1 ? QMPC_KERNEL_DENSE_WS : QMPC_KERNEL_DENSE_LDS);
    p.variant = var;
    p.lds = lds[var];
    p.gws = var == 1 || var == 2 || var == 5 || var == 6;
    return p;
  };

  if (kind == QMPC_CALL_PROFILE) {      // the profiling instantiations: the wrench form, or the round-1 kernel's 0 / 1
    const int wv = wform();
    return wave(wv ? wv : (dense() >= 1 ? 1 : 0));
  }
  if (kind == QMPC_CALL_LOOP || kind == QMPC_CALL_WARM_LOOP) {
    // At most two robots per SIMD: ONE launch, a persistent wave per robot for all ticks (qmpc_loop_fused_kernel: the per-tick
    // tails of different robots average out instead of adding up; +29 % at 1024 robots with different commands).  Larger
    // batches keep the per-tick sequence (several robots per SIMD hide the tails, and the fused kernel pays for its register
    // pressure).  QMPC_LOOP_FUSED=0 / 1 forces one or the other (experiments, tests).
    // measured, persistent vs per-tick: +25 % (256), +28 % (1024), +8 % (2048), -3 % (4096); with the warm start, whose
    // iteration counts spread more: +61 % (1024), +33 % (2048), +8 % (4096), -14 % (16384)
    // (ConvexMpc's own solver mode: the persistent kernel exists on the wrench-form reference bodies only)
    // Round 6 (profiles/r06_loop_decide.txt, profiles/HISTORY_r06.md): the workspace-form instantiations (two waves per SIMD,
    // 256 registers, 41 ... 165 spilled VGPRs outside their inner loops) were measured against the per-tick form on every
    // configuration that selects them -- persistent +8 ... +45 % everywhere except ConvexMpc's own solver mode in the workspace
    // form (N=20, 2048 robots: 0.849 vs 0.832 ms per tick), which therefore takes the per-tick form unless forced.
    const int rwv = ref_wform();
    const bool fused = (convex && ref && !rwv) ? false
                       : (s.loop_fused >= 0 ? s.loop_fused == 1 : (batch <= (warm ? 4096 : 2048) && !(convex && ref && rwv == 5)));
    // per-tick: the plan of the tick the loop repeats
    if (!fused) return plan(s, batch, warm ? QMPC_CALL_WARM_LOOP_TICK : QMPC_CALL_LOOP_TICK, true, handoff_failed);
    wave(ref ? (rwv ? rwv : ref_dense()) : body());
    p.fused = true;
    return p;
  }

  // Large batches go to the lane-per-instance kernel (qmpc_lane.hip): one lane per instance, the working set streamed through
  // a structure-of-arrays HBM workspace sized by the RESIDENT lanes (<= 1024 wavefronts).  It returns forces, info and (on
  // request) the input and state trajectories.
  bool lane = s.lane_slot && (s.variant == 4 || s.variant == 0);
  if (lane && s.variant == 0) {
    if (ref)
      lane = batch >= ((kind == QMPC_CALL_LOOP_TICK && s.lane_ref_min < kLaneRefMinLoop && !s.lane_ref_min_env) ? kLaneRefMinLoop
                                                                                                              : s.lane_ref_min);
    else
      lane = batch >= (warm ? s.lane_min_warm : (cold_loop ? s.lane_min_loop_cold : s.lane_min_batch));
  }
  if (lane) {
    int wv = 0;
    const int cap = has_info ? lane_cap(s, kind, handoff_failed, &wv) : 0;      // the hand-off selects from the status records
    if (cap) {
      wave(wv);
      p.family = QMPC_KERNEL_LANE_HANDOFF;
      p.handoff_variant = wv;
      p.iter_cap = cap;
      p.handoff_grid = lds[wv] <= 40 * 1024 ? 1024 : 512;      // one resident round
    } else {
      p.family = QMPC_KERNEL_LANE;
    }
    p.variant = 4;
    p.upload_params = !loop;
    p.order_prev = loop && !ref;      // the loop's d_info holds every robot's previous record
    return p;
  }
  if (ref) {
    const int rwv = ref_wform();
    return wave(rwv ? rwv : ref_dense());
  }
  return wave(body());
}

// A handle's run-time settings (qmpc_set_instances_policy, qmpc_set_loop_warm_records, qmpc_set_convex_records,
// qmpc_set_convex_lane_records, qmpc_set_convex_warm_records, and what became of its hand-off records): what the planners of the calls with per-instance records read besides the selection state.  The
// handle holds one and passes it whole.
struct qmpc_opts {
  int inst_policy = QMPC_INSTANCES_WAVE;      // qmpc_instances_policy of the solves and ticks with per-instance parameters
  bool handoff_failed = false;                // the hand-off records could not be allocated: the pure lane kernel
  bool loop_warm_records = false;             // the loops with controller records accept lp->warm_start (QuatMpc)
  bool convex_records = false;                // the loops with records accept a ConvexMpc handle
  bool convex_lane = false;                   // ConvexMpc's calls with per-instance records may take the lane kernel (under AUTO)
  bool convex_warm = false;                   // the loops with controller records accept lp->warm_start on a ConvexMpc handle
                                              // that opted in with convex_records (qmpc_set_convex_warm_records)
};

// The plan of qmpc_solve_instances* (per-instance parameters, qmpc_wform.hip: qmpc_solve_w_inst_kernel).  `has_info`: the call
// passes status records.
//   QMPC_INSTANCES_WAVE (the default)  the wrench-form variant (3 / 5 / 6, with its LDS and workspace) that a plain solve of
//       `batch` instances takes on the wave kernels -- also where a plain solve would go to the lane kernel.
//   QMPC_INSTANCES_AUTO  the same on a handle without a slot of the lane kernel's parameter table and below the switch-over
//       lane_min_inst; from there on the lane fields of the plain solve's plan for this batch (qmpc_lane_inst_kernel to the plain
//       solve's cap and qmpc_solve_w_list_inst_kernel on what it leaves: LANE_HANDOFF; LANE where the plain solve does not hand
//       off).  QMPC_VARIANT=4: the pure lane kernel at every batch size, as for plain solves.
// NONE under either policy: not QuatMpc's problem in the converged mode, or no wrench-form kernel for this batch under the
// handle's knobs (QMPC_WFORM=0, QMPC_WFORM=3 beyond the all-LDS sizes, ...).
static inline qmpc_plan plan_instances(const qmpc_select& s, const qmpc_opts& o, int batch, bool has_info) {
  if (s.model != QMPC_MODEL_QUAT || s.mode != QMPC_MODE_CONVERGED || !s.wform) return qmpc_plan();
  qmpc_select t = s;
  t.lane_slot = false;      // no lane kernel to go to: plan() keeps the wave kernels' own rule at every batch size
  const qmpc_plan w = plan(t, batch, QMPC_CALL_PLAIN, true, false);
  if (w.family != QMPC_KERNEL_WFORM_LDS && w.family != QMPC_KERNEL_WFORM_WS) return qmpc_plan();
  if (o.inst_policy != QMPC_INSTANCES_AUTO || !s.lane_slot) return w;
  if (s.variant != 4 && batch < s.lane_min_inst) return w;
  t = s;
  t.lane_min_batch = 0;      // the switch-over is this call's own: the plain plan only names the lane kernel's fields
  const qmpc_plan p = plan(t, batch, QMPC_CALL_PLAIN, has_info, o.handoff_failed);
  return p.variant == 4 ? p : w;
}

// The plan of qmpc_solve_schedule* (a contact schedule over the horizon; qmpc_wform_sched.hip: qmpc_solve_w_sched_kernel<3|5|6>):
// the wave wrench-form variant plan_instances picks for the size with the lane kernel off, under either policy -- the lane
// kernel has no schedule form.  The kernel adds nothing to the layout (the schedule lives in registers), so LDS and workspace
// are that plan's.  NONE where plan_instances refuses: not QuatMpc's problem with four points in the converged mode, or no
// wrench-form kernel under the handle's knobs.
static inline qmpc_plan plan_schedule(const qmpc_select& s, int batch) {
  return plan_instances(s, qmpc_opts(), batch, true);
}

// The plan of qmpc_convex_solve_instances* (ConvexMpc's problem with per-instance parameters; qmpc_wform_cinst.hip:
// qmpc_solve_cw_inst_kernel<3|5|6>).  NONE unless the handle is ConvexMpc in the converged mode with the wrench form on.
// This is the wave form: the plan of every handle that did not opt in to the lane form (the overload below).
// Where a plain solve of `batch` instances on the wave kernels (lane_slot off) takes a wrench-form variant: that variant, and the
// results are the plain solve's bit for bit.  Where it falls to the round-1 family (beyond one resident round of the workspace form, QMPC_VARIANT
// 2 / 3) there is no per-instance dense kernel, and the call keeps the wrench form: 6 (slack arrays in the workspace too: two
// waves per SIMD) under plan()'s own condition for it, else 5 while its layout leaves a CU two instances (80 KB), else 3 if an
// instance fits a CU at all; NONE otherwise.
static inline qmpc_plan plan_convex_instances(const qmpc_select& s, int batch) {
  if (s.model != QMPC_MODEL_CONVEX || s.mode != QMPC_MODE_CONVERGED || !s.wform) return qmpc_plan();
  qmpc_select w = s;
  w.lane_slot = false;
  qmpc_plan p = plan(w, batch, QMPC_CALL_PLAIN, true, false);
  if (p.family == QMPC_KERNEL_WFORM_LDS || p.family == QMPC_KERNEL_WFORM_WS) return p;
  const size_t* lds = s.lds[0];
  const bool w6 = s.horizon >= 4 && lds[6] <= 80 * 1024;      // plan(): WVAR 6 exists from four knots on, two waves per SIMD
  const int var = w6 ? 6 : lds[5] <= 80 * 1024 ? 5 : lds[3] <= 160 * 1024 ? 3 : 0;
  if (!var) return qmpc_plan();
  p = qmpc_plan();
  p.family = var == 3 ? QMPC_KERNEL_WFORM_LDS : QMPC_KERNEL_WFORM_WS;
  p.variant = var;
  p.lds = lds[var];
  p.gws = var != 3;
  return p;
}
// ... with the handle's settings.  The lane form (qmpc_lane_cinst.hip: qmpc_lane_cinst_kernel) is opt-in per handle
// (qmpc_set_convex_lane_records -> convex_lane) and taken only under QMPC_INSTANCES_AUTO, on a handle with a slot of the lane
// kernel's parameter table, where the wave plan above is not NONE: from the switch-over lane_min_cinst on (QMPC_LANE_CINST_MIN
// moves it; QMPC_VARIANT=4: at every size) the lane fields of the plain ConvexMpc solve's plan for this batch -- variant 4,
// QMPC_KERNEL_LANE (ConvexMpc's lane kernel has neither cap nor hand-off), upload_params.  Everywhere else the wave plan.
static inline qmpc_plan plan_convex_instances(const qmpc_select& s, const qmpc_opts& o, int batch, bool has_info) {
  const qmpc_plan w = plan_convex_instances(s, batch);
  if (!o.convex_lane || o.inst_policy != QMPC_INSTANCES_AUTO || !s.lane_slot || w.family == QMPC_KERNEL_NONE) return w;
  if (s.variant != 4 && batch < s.lane_min_cinst) return w;
  qmpc_select t = s;
  t.lane_min_batch = 0;      // the switch-over is this call's own: the plain plan only names the lane kernel's fields
  const qmpc_plan p = plan(t, batch, QMPC_CALL_PLAIN, has_info, o.handoff_failed);
  return p.variant == 4 ? p : w;
}

// The plan of the closed loops with per-robot controller and / or plant records (qmpc_loop_run_instances*, _outcomes*,
// _pushes*; qmpc_loop_inst.hip and its siblings, on a ConvexMpc handle qmpc_loop_crec.hip).  `has_ctrl`: controller records are
// given (their solve is a kernel with per-instance parameters), `warm`: lp->warm_start, `first`: the cold first tick of a
// warm-started call instead of the tick it repeats.
//   persistent  where the plain loop of this batch takes its persistent kernel (2048 robots, 4096 warm, or QMPC_LOOP_FUSED) on a
//               wrench-form variant: that very plan (qmpc_loop_rec_fused_kernel<3|5|6> on the model's body), fused = true --
//               the rule of a call with plant records only, whatever the policy.  Never with variant 4.
//   per tick    otherwise, fused = false.  Without controller records the plain loop's tick (lane kernel and hand-off
//               included).  With them the plan of the model's solve with per-instance parameters under the default settings
//               (plan_instances: qmpc_solve_w_inst_kernel, warm-started qmpc_solve_w_inst_warm_kernel; ConvexMpc:
//               plan_convex_instances(s, batch): the wave kernels).
//   lane form   of QuatMpc's per-tick solve with controller records, under QMPC_INSTANCES_AUTO on a handle with a slot of the
//               lane kernel's parameter table: from the LARGER of the two switch-overs the tick combines on -- that of
//               qmpc_solve_instances* (lane_min_inst; QMPC_LANE_INST_MIN moves it) and the plain loop's own (cold-started:
//               lane_min_loop_cold, warm-started: lane_min_warm; QMPC_LANE_MIN moves both) -- the lane fields of the plain loop's
//               tick for this batch: qmpc_lane_inst_kernel to lane_cap_loop (warm: qmpc_lane_inst_warm_kernel to lane_cap_warm),
//               the per-instance list kernel on what it leaves, the batch ordered by the previous records too, the parameter
//               block uploaded once per call and not inside the tick.  With the defaults the cold switch-over is 16384 robots
//               (16384 and 14336 / 14848), the warm one 18432, 20480 at N = 13 ... 22.  QMPC_VARIANT=4: the pure lane kernel
//               wherever the per-tick form runs, as for the plain loop.  `first`: the lane kernel without cap and hand-off (the
//               plain loop's QMPC_CALL_WARM_LOOP_FIRST); on the wave kernels the first tick's variant is the tick's.
//               ConvexMpc's per-tick solve with controller records takes it on a handle that opted in to BOTH convex_records and
//               convex_lane, under the same policy: from the larger of lane_min_cinst and lane_min_loop_cold the lane fields of the
//               plain cold tick (qmpc_lane_cinst_kernel: no cap, no hand-off; order_prev, no upload inside the tick).
//   ConvexMpc, warm-started with controller records: on a handle that opted in to convex_records AND convex_warm
//               (loop_warm_records has no effect on ConvexMpc).  Persistent where the plain warm-started loop is (up to 4096
//               robots; qmpc_loop_rec_fused_kernel carries the warm start); per tick otherwise: plan_convex_instances(s, batch)
//               (qmpc_solve_cw_inst_warm_kernel; `first`: the cold qmpc_solve_cw_inst_kernel on the same variant); the lane form
//               under the conditions above from the larger of lane_min_cinst and lane_min_warm, with the lane fields of the plain
//               warm ConvexMpc tick (qmpc_lane_cinst_warm_kernel; `first`: qmpc_lane_cinst_kernel) -- QMPC_KERNEL_LANE,
//               order_prev, no upload inside the tick; no cap, no hand-off, no pairs.
// NONE: the reference mode; a model other than QuatMpc and, on a handle that opted in (convex_records), ConvexMpc; controller
// records without a wrench-form kernel for the batch (QMPC_WFORM=0, ...); controller records with the warm start unless the
// handle opted in (QuatMpc: loop_warm_records; ConvexMpc: convex_warm).
static inline qmpc_plan plan_loop_instances(const qmpc_select& s, const qmpc_opts& o, int batch, bool has_ctrl, bool warm,
                                            bool first = false) {
  const bool convex = s.model == QMPC_MODEL_CONVEX && o.convex_records;
  if ((s.model != QMPC_MODEL_QUAT && !convex) || s.mode != QMPC_MODE_CONVERGED) return qmpc_plan();
  if (has_ctrl && (!s.wform || (warm && !(convex ? o.convex_warm : o.loop_warm_records)))) return qmpc_plan();
  const qmpc_plan f = plan(s, batch, warm ? QMPC_CALL_WARM_LOOP : QMPC_CALL_LOOP, true, o.handoff_failed);
  if (f.fused && (f.variant == 3 || f.variant == 5 || f.variant == 6)) return f;
  const qmpc_call tick = !warm ? QMPC_CALL_LOOP_TICK : (has_ctrl && first ? QMPC_CALL_WARM_LOOP_FIRST : QMPC_CALL_WARM_LOOP_TICK);
  qmpc_plan w = !has_ctrl ? plan(s, batch, tick, true, o.handoff_failed)
                : convex  ? plan_convex_instances(s, batch)
                          : plan_instances(s, qmpc_opts(), batch, true);
  w.fused = false;
  if (!has_ctrl || (convex && !o.convex_lane) || o.inst_policy != QMPC_INSTANCES_AUTO || w.family == QMPC_KERNEL_NONE || !s.lane_slot)
    return w;
  qmpc_select l = s;
  int& own = warm ? l.lane_min_warm : l.lane_min_loop_cold;
  const int inst_min = convex ? s.lane_min_cinst : s.lane_min_inst;
  if (s.variant != 4 && batch < (inst_min > own ? inst_min : own)) return w;
  own = 0;      // the switch-over is this call's own: the plain tick's plan only names the lane kernel's fields
  qmpc_plan p = plan(l, batch, tick, true, o.handoff_failed);
  if (p.variant != 4) return w;
  p.fused = false;
  return p;
}

}  // namespace qmpc
