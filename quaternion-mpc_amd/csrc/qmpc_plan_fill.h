// qmpc_plan_fill.h -- the selection state of a handle (qmpc_plan.h), filled from its parameters, the layouts of its horizon
// and the tuning knobs.  Included by qmpc_hip.hip (qmpc_create) and by the planner's host test (tests/native/plan_host.cpp),
// after the layout headers: make_layout (qmpc_device.h) and make_layout_w (qmpc_wform.h) must be visible.
#pragma once

#include <cstdlib>

#include "qmpc_plan.h"

namespace qmpc {

// the wrench-form kernel's layout; kd_global: 0 everything in LDS (WVAR 3), 1 gains / records / blocks in the workspace (5),
// 2 the slack arrays as well (6)
inline size_t qmpc_wform_lds_bytes(int N, int kd_global, int nl, int convex) {
  LayoutW LW;
  return (size_t)(nl == 8 ? make_layout_w<8>(N, &LW, kd_global != 0, kd_global == 2)
                          : make_layout_w<4>(N, &LW, kd_global != 0, kd_global == 2, convex != 0)).total * sizeof(double);
}
// the reference-mode body's layout (full: the direction slots exist for eight points too); kd_global: 0 / 1
inline size_t qmpc_wform_ref_lds_bytes(int N, int kd_global, int nl, int convex) {
  LayoutW LW;
  return (size_t)(nl == 8 ? make_layout_w<8>(N, &LW, kd_global != 0, false, false, true)
                          : make_layout_w<4>(N, &LW, kd_global != 0, false, convex != 0, true)).total * sizeof(double);
}

constexpr int kLaneMinLoopCold = 18432;       // ... of the cold-started closed loop (its states need fewer iterations and spread less; measured:
                                              // 16384 robots 3.95 vs 3.91 M robot-ticks/s, 20480: 4.81 vs 3.97 M; warm-started the general threshold holds)
// measured switch-over against the wave-per-instance kernels (QMPC_LANE_MIN overrides).  QuatMpc, round 4 (the wave side is the
// wrench-form kernel with its gains in the workspace): N=10 24576: lane 3.20 vs wave 3.38 M solves/s, 28672: 3.61 vs 3.44;
// N=20 16384: 1.03 vs 0.99, 24576: 1.49 vs 1.00 (long horizons run one wave per SIMD on either side).  ConvexMpc and the
// 8-point model keep the round-1 wave kernels and cross earlier (ConvexMpc N=10 / 20: equal at 16384 / 20480; 8-point
// 16384: 0.78 vs 0.82 M, 20480: 0.97 vs 0.84 M)
// End of round 5: half-filled wavefronts run as lane PAIRS (qmpc_lane.hip: the per-point blocks of the backward and the trial
// pass split across the partner lanes) and a round of the lane kernel costs 15 % less at every size below 32768 -- cold plain
// solves and cold loops cross over earlier (tools/lane_switch_scan.py): N=10 12288 instances wave 3.26 vs lane 2.66 M solves/s,
// 16384: 3.37 vs 3.50, 20480: 3.49 vs 4.32, 24576: 3.54 vs 5.16; N=16 16384: 2.15 vs 2.13, 20480: 2.22 vs 2.59; N=20 16384: 1.62
// vs 1.59, 20480: 1.66 vs 1.95; N=24 12288: 1.16 vs 0.98, 16384: 1.22 vs 1.25.  Warm-started launches have their own switch-over: kLaneMinWarm*.
// (with the warm instantiations of the split passes, warm-started loops, lane vs wave kernels: N=10 16384 robots 7.13 vs 7.70 M
// robot-ticks/s, 20480: 8.59 vs 7.84, 24576: 9.95 vs 7.98, 32768: 12.1 vs 8.2; N=20 16384: 3.68 vs 4.19, 24576: 5.19 vs 4.31)
constexpr int kLaneMinWarm = 18432, kLaneMinWarmLong = 20480, kLaneMinWarmVeryLong = 18432;
// Round 6 (apply pass split across the lane pair, stores outside the per-lane conditions: a round of the lane kernel another
// 7-10 % cheaper): N=10 13312 instances wave 4.14 vs lane 4.39 ms, 14336: 4.35 vs 4.42, 16384: 4.88 vs 4.45; N=16 14336: 6.93 vs 7.22,
// 16384: 7.80 vs 7.37; N=20 14336: 9.15 vs 9.65, 16384: 10.16 vs 9.73; N=24 14336: 11.8 vs 12.2 (tools/lane_switch_scan.py)
// ... and once more after the backward pass of the pair form was split by blocks and took its constants / the knot's state through LDS
// (profiles/r06_lane_pair_lds.txt): N=10 13824: 4.18 vs 4.22 ms, 14336: 4.36 vs 4.22; N=16 14848: 6.94 vs 6.93; N=20 14848: 9.31 vs 9.23;
// N=24 14336: 11.9 vs 11.7
constexpr int kLaneMinBatch = 14336;          // QuatMpc, horizons up to 12
// QuatMpc, longer horizons; round 5 (the wave side is the wrench-form kernel with its slack arrays in the workspace, WVAR 6):
// N=16 20480: wave 2.20 vs lane 2.15 M solves/s, 24576: 2.23 vs 2.52; N=20 20480: 1.64 vs 1.60, 24576: 1.67 vs 1.90;
// N=24 16384: 1.20 vs 1.03, 20480: 1.20 vs 1.25
constexpr int kLaneMinBatchLong = 14848;
constexpr int kLaneMinBatchVeryLong = 14848;  // horizons beyond 22
constexpr int kLaneMinBatchOther = 18432;      // ConvexMpc, short horizons (round-1 wave kernels below it)
// ConvexMpc at its own horizon (N=20; WVAR 6 below the threshold): 20480 instances wave 1.21 vs lane 1.11 M, 24576: 1.22 vs 1.29
constexpr int kLaneMinBatchConvexLong = 22528;
// 8-point model, round 5 (the wave side is the wrench-form kernel, with its slack arrays in the workspace beyond one resident
// round: two waves per SIMD at N=16): 32768 instances wave 1.95 vs lane 1.35 M solves/s, 49152: 1.99 vs 1.85 M; 65536: lane 2.3 M
constexpr int kLaneMinBatch8 = 57344;
// reference mode (AL-iLQR, <= 10 iterations; qmpc_lane_ref_kernel): measured against the wave-per-instance reference kernels
// (tools/refmode_lane_bench.py, N=10): 16384: 1.49 vs 1.74 M solves/s, 32768: 2.70 vs 1.78 M, 65536: 4.59 vs 1.83 M (N=20: 2.53 vs 0.79 M)
// iteration cap of the lane kernel in the solves of a cold-started closed loop, 11 + N/10 (in-gait states: 10.3 iterations on
// average, 17 at most, against 13.6 / 23 of the random states of the plain-solve benchmark): 32768 robots 7.47 -> 7.96 M
// robot-ticks/s, 65536: 11.98 -> 12.76 M (caps 10 .. 13 scanned, tools/loop_bench.py; QMPC_LANE_CAP_LOOP=0 switches it off)
constexpr int kLaneCapLoopBase = 11;
// ... and in its warm-started ticks (5.7 iterations on average, 13-17 at most; the records then carry the rows' initial slack
// residuals): 32768 robots 8.45 -> 9.97 M robot-ticks/s, 65536: 14.5 -> 15.9 M; N=20: 3.44 -> 4.45 M, 5.87 -> 6.86 M (caps 5 .. 10
// scanned; QMPC_LANE_CAP_WARM=0 switches it off)
constexpr int kLaneCapWarm = 8;
// (round 5, against the wrench-form reference kernels: N=10 24576 instances wave 2.98 vs lane 2.77 M solves/s, 32768: 3.04 vs 3.39 M,
// 40960: 3.07 vs 4.11 M; N=16 20480: 1.68 vs 1.52 M, 28672: 1.69 vs 1.99 M; N=20 20480: 1.28 vs 1.24 M, 24576: 1.29 vs 1.45 M)
// (end of round 5: the AL passes keep their feedback gains in double precision -- 78 instead of 42 elements per knot, every
// truncated iterate within 7e-9 N of the oracle's on 0.6 M instances where the packed form left 0.07-1 % beyond 1e-6 N and a few
// line searches per 100 000 decided the other way -- and pay for it in traffic: N=10 32768 instances wave 2.88 vs lane 2.74 M,
// 36864: 2.89 vs 3.08 M, 65536: 2.97 vs 4.61 M; N=16 24576: 1.70 vs 1.45 M, 32768: 1.71 vs 1.83 M; N=20 24576: 1.30 vs 1.21 M,
// 28672: 1.30 vs 1.36 M, 65536: 1.32 vs 2.53 M)
// Round 6: the trial sweeps and the AL backward pass run as lane PAIRS below 32769 instances (a trial of the sweep per partner lane,
// a point of the pair per lane in the per-point blocks): N=10 18432 instances wave 6.42 vs lane 6.65 ms, 20480: 7.12 vs 6.85, 32768: 11.2 vs
// 8.2 (4.0 M solves/s); N=16 14336: 8.63 vs 9.45, 18432: 10.9 vs 10.2; N=20 14336: 11.4 vs 11.8, 16384: 12.9 vs 12.0, 32768: 25.2 vs 15.1
constexpr int kLaneRefMinBatch = 19456;       // N <= 12
constexpr int kLaneRefMinBatchLong = 14848;   // horizons beyond 12 (N=20 14336: 11.4 vs 11.4 ms, 16384: 12.9 vs 11.9 after the pair forms' LDS staging)
// ConvexMpc's own mode (five iterations; tools/refmode_lane_bench.py --model convex): N=20 16384 instances wave 1.70 vs lane 1.68 M solves/s,
// 24576: 1.72 vs 2.38 M, 65536: 1.74 vs 5.61 M; N=10 16384: 3.85 vs 3.37 M, 32768: 4.00 vs 6.00 M, 65536: 4.05 vs 10.5 M
// 8-point model (N=16; tools/refmode_lane_bench.py --model biped8), against its wrench-form reference kernels (qmpc_ref8_w_kernel):
// 16384 instances wave 1.12 vs lane 0.50 M solves/s, 32768: 1.14 vs 0.85 M, 49152: 1.16 vs 1.18 M, 65536: 1.16 vs 1.45 M
// (the round-1 dense reference kernels it ran on before: 0.43 M at 8192, 0.46 M at 65536)
constexpr int kLaneRefMinBatch8 = 49152;
// (ConvexMpc with double-precision gains: N=10 20480 instances wave 4.06 vs lane 3.70 M, 24576: 4.08 vs 4.26 M, 65536: 4.18 vs
// 8.89 M; N=20 16384: 1.75 vs 1.54 M, 20480: 1.75 vs 1.81 M, 65536: 1.79 vs 4.63 M; the 8-point model's lane rate did not move)
constexpr int kLaneRefMinBatchConvex = 22528;
constexpr int kLaneRefMinBatchConvexLong = 19456;

// qmpc_solve_instances* under QMPC_INSTANCES_AUTO: the lane kernel with per-lane parameters and its hand-off (qmpc_lane_inst.hip)
// against the per-instance wave kernel (qmpc_solve_w_inst_kernel), random-variant records, batches 8192 ... 65536 in steps of
// 2048 (tools/lane_switch_scan.py --instances, profiles/r08_instance_lane_scan.txt): the smallest scanned size from which the lane
// path is faster at every larger one.  N=10 14336: wave 4.16 vs lane 4.49 ms, 16384: 4.64 vs 4.53, 18432: 5.20 vs 4.59, 65536: 17.1 vs
// 9.0; N=20 14336: 9.63 vs 10.20, 16384: 10.55 vs 10.43, 18432: 12.5 vs 10.7, 65536: 37.2 vs 19.7.  (Later than the plain solve's
// 14336 / 14848: this call also pays the expansion kernel and the per-lane rows.)
constexpr int kLaneMinInst = 16384;           // horizons up to 12
constexpr int kLaneMinInstLong = 16384;       // longer horizons
// qmpc_convex_solve_instances* under QMPC_INSTANCES_AUTO on a handle that opted in (qmpc_set_convex_lane_records): ConvexMpc's lane
// kernel with per-lane parameters (qmpc_lane_cinst.hip) against the per-instance wave kernel (qmpc_solve_cw_inst_kernel), random-variant
// records, batches 8192 ... 65536 in steps of 2048 (tools/lane_switch_scan.py --instances --model convex and --loop-instances
// --model convex, profiles/r16_convex_lane_records.txt).  One switch-over serves the solve and the loops' ticks, so it is the
// smallest scanned size from which the lane path is faster at every larger one in BOTH scans.  Solves, N=10 20480: wave 8.28 vs
// lane 9.01 ms, 22528: 9.05 vs 8.90, 24576: 9.70 vs 8.68, 65536: 24.0 vs 10.9; N=20 22528: 18.5 vs 19.4, 24576: 20.0 vs 19.4,
// 26624: 21.7 vs 19.9, 65536: 49.8 vs 28.7.  Loop ticks (20 ticks), N=10 22528: 97.0 vs 98.1 ms, 24576: 105.5 vs 101.3, 65536:
// 269.7 vs 127.1; N=20 24576: 199.3 vs 210.8, 26624: 215.5 vs 210.6, 65536: 509.4 vs 261.8.  (Later than the plain ConvexMpc
// solve's 18432 / 22528: without lane pairs a launch below 32769 instances costs what 32768 cost, and this call also pays the
// expansion kernel and the per-lane rows.)
constexpr int kLaneMinCinst = 24576;          // horizons up to 12
constexpr int kLaneMinCinstLong = 26624;      // longer horizons
// env(name): the knob's value as a string, or null (qmpc_create passes std::getenv; qmpc_plan.h lists the knobs);
// lane_slot: qmpc_create obtained a slot of the lane kernel's parameter table.  false: qmpc_create refuses the horizon (the
// round-1 workspace layout does not fit a CU).
template <class Env>
inline bool qmpc_fill_select(qmpc_select* h, const qmpc_params* params, Env env, bool lane_slot) {
  auto knob = [&](const char* name, int dflt) { const char* v = env(name); return v ? std::atoi(v) : dflt; };
  *h = qmpc_select();
  h->model = params->model;
  h->mode = params->mode;
  h->horizon = params->horizon;
  h->iterations_max = params->iterations_max;
  h->lane_slot = lane_slot;
  const int N = params->horizon;
  const int nl = model_nl(params->model), convex = params->model == QMPC_MODEL_CONVEX;
  const Layout L = make_layout(N, false, nl), Lg = make_layout(N, true, nl), Ls = make_layout(N, true, nl, true);
  for (int mode = 0; mode < 2; ++mode) {
    size_t* lds = h->lds[mode];
    lds[0] = (size_t)L.total * sizeof(double);
    lds[1] = (size_t)Lg.total * sizeof(double);
    lds[2] = (size_t)Ls.total * sizeof(double);
    lds[3] = mode ? qmpc_wform_ref_lds_bytes(N, 0, nl, convex) : qmpc_wform_lds_bytes(N, 0, nl, convex);
    lds[5] = mode ? qmpc_wform_ref_lds_bytes(N, 1, nl, convex) : qmpc_wform_lds_bytes(N, 1, nl, convex);
    lds[6] = qmpc_wform_lds_bytes(N, 2, nl, convex);
  }
  h->variant = knob("QMPC_VARIANT", 0);
  h->wform = knob("QMPC_WFORM", 1);
  const char* lm = env("QMPC_LANE_MIN");
  h->lane_min_batch = lm ? std::atoi(lm) : (params->model == QMPC_MODEL_QUAT ? (N <= 12 ? kLaneMinBatch : (N <= 22 ? kLaneMinBatchLong : kLaneMinBatchVeryLong))
                                                        : (params->model == QMPC_MODEL_QUAT8 ? kLaneMinBatch8
                                                                                             : (N > 12 ? kLaneMinBatchConvexLong : kLaneMinBatchOther)));
  // (warm-started solves share the plain solve's variants and switch-over; the cold-started loop's in-gait states switch earlier)
  h->lane_min_loop_cold = lm ? h->lane_min_batch : (kLaneMinLoopCold < h->lane_min_batch ? kLaneMinLoopCold : h->lane_min_batch);
  h->lane_min_warm = (lm || params->model != QMPC_MODEL_QUAT) ? h->lane_min_batch
                                                              : (N <= 12 ? kLaneMinWarm : (N <= 22 ? kLaneMinWarmLong : kLaneMinWarmVeryLong));
  h->lane_min_inst = knob("QMPC_LANE_INST_MIN", N <= 12 ? kLaneMinInst : kLaneMinInstLong);
  h->lane_min_cinst = knob("QMPC_LANE_CINST_MIN", N <= 12 ? kLaneMinCinst : kLaneMinCinstLong);
  // Straggler hand-off (cold plain solves of QuatMpc's problem on the lane kernel): a launch of the lane kernel lasts as
  // long as its slowest instance -- 23 interior-point iterations at N=10 (mean 13.6), 31 at N=20 (mean 14.6) -- while
  // only 8 % / 10 % of the instances are still running after 16 / 17.  The lane kernel stops there, leaves the state of
  // those instances in a record each, and the wave-per-instance kernel, whose iteration takes a tenth of the time,
  // CONTINUES them (launch_solve; qmpc_wform_body.inc `resume`).  The cap is a fixed function of the horizon, so the
  // result of an instance depends neither on timing nor on the batch it is part of.  Measured (caps 14 .. 20 scanned):
  // B=32768 N=10 4.14 -> 5.2 M solves/s, B=65536 N=10 6.8 -> 8.3 M, B=65536 N=20 3.25 -> 3.83 M, B=262144 N=10 9.1 -> 9.8 M.
  h->lane_ref_min_env = env("QMPC_LANE_REF_MIN") != nullptr;
  h->lane_ref_min = knob("QMPC_LANE_REF_MIN", params->model == QMPC_MODEL_CONVEX ? (N <= 12 ? kLaneRefMinBatchConvex : kLaneRefMinBatchConvexLong)
                                              : params->model == QMPC_MODEL_QUAT8 ? kLaneRefMinBatch8
                                                                                  : (N <= 12 ? kLaneRefMinBatch : kLaneRefMinBatchLong));
  h->lane_cap = knob("QMPC_LANE_CAP", 15 + N / 10);
  h->lane_cap_loop = knob("QMPC_LANE_CAP_LOOP", kLaneCapLoopBase + N / 10);
  h->lane_cap_warm = knob("QMPC_LANE_CAP_WARM", kLaneCapWarm);
  h->handoff_restart = knob("QMPC_HANDOFF_RESTART", 0) != 0;
  h->lane_sort = knob("QMPC_LANE_SORT", 1);
  h->lane_pair = knob("QMPC_LANE_PAIR", 1);
  h->lane_sort_idle = knob("QMPC_LANE_SORT_IDLE", 1);
  const char* lf = env("QMPC_LOOP_FUSED");
  h->loop_fused = lf ? (lf[0] == '0' ? 0 : 1) : -1;
  h->ref_wform_maxn = knob("QMPC_REF_WFORM_MAXN", QMPC_MAX_HORIZON);
  h->zero_copy = knob("QMPC_ZERO_COPY", 1);
  return h->lds[0][1] <= 160 * 1024;
}

}  // namespace qmpc
