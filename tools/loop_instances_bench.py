#!/usr/bin/env python3
"""Robot-ticks per second of the device closed loop: the plain loop (qmpc_loop_run_device), plant records only and controller +
plant records (qmpc_loop_run_instances_device), uniform records (every robot carries the handle's values), cold start, robots
walking with different commands, device buffers, one handle per size.  The three calls alternate on the same states (copied
back before each call), each timed with device events around the call after warm-up; median of the repetitions.  The
per-robot calls include their expansion kernels.
    python tools/loop_instances_bench.py [--reps 5] [--warmup 1] [--ticks 50] [--sizes 10:1024,10:4096,10:65536] [--json FILE]
--outcomes: the same two per-robot calls through qmpc_loop_run_outcomes_device as well (empty records before every call), each
    next to its qmpc_loop_run_instances_device twin: what accumulating the outcome records costs, as same-job pairs.
--outcomes --stop: instead, a population of which half certainly falls (robots standing at 0.3 m, every second one pressed down
    with 1000 N) through the outcome call with stop_when_down = 0 and = 1: time of each, and the solves that ran to the
    iteration cap (from the records; for the run that does not stop, from a run whose thresholds never freeze a record).
--policy wave|auto|both: the handle's qmpc_instances_policy for the calls with controller records (default wave).  both: every
    such call twice in the same job on the same records, under WAVE (the per-instance wave kernel in every tick) and under AUTO
    (the lane kernel with per-lane parameters and its hand-off from the switch-over on), next to the plain loop's figure.  With
    --outcomes --stop the falling population runs with uniform controller records under each policy asked for (auto: e.g. with
    and without QMPC_LANE_SORT_IDLE=0 in the environment, the sort's class for robots that will not solve).
--pushes [--per-robot K]: instead, same-job pairs of qmpc_loop_run_outcomes_device against qmpc_loop_run_pushes_device whose K
    windows per robot never act (they lie beyond the run, with a wrench that is not zero): what reading the windows in every tick
    costs, with plant records and with controller + plant records, on the walking fleet.  The two calls compute the same bytes.
--ground: instead, same-job pairs of qmpc_loop_run_pushes_device (one idle window per robot) against qmpc_loop_run_ground_device on the
    same windows, first with ground records that never bind (mu = 10, fz_max = 1e4: what reading the record and clamping in
    every tick costs; the same bytes up to the robots a zero-force leg binds on, counted in the row) and then with
    mu_true = 0.5 mu_ctrl on every robot (the clamp binds: the robots compute something else), with plant records and with
    controller + plant records, on the walking fleet.  Median, minimum and maximum of the repetitions beside each ratio.
--actuation: instead, same-job pairs of qmpc_loop_run_ground_device (one idle window per robot, ground records that never bind:
    mu = 10, fz_max = 1e4) against qmpc_loop_run_actuation_device on the same windows and ground records, first with identity
    records (what reaching the record and keeping the delay line current in every tick costs; the ground call's bytes, stated
    in the row) and then with delay 2, alpha = 0.5 on every robot (the robots compute something else), with plant records and
    with controller + plant records, on the walking fleet.  Median, minimum and maximum of the repetitions beside each ratio.
    --policy auto puts the calls with controller records on the lane tick from its switch-over on.
--sensing: instead, same-job pairs of qmpc_loop_run_actuation_device (one idle window per robot, ground records that never bind,
    identity actuation records) against qmpc_loop_run_sensing_device on the same records, first with identity sensing records
    (what reaching the record in every tick's front end costs; the actuation call's bytes, stated in the row) and then with
    fully noisy records (random_go1_senses with a bias added on every channel: 12 active channels, seen given: twelve hashes,
    the substitution and the restore per tick; the robots compute something else), with plant records and with controller +
    plant records, on the walking fleet.  Median, minimum and maximum of the repetitions beside each ratio.
--gaits: instead, same-job pairs of qmpc_loop_run_sensing_device (--sensing's identity case: the same fleet and records) against
    qmpc_loop_run_gaits_device on the same records, first with identity gait records (what reaching the record in every tick's
    front end costs; the sensing call's bytes, stated in the row) and then with a mixed-gait fleet (random_go1_gaits: six gaits at
    1.5 - 3 Hz, started from qmpc_loop_state_set_gait; the robots solve other problems and, on the lane tick, fill more classes of
    the stance sort -- a description of that fleet, not an overhead), with plant records and with controller + plant records.
--motors [--tau-scale-lo 0.15 --tau-scale-hi 0.6]: instead, same-job pairs of qmpc_loop_run_gaits_device (--gaits' identity case: the
    same fleet and records) against qmpc_loop_run_motors_device on the same records, first with +inf limits (what a tick's inverse
    kinematics, Jacobians and tally cost; the gaits call's bytes, stated in the row) and then with the Go1's limits times
    U(lo, hi) per joint type (random_go1_motors: limits that bind, the robots compute something else), with plant records and
    with controller + plant records.  Beside each row the fleet's peak torque per joint type and the robots clipped.
--records uniform|random: every robot carries the handle's values (default), or random_go1_variants / random_go1_plants.
--warm-records [--mu0 1e-6]: instead, the warm-started loop with controller + plant records (qmpc_set_loop_warm_records) as same-job
    pairs: the plain loop and the call with records, each cold-started (a handle on the default barrier parameter) and
    warm-started (lp.warm_start = 1 on a handle with ipm_mu0 = --mu0, the setting the plain warm loop's figures were taken
    with), alternating on the same states.  Per size: robot-ticks/s of the four calls, warm / cold of the call with records, and
    that ratio against the plain loop's own warm / cold -- with uniform records the plain warm loop is the ceiling.  --policy
    both adds the calls with records under AUTO (the lane form from its switch-over on).
--model convex: the default comparison (plain / plant records / controller + plant records) on a ConvexMpc handle that opted in
    with qmpc_set_convex_records, with the commands of the ConvexMpc loop tests and records around default_convex_params
    (random_go1_convex_variants).  The handle also opts in to the lane form (qmpc_set_convex_lane_records): with ctrl the ticks
    take qmpc_lane_cinst_kernel from the switch-over on under AUTO and stay on the wave kernels under WAVE.  With --warm-records:
    the cold / warm pairs above on ConvexMpc handles, the warm one opted in with qmpc_set_convex_warm_records (under AUTO its warm
    ticks take qmpc_lane_cinst_warm_kernel from the warm switch-over on)."""
import argparse
import importlib.util
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
DEFAULT_SIZES = "10:1024,10:4096,10:65536"


def load_pkg():
    spec = importlib.util.spec_from_file_location("quaternion_mpc_amd", REPO / "quaternion-mpc_amd" / "__init__.py",
                                                  submodule_search_locations=[str(REPO / "quaternion-mpc_amd")])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["quaternion_mpc_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def falling(pkg, lib, torch, N, B, a, policy=None):
    """the population of which half certainly falls, with and without stop_when_down (see the module docstring); policy: None,
    or the policy under which the call runs with uniform controller records"""
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    lp = pkg.default_loop_params(lib)
    T = a.ticks
    st = pkg.loop_states([[0.0, 0.0, 0.30, 0.0, 0.0, 0.0, 0.0]] * B, lp, height=0.3, yaw=np.linspace(-3, 3, B), lib=lib)
    plant = pkg.plant_params(p, B)
    plant["ext_force_world"][1::2, 2] = -1000.0
    s = pkg.Solver(p, B, device=0, lib=lib)
    if policy:
        s.set_instances_policy(policy)
    s.prepare(B)
    s.prepare_instances()
    dev = lambda x: torch.from_numpy(x.view(np.uint8).copy()).cuda()      # noqa: E731
    d_st0, d_oc0, d_plant = dev(st), dev(pkg.loop_outcomes(B, lib)), dev(plant)
    d_ctrl = dev(pkg.instance_params(p, B)) if policy else None
    d_st, d_oc = d_st0.clone(), d_oc0.clone()
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    torch.cuda.synchronize()
    never = pkg.default_outcome_params(lib)
    never.down_height = never.down_upright = -1e300      # only a non-finite state freezes a record: every solve is counted
    ops = {"go": pkg.default_outcome_params(lib), "stop": pkg.default_outcome_params(lib, stop_when_down=True), "count": never}
    times, recs = {k: [] for k in ops}, {}
    for r in range(a.warmup + a.reps):
        for k, op in ops.items():
            with torch.cuda.stream(stream):
                d_st.copy_(d_st0)
                d_oc.copy_(d_oc0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            s.loop_run_outcomes_device(B, d_st.data_ptr(), T, d_oc.data_ptr(), lp, op, d_ctrl=d_ctrl.data_ptr() if policy else 0,
                                       d_plant=d_plant.data_ptr(), stream=sp)
            e1.record(stream)
            e1.synchronize()
            if r >= a.warmup:
                times[k].append(e0.elapsed_time(e1))
            recs[k] = d_oc.cpu().numpy().view(pkg.LOOP_OUTCOME_DTYPE).reshape(B)
    form = s.loop_instances_plan(B, policy is not None, False)
    s.close()
    capped = lambda o: int((o["not_ok_ticks"] - o["rejected_ticks"]).sum())      # noqa: E731  (status QMPC_MAX_ITER)
    ms = {k: float(np.median(v)) for k, v in times.items()}
    row = {"N": N, "B": B, "ticks": T, "policy": policy, "form": form, "down": int((recs["go"]["down_tick"] >= 0).sum()),
           "go_ms": ms["go"], "stop_ms": ms["stop"], "stop_over_go": ms["stop"] / ms["go"],
           "go_solves": int(recs["count"]["ticks"].sum()), "stop_solves": int(recs["stop"]["ticks"].sum()),
           "go_capped_solves": capped(recs["count"]), "stop_capped_solves": capped(recs["stop"]),
           "go_rejected_solves": int(recs["count"]["rejected_ticks"].sum()), "stop_rejected_solves": int(recs["stop"]["rejected_ticks"].sum())}
    print(f"N={N:2d} B={B:6d} {'policy ' + policy + ' ' if policy else ''}{form}: {row['down']} of {B} robots down within {T} ticks   simulated on {ms['go']:9.3f} ms "
          f"(min {min(times['go']):.3f}, max {max(times['go']):.3f}; {row['go_solves']} solves, {row['go_capped_solves']} at the iteration cap, "
          f"{row['go_rejected_solves']} rejected)   stop_when_down {ms['stop']:9.3f} ms (min {min(times['stop']):.3f}, max {max(times['stop']):.3f}; "
          f"{row['stop_solves']} solves, {row['stop_capped_solves']} at the cap, {row['stop_rejected_solves']} rejected)   "
          f"stop / go {row['stop_over_go']:.3f}", flush=True)
    return row


def pushes(pkg, lib, torch, N, B, a):
    """the outcome call against the push call whose windows never act (see the module docstring)"""
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    lp = pkg.default_loop_params(lib)
    T, K = a.ticks, a.per_robot
    rng = np.random.default_rng(5)
    cmds = np.zeros((B, 7))
    cmds[:, 0] = rng.uniform(-0.4, 0.4, B); cmds[:, 1] = rng.uniform(-0.15, 0.15, B)
    cmds[:, 2] = rng.uniform(0.26, 0.32, B); cmds[:, 5] = rng.uniform(-0.4, 0.4, B)
    cmds[:, 6] = (rng.random(B) < 0.85).astype(float)
    stand = cmds.copy(); stand[:, 6] = 0.0
    st = pkg.loop_states(stand, lp, height=0.3, yaw=rng.uniform(-3, 3, B), lib=lib)
    s = pkg.Solver(p, B, device=0, lib=lib)
    s.set_instances_policy(a.policy if a.policy != "both" else "wave")
    s.prepare(B)
    s.prepare_instances()
    st = s.loop_run(st, 6, lp)
    st["movement_mode"] = cmds[:, 6]
    if a.records == "random":
        ctrl = pkg.random_go1_variants(B, seed=12, base=p)
        ctrl["mu"] = np.maximum(ctrl["mu"], 0.5)
        plant = pkg.random_go1_plants(B, seed=11, base=p, payload=(-1.0, 3.0), force=(0.0, 10.0))
    else:
        ctrl, plant = pkg.instance_params(p, B), pkg.plant_params(p, B)
    push = pkg.random_go1_pushes(B, seed=13, per_robot=K, impulse=(1.0, 5.0), dt=lp.dt)
    push["start_tick"] += 1e9      # beyond any run
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).cuda()      # noqa: E731
    d_st0, d_oc0, d_ctrl, d_plant, d_push = dev(st), dev(pkg.loop_outcomes(B, lib)), dev(ctrl), dev(plant), dev(push)
    d_st, d_oc = d_st0.clone(), d_oc0.clone()
    op = pkg.default_outcome_params(lib)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    torch.cuda.synchronize()
    calls = {}
    for name, c in (("plant", 0), ("ctrl_plant", d_ctrl.data_ptr())):
        calls[name + "_outcomes"] = lambda c=c: s.loop_run_outcomes_device(B, d_st.data_ptr(), T, d_oc.data_ptr(), lp, op, d_ctrl=c,
                                                                          d_plant=d_plant.data_ptr(), stream=sp)
        calls[name + "_pushes"] = lambda c=c: s.loop_run_pushes_device(B, d_st.data_ptr(), T, d_oc.data_ptr(), d_push.data_ptr(), K, lp, op,
                                                                      d_ctrl=c, d_plant=d_plant.data_ptr(), stream=sp)
    times, bits = {k: [] for k in calls}, {}
    for r in range(a.warmup + a.reps):
        for k, fn in calls.items():
            with torch.cuda.stream(stream):
                d_st.copy_(d_st0)
                d_oc.copy_(d_oc0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if r >= a.warmup:
                times[k].append(e0.elapsed_time(e1))
            bits[k] = (d_st.cpu().numpy().tobytes(), d_oc.cpu().numpy().tobytes())
    forms = {"plant": s.loop_instances_plan(B, False, False), "ctrl_plant": s.loop_instances_plan(B, True, False)}
    s.close()
    ms = {k: float(np.median(v)) for k, v in times.items()}
    row = {"N": N, "B": B, "ticks": T, "records": a.records, "pushes_per_robot": K}
    for k in ("plant", "ctrl_plant"):
        o, q = k + "_outcomes", k + "_pushes"
        row.update({o + "_ms": ms[o], q + "_ms": ms[q], k + "_form": forms[k], k + "_pushes_ratio": ms[q] / ms[o],
                    k + "_outcomes_spread": (max(times[o]) - min(times[o])) / ms[o], k + "_pushes_spread": (max(times[q]) - min(times[q])) / ms[q],
                    k + "_same_bytes": bits[o] == bits[q]})
        print(f"N={N:2d} B={B:6d} {k:10s} {forms[k]}: outcome call {ms[o]:9.3f} ms (min {min(times[o]):.3f}, max {max(times[o]):.3f})   push call, "
              f"{K} idle window(s) per robot {ms[q]:9.3f} ms (min {min(times[q]):.3f}, max {max(times[q]):.3f})   push / outcome "
              f"{row[k + '_pushes_ratio']:.4f}   same bytes: {row[k + '_same_bytes']}", flush=True)
    return row


def ground(pkg, lib, torch, N, B, a):
    """the push call against the ground call, with records that never bind and with binding ones (see the module docstring)"""
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    lp = pkg.default_loop_params(lib)
    T = a.ticks
    rng = np.random.default_rng(5)
    cmds = np.zeros((B, 7))
    cmds[:, 0] = rng.uniform(-0.4, 0.4, B); cmds[:, 1] = rng.uniform(-0.15, 0.15, B)
    cmds[:, 2] = rng.uniform(0.26, 0.32, B); cmds[:, 5] = rng.uniform(-0.4, 0.4, B)
    cmds[:, 6] = (rng.random(B) < 0.85).astype(float)
    stand = cmds.copy(); stand[:, 6] = 0.0
    st = pkg.loop_states(stand, lp, height=0.3, yaw=rng.uniform(-3, 3, B), lib=lib)
    s = pkg.Solver(p, B, device=0, lib=lib)
    s.set_instances_policy(a.policy if a.policy != "both" else "wave")
    s.prepare(B)
    s.prepare_instances()
    st = s.loop_run(st, 6, lp)
    st["movement_mode"] = cmds[:, 6]
    if a.records == "random":
        ctrl = pkg.random_go1_variants(B, seed=12, base=p)
        ctrl["mu"] = np.maximum(ctrl["mu"], 0.5)
        plant = pkg.random_go1_plants(B, seed=11, base=p, payload=(-1.0, 3.0), force=(0.0, 10.0))
    else:
        ctrl, plant = pkg.instance_params(p, B), pkg.plant_params(p, B)
    push = pkg.random_go1_pushes(B, seed=13, per_robot=1, impulse=(1.0, 5.0), dt=lp.dt)
    push["start_tick"] += 1e9      # beyond any run
    loose, tight = pkg.ground_params(B), pkg.ground_params(B)
    loose["mu"], loose["fz_max"] = 10.0, 1e4
    tight["mu"] = 0.5 * ctrl["mu"][:, None]
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).cuda()      # noqa: E731
    d_st0, d_oc0, d_ta0, d_ctrl, d_plant, d_push = dev(st), dev(pkg.loop_outcomes(B, lib)), dev(pkg.ground_tallies(B)), dev(ctrl), dev(plant), dev(push)
    d_loose, d_tight = dev(loose), dev(tight)
    d_st, d_oc, d_ta = d_st0.clone(), d_oc0.clone(), d_ta0.clone()
    op = pkg.default_outcome_params(lib)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    torch.cuda.synchronize()
    calls = {}
    for name, c in (("plant", 0), ("ctrl_plant", d_ctrl.data_ptr())):
        calls[name + "_pushes"] = lambda c=c: s.loop_run_pushes_device(B, d_st.data_ptr(), T, d_oc.data_ptr(), d_push.data_ptr(), 1, lp, op,
                                                                      d_ctrl=c, d_plant=d_plant.data_ptr(), stream=sp)
        for kind, d_g in (("loose", d_loose), ("tight", d_tight)):
            calls[name + "_" + kind] = lambda c=c, d_g=d_g: s.loop_run_ground_device(B, d_st.data_ptr(), T, d_oc.data_ptr(), d_g.data_ptr(), d_ta.data_ptr(),
                                                                                     d_push.data_ptr(), 1, lp, op, d_ctrl=c, d_plant=d_plant.data_ptr(),
                                                                                     stream=sp)
    times, bits, tallies = {k: [] for k in calls}, {}, {}
    for r in range(a.warmup + a.reps):
        for k, fn in calls.items():
            with torch.cuda.stream(stream):
                d_st.copy_(d_st0)
                d_oc.copy_(d_oc0)
                d_ta.copy_(d_ta0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if r >= a.warmup:
                times[k].append(e0.elapsed_time(e1))
            bits[k] = (d_st.cpu().numpy().view(pkg.LOOP_STATE_DTYPE), d_oc.cpu().numpy().view(pkg.LOOP_OUTCOME_DTYPE))
            tallies[k] = d_ta.cpu().numpy().view(pkg.GROUND_TALLY_DTYPE).reshape(B)
    forms = {"plant": s.loop_instances_plan(B, False, False), "ctrl_plant": s.loop_instances_plan(B, True, False)}
    s.close()
    ms = {k: float(np.median(v)) for k, v in times.items()}
    row = {"N": N, "B": B, "ticks": T, "records": a.records}
    for k in ("plant", "ctrl_plant"):
        q = k + "_pushes"
        row.update({q + "_ms": ms[q], k + "_form": forms[k], q + "_spread": (max(times[q]) - min(times[q])) / ms[q]})
        print(f"N={N:2d} B={B:6d} {k:10s} {forms[k]}: push call {ms[q]:9.3f} ms (min {min(times[q]):.3f}, max {max(times[q]):.3f})", flush=True)
        for kind, what in (("loose", "mu = 10, fz_max = 1e4"), ("tight", "mu_true = 0.5 mu_ctrl")):
            g = k + "_" + kind
            ta = tallies[g]
            quiet = ta["clipped_ticks"] == 0
            same = all(x.reshape(B)[quiet].tobytes() == y.reshape(B)[quiet].tobytes() for x, y in zip(bits[g], bits[q]))
            row.update({g + "_ms": ms[g], g + "_ratio": ms[g] / ms[q], g + "_spread": (max(times[g]) - min(times[g])) / ms[g],
                        g + "_robots_clipped": int((~quiet).sum()), g + "_unclipped_same_bytes": same})
            print(f"    ground call, {what:22s} {ms[g]:9.3f} ms (min {min(times[g]):.3f}, max {max(times[g]):.3f})   ground / push {row[g + '_ratio']:.4f}   "
                  f"robots clipped {int((~quiet).sum())} (clipped ticks {int(ta['clipped_ticks'].sum())}, friction leg-ticks {int(ta['friction_leg_ticks'].sum())}, "
                  f"normal {int(ta['normal_leg_ticks'].sum())}); robots never clipped have the push call's bytes: {same}", flush=True)
    return row


def actuation(pkg, lib, torch, N, B, a):
    """the ground call against the actuation call, with identity records and with delay 2, alpha 0.5 (see the module docstring)"""
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    lp = pkg.default_loop_params(lib)
    T = a.ticks
    rng = np.random.default_rng(5)
    cmds = np.zeros((B, 7))
    cmds[:, 0] = rng.uniform(-0.4, 0.4, B); cmds[:, 1] = rng.uniform(-0.15, 0.15, B)
    cmds[:, 2] = rng.uniform(0.26, 0.32, B); cmds[:, 5] = rng.uniform(-0.4, 0.4, B)
    cmds[:, 6] = (rng.random(B) < 0.85).astype(float)
    stand = cmds.copy(); stand[:, 6] = 0.0
    st = pkg.loop_states(stand, lp, height=0.3, yaw=rng.uniform(-3, 3, B), lib=lib)
    s = pkg.Solver(p, B, device=0, lib=lib)
    s.set_instances_policy(a.policy if a.policy != "both" else "wave")
    s.prepare(B)
    s.prepare_instances()
    st = s.loop_run(st, 6, lp)
    st["movement_mode"] = cmds[:, 6]
    if a.records == "random":
        ctrl = pkg.random_go1_variants(B, seed=12, base=p)
        ctrl["mu"] = np.maximum(ctrl["mu"], 0.5)
        plant = pkg.random_go1_plants(B, seed=11, base=p, payload=(-1.0, 3.0), force=(0.0, 10.0))
    else:
        ctrl, plant = pkg.instance_params(p, B), pkg.plant_params(p, B)
    push = pkg.random_go1_pushes(B, seed=13, per_robot=1, impulse=(1.0, 5.0), dt=lp.dt)
    push["start_tick"] += 1e9      # beyond any run
    loose = pkg.ground_params(B)
    loose["mu"], loose["fz_max"] = 10.0, 1e4
    ident, slow = pkg.actuation_params(B), pkg.actuation_params(B, delay_ticks=2)
    slow["alpha"] = 0.5
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).cuda()      # noqa: E731
    d_st0, d_oc0, d_ta0, d_ctrl, d_plant, d_push = dev(st), dev(pkg.loop_outcomes(B, lib)), dev(pkg.ground_tallies(B)), dev(ctrl), dev(plant), dev(push)
    d_li0 = dev(pkg.actuation_lines(B, pkg.stand_forces_body(p.mass)))
    d_loose, d_ident, d_slow = dev(loose), dev(ident), dev(slow)
    d_st, d_oc, d_ta, d_li = d_st0.clone(), d_oc0.clone(), d_ta0.clone(), d_li0.clone()
    op = pkg.default_outcome_params(lib)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    torch.cuda.synchronize()
    calls = {}
    for name, c in (("plant", 0), ("ctrl_plant", d_ctrl.data_ptr())):
        calls[name + "_ground"] = lambda c=c: s.loop_run_ground_device(B, d_st.data_ptr(), T, d_oc.data_ptr(), d_loose.data_ptr(), d_ta.data_ptr(),
                                                                      d_push.data_ptr(), 1, lp, op, d_ctrl=c, d_plant=d_plant.data_ptr(), stream=sp)
        for kind, d_a in (("identity", d_ident), ("slow", d_slow)):
            calls[name + "_" + kind] = lambda c=c, d_a=d_a: s.loop_run_actuation_device(B, d_st.data_ptr(), T, d_oc.data_ptr(), d_a.data_ptr(), d_li.data_ptr(),
                                                                                        d_loose.data_ptr(), d_ta.data_ptr(), d_push.data_ptr(), 1, lp, op,
                                                                                        d_ctrl=c, d_plant=d_plant.data_ptr(), stream=sp)
    times, bits = {k: [] for k in calls}, {}
    for r in range(a.warmup + a.reps):
        for k, fn in calls.items():
            with torch.cuda.stream(stream):
                d_st.copy_(d_st0)
                d_oc.copy_(d_oc0)
                d_ta.copy_(d_ta0)
                d_li.copy_(d_li0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if r >= a.warmup:
                times[k].append(e0.elapsed_time(e1))
            bits[k] = (d_st.cpu().numpy().tobytes(), d_oc.cpu().numpy().tobytes(), d_ta.cpu().numpy().tobytes())
    forms = {"plant": s.loop_instances_plan(B, False, False), "ctrl_plant": s.loop_instances_plan(B, True, False)}
    s.close()
    ms = {k: float(np.median(v)) for k, v in times.items()}
    row = {"N": N, "B": B, "ticks": T, "records": a.records, "policy": a.policy}
    for k in ("plant", "ctrl_plant"):
        q = k + "_ground"
        row.update({q + "_ms": ms[q], k + "_form": forms[k], q + "_spread": (max(times[q]) - min(times[q])) / ms[q]})
        print(f"N={N:2d} B={B:6d} {k:10s} {forms[k]}: ground call {ms[q]:9.3f} ms (min {min(times[q]):.3f}, max {max(times[q]):.3f}, spread "
              f"{100 * row[q + '_spread']:.1f} %)", flush=True)
        for kind, what in (("identity", "identity records"), ("slow", "delay 2, alpha 0.5")):
            g = k + "_" + kind
            same = bits[g] == bits[q]
            row.update({g + "_ms": ms[g], g + "_ratio": ms[g] / ms[q], g + "_spread": (max(times[g]) - min(times[g])) / ms[g],
                        g + "_same_bytes_as_ground": same})
            print(f"    actuation call, {what:18s} {ms[g]:9.3f} ms (min {min(times[g]):.3f}, max {max(times[g]):.3f}, spread "
                  f"{100 * row[g + '_spread']:.1f} %)   actuation / ground {row[g + '_ratio']:.4f}   the ground call's bytes: {same}", flush=True)
    return row


def sensing(pkg, lib, torch, N, B, a):
    """the actuation call against the sensing call, with identity records and with fully noisy ones (see the module docstring)"""
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    lp = pkg.default_loop_params(lib)
    T = a.ticks
    rng = np.random.default_rng(5)
    cmds = np.zeros((B, 7))
    cmds[:, 0] = rng.uniform(-0.4, 0.4, B); cmds[:, 1] = rng.uniform(-0.15, 0.15, B)
    cmds[:, 2] = rng.uniform(0.26, 0.32, B); cmds[:, 5] = rng.uniform(-0.4, 0.4, B)
    cmds[:, 6] = (rng.random(B) < 0.85).astype(float)
    stand = cmds.copy(); stand[:, 6] = 0.0
    st = pkg.loop_states(stand, lp, height=0.3, yaw=rng.uniform(-3, 3, B), lib=lib)
    s = pkg.Solver(p, B, device=0, lib=lib)
    s.set_instances_policy(a.policy if a.policy != "both" else "wave")
    s.prepare(B)
    s.prepare_instances()
    st = s.loop_run(st, 6, lp)
    st["movement_mode"] = cmds[:, 6]
    if a.records == "random":
        ctrl = pkg.random_go1_variants(B, seed=12, base=p)
        ctrl["mu"] = np.maximum(ctrl["mu"], 0.5)
        plant = pkg.random_go1_plants(B, seed=11, base=p, payload=(-1.0, 3.0), force=(0.0, 10.0))
    else:
        ctrl, plant = pkg.instance_params(p, B), pkg.plant_params(p, B)
    push = pkg.random_go1_pushes(B, seed=13, per_robot=1, impulse=(1.0, 5.0), dt=lp.dt)
    push["start_tick"] += 1e9      # beyond any run
    loose = pkg.ground_params(B)
    loose["mu"], loose["fz_max"] = 10.0, 1e4
    noisy = pkg.random_go1_senses(B, seed=14)
    noisy["bias"] += 1e-3      # every channel active: a bias and a noise level on all twelve
    noisy["sigma"] += 1e-4
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).cuda()      # noqa: E731
    d_st0, d_oc0, d_ta0, d_ctrl, d_plant, d_push = dev(st), dev(pkg.loop_outcomes(B, lib)), dev(pkg.ground_tallies(B)), dev(ctrl), dev(plant), dev(push)
    d_li0, d_sn0 = dev(pkg.actuation_lines(B, pkg.stand_forces_body(p.mass))), dev(pkg.sense_seen(B))
    d_loose, d_act, d_ident, d_noisy = dev(loose), dev(pkg.actuation_params(B)), dev(pkg.sense_params(B)), dev(noisy)
    d_st, d_oc, d_ta, d_li, d_sn = d_st0.clone(), d_oc0.clone(), d_ta0.clone(), d_li0.clone(), d_sn0.clone()
    op = pkg.default_outcome_params(lib)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    torch.cuda.synchronize()
    calls = {}
    for name, c in (("plant", 0), ("ctrl_plant", d_ctrl.data_ptr())):
        calls[name + "_actuation"] = lambda c=c: s.loop_run_actuation_device(B, d_st.data_ptr(), T, d_oc.data_ptr(), d_act.data_ptr(), d_li.data_ptr(),
                                                                            d_loose.data_ptr(), d_ta.data_ptr(), d_push.data_ptr(), 1, lp, op, d_ctrl=c,
                                                                            d_plant=d_plant.data_ptr(), stream=sp)
        for kind, d_s in (("identity", d_ident), ("noisy", d_noisy)):
            calls[name + "_" + kind] = lambda c=c, d_s=d_s: s.loop_run_sensing_device(B, d_st.data_ptr(), T, d_oc.data_ptr(), d_s.data_ptr(), d_sn.data_ptr(),
                                                                                      d_act.data_ptr(), d_li.data_ptr(), d_loose.data_ptr(), d_ta.data_ptr(),
                                                                                      d_push.data_ptr(), 1, lp, op, d_ctrl=c, d_plant=d_plant.data_ptr(),
                                                                                      stream=sp)
    times, bits, seen = {k: [] for k in calls}, {}, {}
    for r in range(a.warmup + a.reps):
        for k, fn in calls.items():
            with torch.cuda.stream(stream):
                d_st.copy_(d_st0)
                d_oc.copy_(d_oc0)
                d_ta.copy_(d_ta0)
                d_li.copy_(d_li0)
                d_sn.copy_(d_sn0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if r >= a.warmup:
                times[k].append(e0.elapsed_time(e1))
            bits[k] = (d_st.cpu().numpy().tobytes(), d_oc.cpu().numpy().tobytes(), d_ta.cpu().numpy().tobytes(), d_li.cpu().numpy().tobytes())
            seen[k] = d_sn.cpu().numpy().view(pkg.SENSE_SEEN_DTYPE).reshape(B)
    forms = {"plant": s.loop_instances_plan(B, False, False), "ctrl_plant": s.loop_instances_plan(B, True, False)}
    s.close()
    ms = {k: float(np.median(v)) for k, v in times.items()}
    row = {"N": N, "B": B, "ticks": T, "records": a.records, "policy": a.policy}
    for k in ("plant", "ctrl_plant"):
        q = k + "_actuation"
        row.update({q + "_ms": ms[q], k + "_form": forms[k], q + "_spread": (max(times[q]) - min(times[q])) / ms[q]})
        print(f"N={N:2d} B={B:6d} {k:10s} {forms[k]}: actuation call {ms[q]:9.3f} ms (min {min(times[q]):.3f}, max {max(times[q]):.3f}, spread "
              f"{100 * row[q + '_spread']:.1f} %)", flush=True)
        for kind, what in (("identity", "identity records"), ("noisy", "12 noisy channels, seen")):
            g = k + "_" + kind
            same = bits[g] == bits[q]
            row.update({g + "_ms": ms[g], g + "_ratio": ms[g] / ms[q], g + "_spread": (max(times[g]) - min(times[g])) / ms[g],
                        g + "_same_bytes_as_actuation": same, g + "_measurements": int(seen[g]["ticks"].sum())})
            print(f"    sensing call, {what:24s} {ms[g]:9.3f} ms (min {min(times[g]):.3f}, max {max(times[g]):.3f}, spread "
                  f"{100 * row[g + '_spread']:.1f} %)   sensing / actuation {row[g + '_ratio']:.4f}   the actuation call's bytes: {same}   "
                  f"measurements formed: {row[g + '_measurements']}", flush=True)
    return row


def gaits(pkg, lib, torch, N, B, a):
    """the sensing call (identity sensing records: --sensing's identity case, the same fleet and records) against the gait call, with
    identity gait records and with a mixed-gait fleet (see the module docstring)"""
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    lp = pkg.default_loop_params(lib)
    T = a.ticks
    rng = np.random.default_rng(5)
    cmds = np.zeros((B, 7))
    cmds[:, 0] = rng.uniform(-0.4, 0.4, B); cmds[:, 1] = rng.uniform(-0.15, 0.15, B)
    cmds[:, 2] = rng.uniform(0.26, 0.32, B); cmds[:, 5] = rng.uniform(-0.4, 0.4, B)
    cmds[:, 6] = (rng.random(B) < 0.85).astype(float)
    stand = cmds.copy(); stand[:, 6] = 0.0
    st = pkg.loop_states(stand, lp, height=0.3, yaw=rng.uniform(-3, 3, B), lib=lib)
    s = pkg.Solver(p, B, device=0, lib=lib)
    s.set_instances_policy(a.policy if a.policy != "both" else "wave")
    s.prepare(B)
    s.prepare_instances()
    st = s.loop_run(st, 6, lp)
    st["movement_mode"] = cmds[:, 6]
    if a.records == "random":
        ctrl = pkg.random_go1_variants(B, seed=12, base=p)
        ctrl["mu"] = np.maximum(ctrl["mu"], 0.5)
        plant = pkg.random_go1_plants(B, seed=11, base=p, payload=(-1.0, 3.0), force=(0.0, 10.0))
    else:
        ctrl, plant = pkg.instance_params(p, B), pkg.plant_params(p, B)
    push = pkg.random_go1_pushes(B, seed=13, per_robot=1, impulse=(1.0, 5.0), dt=lp.dt)
    push["start_tick"] += 1e9      # beyond any run
    loose = pkg.ground_params(B)
    loose["mu"], loose["fz_max"] = 10.0, 1e4
    mixed = pkg.random_go1_gaits(B, seed=15)
    # the mixed fleet starts in its gaits' own states (the identity runs from the trot's: the sensing call's robots)
    st_mixed = pkg.loop_states_set_gait(st, mixed, lib)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).cuda()      # noqa: E731
    d_st0, d_oc0, d_ta0, d_ctrl, d_plant, d_push = dev(st), dev(pkg.loop_outcomes(B, lib)), dev(pkg.ground_tallies(B)), dev(ctrl), dev(plant), dev(push)
    d_stm0 = dev(st_mixed)
    d_li0, d_sn0 = dev(pkg.actuation_lines(B, pkg.stand_forces_body(p.mass))), dev(pkg.sense_seen(B))
    d_loose, d_act, d_sense = dev(loose), dev(pkg.actuation_params(B)), dev(pkg.sense_params(B))
    d_ident, d_mixed = dev(pkg.gait_params(B, lp=lp)), dev(mixed)
    d_st, d_oc, d_ta, d_li, d_sn = d_st0.clone(), d_oc0.clone(), d_ta0.clone(), d_li0.clone(), d_sn0.clone()
    op = pkg.default_outcome_params(lib)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    torch.cuda.synchronize()
    calls = {}
    for name, c in (("plant", 0), ("ctrl_plant", d_ctrl.data_ptr())):
        calls[name + "_sensing"] = lambda c=c: s.loop_run_sensing_device(B, d_st.data_ptr(), T, d_oc.data_ptr(), d_sense.data_ptr(), d_sn.data_ptr(),
                                                                        d_act.data_ptr(), d_li.data_ptr(), d_loose.data_ptr(), d_ta.data_ptr(),
                                                                        d_push.data_ptr(), 1, lp, op, d_ctrl=c, d_plant=d_plant.data_ptr(), stream=sp)
        for kind, d_g in (("identity", d_ident), ("mixed", d_mixed)):
            calls[name + "_" + kind] = lambda c=c, d_g=d_g: s.loop_run_gaits_device(B, d_st.data_ptr(), T, d_oc.data_ptr(), d_g.data_ptr(), d_sense.data_ptr(),
                                                                                    d_sn.data_ptr(), d_act.data_ptr(), d_li.data_ptr(), d_loose.data_ptr(),
                                                                                    d_ta.data_ptr(), d_push.data_ptr(), 1, lp, op, d_ctrl=c,
                                                                                    d_plant=d_plant.data_ptr(), stream=sp)
    times, bits, fin = {k: [] for k in calls}, {}, {}
    for r in range(a.warmup + a.reps):
        for k, fn in calls.items():
            with torch.cuda.stream(stream):
                d_st.copy_(d_stm0 if k.endswith("_mixed") else d_st0)
                d_oc.copy_(d_oc0)
                d_ta.copy_(d_ta0)
                d_li.copy_(d_li0)
                d_sn.copy_(d_sn0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if r >= a.warmup:
                times[k].append(e0.elapsed_time(e1))
            bits[k] = (d_st.cpu().numpy().tobytes(), d_oc.cpu().numpy().tobytes(), d_ta.cpu().numpy().tobytes(), d_li.cpu().numpy().tobytes())
            fin[k] = d_st.cpu().numpy().view(pkg.LOOP_STATE_DTYPE).reshape(B)
    forms = {"plant": s.loop_instances_plan(B, False, False), "ctrl_plant": s.loop_instances_plan(B, True, False)}
    s.close()
    ms = {k: float(np.median(v)) for k, v in times.items()}
    row = {"N": N, "B": B, "ticks": T, "records": a.records, "policy": a.policy}
    for k in ("plant", "ctrl_plant"):
        q = k + "_sensing"
        row.update({q + "_ms": ms[q], k + "_form": forms[k], q + "_spread": (max(times[q]) - min(times[q])) / ms[q]})
        print(f"N={N:2d} B={B:6d} {k:10s} {forms[k]}: sensing call {ms[q]:9.3f} ms (min {min(times[q]):.3f}, max {max(times[q]):.3f}, spread "
              f"{100 * row[q + '_spread']:.1f} %)", flush=True)
        for kind, what in (("identity", "identity records"), ("mixed", "six gaits, 1.5 - 3 Hz")):
            g = k + "_" + kind
            same = bits[g] == bits[q]
            sets = len({tuple(r) for r in fin[g]["contacts"].astype(int).tolist()})
            ok = int(np.isin(fin[g]["status"], (pkg.OK, pkg.MAX_ITER)).sum())
            row.update({g + "_ms": ms[g], g + "_ratio": ms[g] / ms[q], g + "_spread": (max(times[g]) - min(times[g])) / ms[g],
                        g + "_same_bytes_as_sensing": same, g + "_stance_sets_in_last_tick": sets, g + "_robots_ok": ok,
                        g + "_mean_iterations": float(fin[g]["iterations"].mean())})
            print(f"    gait call, {what:22s} {ms[g]:9.3f} ms (min {min(times[g]):.3f}, max {max(times[g]):.3f}, spread "
                  f"{100 * row[g + '_spread']:.1f} %)   gait / sensing {row[g + '_ratio']:.4f}   the sensing call's bytes: {same}   "
                  f"stance sets in the last tick: {sets}, robots OK: {ok}, its mean iterations {row[g + '_mean_iterations']:.2f}", flush=True)
    return row


def motors(pkg, lib, torch, N, B, a):
    """the gaits call (--gaits' identity case: the same fleet and records) against the motor call, with +inf limits and with the
    random limits of random_go1_motors (see the module docstring)"""
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    lp = pkg.default_loop_params(lib)
    T = a.ticks
    rng = np.random.default_rng(5)
    cmds = np.zeros((B, 7))
    cmds[:, 0] = rng.uniform(-0.4, 0.4, B); cmds[:, 1] = rng.uniform(-0.15, 0.15, B)
    cmds[:, 2] = rng.uniform(0.26, 0.32, B); cmds[:, 5] = rng.uniform(-0.4, 0.4, B)
    cmds[:, 6] = (rng.random(B) < 0.85).astype(float)
    stand = cmds.copy(); stand[:, 6] = 0.0
    st = pkg.loop_states(stand, lp, height=0.3, yaw=rng.uniform(-3, 3, B), lib=lib)
    s = pkg.Solver(p, B, device=0, lib=lib)
    s.set_instances_policy(a.policy if a.policy != "both" else "wave")
    s.prepare(B)
    s.prepare_instances()
    st = s.loop_run(st, 6, lp)
    st["movement_mode"] = cmds[:, 6]
    if a.records == "random":
        ctrl = pkg.random_go1_variants(B, seed=12, base=p)
        ctrl["mu"] = np.maximum(ctrl["mu"], 0.5)
        plant = pkg.random_go1_plants(B, seed=11, base=p, payload=(-1.0, 3.0), force=(0.0, 10.0))
    else:
        ctrl, plant = pkg.instance_params(p, B), pkg.plant_params(p, B)
    push = pkg.random_go1_pushes(B, seed=13, per_robot=1, impulse=(1.0, 5.0), dt=lp.dt)
    push["start_tick"] += 1e9      # beyond any run
    loose = pkg.ground_params(B)
    loose["mu"], loose["fz_max"] = 10.0, 1e4
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).cuda()      # noqa: E731
    d_st0, d_oc0, d_ta0, d_ctrl, d_plant, d_push = dev(st), dev(pkg.loop_outcomes(B, lib)), dev(pkg.ground_tallies(B)), dev(ctrl), dev(plant), dev(push)
    d_li0, d_sn0, d_mt0 = dev(pkg.actuation_lines(B, pkg.stand_forces_body(p.mass))), dev(pkg.sense_seen(B)), dev(pkg.motor_tallies(B, lib))
    d_loose, d_act, d_sense, d_gait = dev(loose), dev(pkg.actuation_params(B)), dev(pkg.sense_params(B)), dev(pkg.gait_params(B, lp=lp))
    d_free, d_bind = dev(pkg.motor_params(B)), dev(pkg.random_go1_motors(B, seed=16, scale=(a.tau_scale_lo, a.tau_scale_hi)))
    d_st, d_oc, d_ta, d_li, d_sn, d_mt = d_st0.clone(), d_oc0.clone(), d_ta0.clone(), d_li0.clone(), d_sn0.clone(), d_mt0.clone()
    op = pkg.default_outcome_params(lib)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    torch.cuda.synchronize()
    calls = {}
    for name, c in (("plant", 0), ("ctrl_plant", d_ctrl.data_ptr())):
        calls[name + "_gaits"] = lambda c=c: s.loop_run_gaits_device(B, d_st.data_ptr(), T, d_oc.data_ptr(), d_gait.data_ptr(), d_sense.data_ptr(),
                                                                    d_sn.data_ptr(), d_act.data_ptr(), d_li.data_ptr(), d_loose.data_ptr(),
                                                                    d_ta.data_ptr(), d_push.data_ptr(), 1, lp, op, d_ctrl=c,
                                                                    d_plant=d_plant.data_ptr(), stream=sp)
        for kind, d_m in (("free", d_free), ("binding", d_bind)):
            calls[name + "_" + kind] = lambda c=c, d_m=d_m: s.loop_run_motors_device(B, d_st.data_ptr(), T, d_oc.data_ptr(), d_m.data_ptr(), d_mt.data_ptr(),
                                                                                     None, d_gait.data_ptr(), d_sense.data_ptr(), d_sn.data_ptr(),
                                                                                     d_act.data_ptr(), d_li.data_ptr(), d_loose.data_ptr(),
                                                                                     d_ta.data_ptr(), d_push.data_ptr(), 1, lp, op, d_ctrl=c,
                                                                                     d_plant=d_plant.data_ptr(), stream=sp)
    times, bits, fin, tal = {k: [] for k in calls}, {}, {}, {}
    for r in range(a.warmup + a.reps):
        for k, fn in calls.items():
            with torch.cuda.stream(stream):
                d_st.copy_(d_st0)
                d_oc.copy_(d_oc0)
                d_ta.copy_(d_ta0)
                d_li.copy_(d_li0)
                d_sn.copy_(d_sn0)
                d_mt.copy_(d_mt0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if r >= a.warmup:
                times[k].append(e0.elapsed_time(e1))
            bits[k] = (d_st.cpu().numpy().tobytes(), d_oc.cpu().numpy().tobytes(), d_ta.cpu().numpy().tobytes(), d_li.cpu().numpy().tobytes())
            fin[k] = d_st.cpu().numpy().view(pkg.LOOP_STATE_DTYPE).reshape(B)
            tal[k] = d_mt.cpu().numpy().view(pkg.MOTOR_TALLY_DTYPE).reshape(B)
    forms = {"plant": s.loop_instances_plan(B, False, False), "ctrl_plant": s.loop_instances_plan(B, True, False)}
    s.close()
    ms = {k: float(np.median(v)) for k, v in times.items()}
    row = {"N": N, "B": B, "ticks": T, "records": a.records, "policy": a.policy}
    for k in ("plant", "ctrl_plant"):
        q = k + "_gaits"
        row.update({q + "_ms": ms[q], k + "_form": forms[k], q + "_spread": (max(times[q]) - min(times[q])) / ms[q]})
        print(f"N={N:2d} B={B:6d} {k:10s} {forms[k]}: gaits call {ms[q]:9.3f} ms (min {min(times[q]):.3f}, max {max(times[q]):.3f}, spread "
              f"{100 * row[q + '_spread']:.1f} %)", flush=True)
        for kind, what in (("free", "+inf limits"), ("binding", f"Go1 limits x U({a.tau_scale_lo}, {a.tau_scale_hi})")):
            g = k + "_" + kind
            same = bits[g] == bits[q]
            ok = int(np.isin(fin[g]["status"], (pkg.OK, pkg.MAX_ITER)).sum())
            t = tal[g]
            peak = t["peak_tau"].reshape(B, 4, 3).max(axis=1)
            row.update({g + "_ms": ms[g], g + "_ratio": ms[g] / ms[q], g + "_spread": (max(times[g]) - min(times[g])) / ms[g],
                        g + "_same_bytes_as_gaits": same, g + "_robots_ok": ok, g + "_robots_clipped": int((t["clipped_ticks"] > 0).sum()),
                        g + "_peak_tau_by_type_max": peak.max(axis=0).tolist(), g + "_peak_tau_by_type_median": np.median(peak, axis=0).tolist(),
                        g + "_unreachable_leg_ticks": float(t["unreachable_leg_ticks"].sum())})
            print(f"    motor call, {what:28s} {ms[g]:9.3f} ms (min {min(times[g]):.3f}, max {max(times[g]):.3f}, spread "
                  f"{100 * row[g + '_spread']:.1f} %)   motor / gaits {row[g + '_ratio']:.4f}   the gaits call's bytes: {same}   "
                  f"robots OK: {ok}, clipped: {row[g + '_robots_clipped']}, peak torque hip / thigh / calf [N m] max "
                  f"{np.round(peak.max(axis=0), 2).tolist()} median {np.round(np.median(peak, axis=0), 2).tolist()}, unreachable leg-ticks "
                  f"{row[g + '_unreachable_leg_ticks']:.0f}", flush=True)
    return row


def warm_records(pkg, lib, torch, N, B, a):
    """cold against warm, the plain loop and the call with controller + plant records (see the module docstring)"""
    lp_c = pkg.default_loop_params(lib)
    lp_w = pkg.default_loop_params(lib)
    lp_w.warm_start = 1.0
    convex = a.model == "convex"
    defaults = pkg.default_convex_params if convex else pkg.default_params
    p_c = defaults(N, pkg.MODE_CONVERGED, lib)
    p_w = defaults(N, pkg.MODE_CONVERGED, lib)
    p_w.ipm_mu0 = a.mu0
    T = a.ticks
    rng = np.random.default_rng(5)
    cmds = np.zeros((B, 7))
    cmds[:, 0] = rng.uniform(-0.4, 0.4, B); cmds[:, 1] = rng.uniform(-0.15, 0.15, B)
    cmds[:, 2] = rng.uniform(0.26, 0.32, B); cmds[:, 5] = rng.uniform(-0.4, 0.4, B)
    cmds[:, 6] = (rng.random(B) < 0.85).astype(float)
    if convex:      # (this controller has no command for a robot that stands: tests/test_gpu_lane.py)
        cmds[cmds[:, 6] == 0, :2] = 0.0
        cmds[cmds[:, 6] == 0, 5] = 0.0
    stand = cmds.copy(); stand[:, 6] = 0.0
    st = pkg.loop_states(stand, lp_c, height=0.3, yaw=rng.uniform(-3, 3, B), lib=lib)
    policies = ("wave", "auto") if a.policy == "both" else (a.policy,)
    handles = {}
    for kind, p in (("cold", p_c), ("warm", p_w)):
        h = pkg.Solver(p, B, device=0, lib=lib)
        if convex:
            h.set_convex_records(True)
            h.set_convex_lane_records(True)      # (takes effect under AUTO only)
            h.set_convex_warm_records(kind == "warm")
        elif kind == "warm":
            h.set_loop_warm_records(True)
        for pol in policies:      # (the buffers of every policy asked for: allocated before anything is timed)
            h.set_instances_policy(pol)
            h.prepare(B)
        h.prepare_instances()
        handles[kind] = h
    st = handles["cold"].loop_run(st, 6, lp_c)
    st["movement_mode"] = cmds[:, 6]
    if a.records == "random":
        ctrl = (pkg.random_go1_convex_variants if convex else pkg.random_go1_variants)(B, seed=12, base=p_c)
        ctrl["mu"] = np.maximum(ctrl["mu"], 0.5)
        plant = pkg.random_go1_plants(B, seed=11, base=p_c, payload=(-1.0, 3.0), force=(0.0, 10.0))
    else:
        ctrl, plant = pkg.instance_params(p_c, B), pkg.plant_params(p_c, B)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).cuda()      # noqa: E731
    d_st0, d_ctrl, d_plant = dev(st), dev(ctrl), dev(plant)
    d_st = d_st0.clone()
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    torch.cuda.synchronize()

    def rec_call(kind, pol):
        h = handles[kind]
        h.set_instances_policy(pol)
        h.loop_run_instances_device(B, d_st.data_ptr(), T, lp_w if kind == "warm" else lp_c, d_ctrl=d_ctrl.data_ptr(), d_plant=d_plant.data_ptr(),
                                    stream=sp)

    calls, forms = {}, {}
    for kind, lp in (("cold", lp_c), ("warm", lp_w)):
        calls["plain_" + kind] = lambda kind=kind, lp=lp: handles[kind].loop_run_device(B, d_st.data_ptr(), T, lp, stream=sp)
        for pol in policies:
            calls[f"records_{pol}_{kind}"] = lambda kind=kind, pol=pol: rec_call(kind, pol)
            handles[kind].set_instances_policy(pol)
            forms[f"records_{pol}_{kind}"] = handles[kind].loop_instances_plan(B, True, kind == "warm")
    times, its = {k: [] for k in calls}, {}
    for r in range(a.warmup + a.reps):
        for k, fn in calls.items():
            with torch.cuda.stream(stream):
                d_st.copy_(d_st0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if r >= a.warmup:
                times[k].append(e0.elapsed_time(e1))
            x = d_st.cpu().numpy().view(pkg.LOOP_STATE_DTYPE).reshape(B)
            its[k] = (float(x["iterations"].mean()), int((x["status"] != 0).sum()))
    for h in handles.values():
        h.close()
    ms = {k: float(np.median(v)) for k, v in times.items()}
    row = {"N": N, "B": B, "ticks": T, "records": a.records, "mu0_warm": a.mu0, "model": a.model}
    for k in calls:
        row[k + "_ms"] = ms[k]
        row[k + "_Mrobot_ticks_s"] = B * T / ms[k] / 1e3
        row[k + "_form"] = forms.get(k)
        row[k + "_last_tick_iterations"] = its[k][0]
    row["plain_warm_over_cold"] = ms["plain_cold"] / ms["plain_warm"]
    print(f"N={N:2d} B={B:6d}  plain loop cold {row['plain_cold_Mrobot_ticks_s']:7.3f} M/s   warm {row['plain_warm_Mrobot_ticks_s']:7.3f} M/s   "
          f"warm / cold x{row['plain_warm_over_cold']:.3f}   (ms min/median/max cold {min(times['plain_cold']):.3f} / {ms['plain_cold']:.3f} / "
          f"{max(times['plain_cold']):.3f}, warm {min(times['plain_warm']):.3f} / {ms['plain_warm']:.3f} / {max(times['plain_warm']):.3f}; last tick's "
          f"mean iterations {its['plain_cold'][0]:.2f} / {its['plain_warm'][0]:.2f})", flush=True)
    for pol in policies:
        c, w = f"records_{pol}_cold", f"records_{pol}_warm"
        row[f"records_{pol}_warm_over_cold"] = ms[c] / ms[w]
        row[f"records_{pol}_gain_over_plain_gain"] = row[f"records_{pol}_warm_over_cold"] / row["plain_warm_over_cold"]
        row[f"records_{pol}_warm_over_plain_warm"] = ms["plain_warm"] / ms[w]
        print(f"            {a.records} ctrl+plant records, {pol}: cold {row[c + '_Mrobot_ticks_s']:7.3f} M/s {forms[c]}   warm "
              f"{row[w + '_Mrobot_ticks_s']:7.3f} M/s {forms[w]}   warm / cold x{row[f'records_{pol}_warm_over_cold']:.3f} "
              f"({row[f'records_{pol}_gain_over_plain_gain']:.3f} of the plain loop's ratio; {row[f'records_{pol}_warm_over_plain_warm']:.3f} of the "
              f"plain warm loop)   ms min/median/max cold {min(times[c]):.3f} / {ms[c]:.3f} / {max(times[c]):.3f}, warm {min(times[w]):.3f} / "
              f"{ms[w]:.3f} / {max(times[w]):.3f}; last tick's mean iterations {its[c][0]:.2f} / {its[w][0]:.2f}, robots not OK {its[c][1]} / {its[w][1]}",
              flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--sizes", default=DEFAULT_SIZES)
    ap.add_argument("--json", default=None)
    ap.add_argument("--outcomes", action="store_true")
    ap.add_argument("--stop", action="store_true")
    ap.add_argument("--pushes", action="store_true")
    ap.add_argument("--per-robot", type=int, default=1)
    ap.add_argument("--ground", action="store_true")
    ap.add_argument("--actuation", action="store_true")
    ap.add_argument("--sensing", action="store_true")
    ap.add_argument("--gaits", action="store_true")
    ap.add_argument("--motors", action="store_true")
    ap.add_argument("--tau-scale-lo", type=float, default=0.15)
    ap.add_argument("--tau-scale-hi", type=float, default=0.6)
    ap.add_argument("--policy", choices=("wave", "auto", "both"), default="wave")
    ap.add_argument("--records", choices=("uniform", "random"), default="uniform")
    ap.add_argument("--warm-records", action="store_true")
    ap.add_argument("--mu0", type=float, default=1e-6)
    ap.add_argument("--model", choices=("quat", "convex"), default="quat")
    a = ap.parse_args()
    import torch

    pkg = load_pkg()
    lib = pkg.load_library()
    rows = []
    if a.stop and not a.outcomes:
        ap.error("--stop goes with --outcomes")
    convex = a.model == "convex"
    if convex and (a.pushes or a.stop or a.ground or a.actuation or a.sensing or a.gaits or a.motors):
        ap.error("--model convex goes with the default comparison, --outcomes and --warm-records")
    for item in a.sizes.split(","):
        N, B = (int(x) for x in item.split(":"))
        policies = ("wave", "auto") if a.policy == "both" else (a.policy,)
        if a.pushes:
            rows.append(pushes(pkg, lib, torch, N, B, a))
            continue
        if a.ground:
            rows.append(ground(pkg, lib, torch, N, B, a))
            continue
        if a.actuation:
            rows.append(actuation(pkg, lib, torch, N, B, a))
            continue
        if a.sensing:
            rows.append(sensing(pkg, lib, torch, N, B, a))
            continue
        if a.gaits:
            rows.append(gaits(pkg, lib, torch, N, B, a))
            continue
        if a.motors:
            rows.append(motors(pkg, lib, torch, N, B, a))
            continue
        if a.warm_records:
            rows.append(warm_records(pkg, lib, torch, N, B, a))
            continue
        if a.stop:
            if a.policy == "wave":      # (as before the policy existed: plant records only)
                rows.append(falling(pkg, lib, torch, N, B, a))
            else:
                rows.extend(falling(pkg, lib, torch, N, B, a, pol) for pol in policies)
            continue
        p = (pkg.default_convex_params if convex else pkg.default_params)(N, pkg.MODE_CONVERGED, lib)
        lp = pkg.default_loop_params(lib)
        rng = np.random.default_rng(5)
        cmds = np.zeros((B, 7))
        cmds[:, 0] = rng.uniform(-0.4, 0.4, B); cmds[:, 1] = rng.uniform(-0.15, 0.15, B)
        cmds[:, 2] = rng.uniform(0.26, 0.32, B); cmds[:, 5] = rng.uniform(-0.4, 0.4, B)
        cmds[:, 6] = (rng.random(B) < 0.85).astype(float)
        if convex:      # (this controller has no command for a robot that stands: tests/test_gpu_lane.py)
            cmds[cmds[:, 6] == 0, :2] = 0.0
            cmds[cmds[:, 6] == 0, 5] = 0.0
        stand = cmds.copy(); stand[:, 6] = 0.0
        st = pkg.loop_states(stand, lp, height=0.3, yaw=rng.uniform(-3, 3, B), lib=lib)
        s = pkg.Solver(p, B, device=0, lib=lib)
        if convex:
            s.set_convex_records(True)
            s.set_convex_lane_records(True)      # (takes effect under AUTO only)
        for pol in policies:      # (the buffers of every policy asked for: allocated before anything is timed)
            s.set_instances_policy(pol)
            s.prepare(B)
        s.prepare_instances()
        st = s.loop_run(st, 6, lp)
        st["movement_mode"] = cmds[:, 6]
        d_st0 = torch.from_numpy(st.view(np.uint8).copy()).cuda()
        d_st = d_st0.clone()
        if a.records == "random":
            ctrl = (pkg.random_go1_convex_variants if convex else pkg.random_go1_variants)(B, seed=12, base=p)
            ctrl["mu"] = np.maximum(ctrl["mu"], 0.5)
            plant = pkg.random_go1_plants(B, seed=11, base=p, payload=(-1.0, 3.0), force=(0.0, 10.0))
        else:
            ctrl, plant = pkg.instance_params(p, B), pkg.plant_params(p, B)
        if convex:      # (the buffers of the calls with records, the outcome scratch included: before anything is timed)
            s.loop_run_instances(st, 0, lp, ctrl=ctrl, plant=plant)
        d_ctrl = torch.from_numpy(ctrl.view(np.uint8).copy()).cuda()
        d_plant = torch.from_numpy(plant.view(np.uint8).copy()).cuda()
        stream = torch.cuda.Stream()
        sp = stream.cuda_stream
        torch.cuda.synchronize()
        T = a.ticks
        # the calls with controller records: "ctrl_plant" under the first policy asked for, "ctrl_plant_auto" the second of both
        suffix = {pol: ("" if i == 0 else "_" + pol) for i, pol in enumerate(policies)}

        def ctrl_call(pol):
            s.set_instances_policy(pol)
            s.loop_run_instances_device(B, d_st.data_ptr(), T, lp, d_ctrl=d_ctrl.data_ptr(), d_plant=d_plant.data_ptr(), stream=sp)

        def ctrl_outcomes_call(pol):
            s.set_instances_policy(pol)
            s.loop_run_outcomes_device(B, d_st.data_ptr(), T, d_oc.data_ptr(), lp, op, d_ctrl=d_ctrl.data_ptr(), d_plant=d_plant.data_ptr(),
                                       stream=sp)

        calls = {"plain": lambda: s.loop_run_device(B, d_st.data_ptr(), T, lp, stream=sp),
                 "plant": lambda: s.loop_run_instances_device(B, d_st.data_ptr(), T, lp, d_plant=d_plant.data_ptr(), stream=sp)}
        for pol in policies:
            calls["ctrl_plant" + suffix[pol]] = lambda pol=pol: ctrl_call(pol)
        if a.outcomes:
            op = pkg.default_outcome_params(lib)
            d_oc0 = torch.from_numpy(pkg.loop_outcomes(B, lib).view(np.uint8).copy()).cuda()
            d_oc = d_oc0.clone()
            calls["plant_outcomes"] = lambda: s.loop_run_outcomes_device(B, d_st.data_ptr(), T, d_oc.data_ptr(), lp, op,
                                                                         d_plant=d_plant.data_ptr(), stream=sp)
            for pol in policies:
                calls["ctrl_plant" + suffix[pol] + "_outcomes"] = lambda pol=pol: ctrl_outcomes_call(pol)
            order = ["plain", "plant", "plant_outcomes"]
            for pol in policies:
                order += ["ctrl_plant" + suffix[pol], "ctrl_plant" + suffix[pol] + "_outcomes"]
            calls = {k: calls[k] for k in order}
        times = {k: [] for k in calls}
        for r in range(a.warmup + a.reps):
            for k, fn in calls.items():
                with torch.cuda.stream(stream):
                    d_st.copy_(d_st0)
                    if a.outcomes:
                        d_oc.copy_(d_oc0)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                if r >= a.warmup:
                    times[k].append(e0.elapsed_time(e1))
        forms = {"plain": None, "plant": s.loop_instances_plan(B, False, False)}
        forms["plant_outcomes"] = forms["plant"]
        for pol in policies:
            s.set_instances_policy(pol)
            forms["ctrl_plant" + suffix[pol]] = forms["ctrl_plant" + suffix[pol] + "_outcomes"] = s.loop_instances_plan(B, True, False)
        s.close()
        ms = {k: float(np.median(v)) for k, v in times.items()}
        row = {"N": N, "B": B, "ticks": T, "records": a.records, "policy": policies[0], "model": a.model}
        for k in calls:
            row[k + "_ms"] = ms[k]
            row[k + "_Mrobot_ticks_s"] = B * T / ms[k] / 1e3
            row[k + "_form"] = forms[k]
        row["plant_ratio"] = row["plant_Mrobot_ticks_s"] / row["plain_Mrobot_ticks_s"]
        row["ctrl_plant_ratio"] = row["ctrl_plant_Mrobot_ticks_s"] / row["plain_Mrobot_ticks_s"]
        rows.append(row)
        print(f"N={N:2d} B={B:6d}  plain {row['plain_Mrobot_ticks_s']:7.3f} M/s   plant {row['plant_Mrobot_ticks_s']:7.3f} M/s "
              f"({row['plant_ratio']:.3f}, {forms['plant']})   ctrl+plant {row['ctrl_plant_Mrobot_ticks_s']:7.3f} M/s "
              f"({row['ctrl_plant_ratio']:.3f}, {policies[0]} policy, {forms['ctrl_plant']})", flush=True)
        for pol in policies[1:]:
            k = "ctrl_plant" + suffix[pol]
            row[k + "_ratio"] = row[k + "_Mrobot_ticks_s"] / row["plain_Mrobot_ticks_s"]
            row[k + "_over_" + policies[0]] = row[k + "_Mrobot_ticks_s"] / row["ctrl_plant_Mrobot_ticks_s"]
            print(f"            {a.records} records, ctrl+plant under {pol}: {row[k + '_Mrobot_ticks_s']:7.3f} M/s ({row[k + '_ratio']:.3f} of plain, "
                  f"{forms[k]})   {pol} / {policies[0]} x{row[k + '_over_' + policies[0]]:.3f}   ms min/median/max {min(times[k]):.3f} / "
                  f"{ms[k]:.3f} / {max(times[k]):.3f} against {min(times['ctrl_plant']):.3f} / {ms['ctrl_plant']:.3f} / {max(times['ctrl_plant']):.3f}",
                  flush=True)
        if a.outcomes:
            for k in ["plant"] + ["ctrl_plant" + suffix[pol] for pol in policies]:
                spread = (max(times[k]) - min(times[k])) / ms[k]
                row[k + "_outcomes_ratio"] = ms[k + "_outcomes"] / ms[k]
                row[k + "_spread"] = spread
                print(f"            {k:10s} instances call {ms[k]:9.3f} ms (min {min(times[k]):.3f}, max {max(times[k]):.3f})   outcome call "
                      f"{ms[k + '_outcomes']:9.3f} ms (min {min(times[k + '_outcomes']):.3f}, max {max(times[k + '_outcomes']):.3f})   "
                      f"outcome / instances {row[k + '_outcomes_ratio']:.4f}", flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
