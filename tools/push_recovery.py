#!/usr/bin/env python3
"""Push recovery of the trotting Go1 on the device: a fleet under a grid of impulse magnitude x 8 directions x start tick over one
gait period (91 ticks of 5 ms at 2.2 Hz), every robot shoved once (qmpc_loop_run_pushes, one window per robot), the share of robots
still up per cell from the outcome records.  The robots of a cell differ in their true plant (random_go1_plants: payload and
inertia); the controller is the handle's and is not told about the push.
    python tools/push_recovery.py [--impulses 2,4,6,8,10] [--starts 13] [--length 10] [--per-cell 8] [--speed 0.3] [--settle 60]
                                  [--recover 200] [--horizon 10] [--controller quat|convex|both] [--ctrl-records] [--warm] [--json FILE]
                                  [--mu-true LO HI [--mu-steps 5]] [--delay LO HI] [--tau LO HI [--tau-steps 3]]
                                  [--gyro-bias LO HI] [--pos-noise LO HI] [--att-noise LO HI] [--vel-noise LO HI] [--sense-steps 3]
                                  [--gait NAME[,NAME...]] [--gait-freq LO HI [--gait-steps 3]] [--tau-max S]
Every robot stands for 6 ticks, trots at --speed for --settle ticks, is shoved at tick 6 + settle + start for --length ticks with
force impulse / (length dt) in its cell's direction (0 degrees: ahead, 90: to its left), and trots on until --recover ticks after
the last start.  Down: below 0.15 m or tilted beyond 60 degrees (qmpc_default_outcome_params); stop_when_down halts a fallen robot.
Prints one table per impulse (rows: start tick in the gait period, columns: direction) and the marginals.  The figures are whatever
the run gives.
--controller: QuatMpc (default), ConvexMpc (a handle that opted in with qmpc_set_convex_records), or both -- the same pushes,
plants and commands under each controller, one summary per controller.  --horizon is then each controller's horizon.
--mu-true LO HI: the true-friction axis.  The grid is repeated on --mu-steps grounds whose Coulomb coefficient runs from LO to HI
(qmpc_loop_run_ground: the plant delivers what that ground allows, the controller keeps assuming its own mu), and a table of falls
per (impulse, mu_true) cell with the ground tallies is printed after the tables above, which then pool the grounds.
--delay LO HI, --tau LO HI: the time axes.  The grid is repeated for every actuation delay of LO .. HI ticks (integers, at most 8) and
for --tau-steps actuator time constants from LO to HI seconds (qmpc_loop_run_actuation: the plant receives the command of `delay`
ticks ago through a first-order lag, alpha = 1 - exp(-dt / tau); the controller is not told; the delay lines start from the stand
force m g / 4 per leg), and a table of falls per (impulse, delay, tau) cell is printed after the tables above, which then pool them.
--gyro-bias LO HI, --pos-noise LO HI, --att-noise LO HI, --vel-noise LO HI: the estimator axes (qmpc_loop_run_sensing: the
controller reads the true state plus a bias and reproducible bounded noise; the plant works on the truth).  The grid is repeated
for --sense-steps gyro biases from LO to HI rad/s (on all three body axes, the signs by the robot's place in its cell) and for
--sense-steps noise levels: level j takes the j-th of --sense-steps values from LO to HI of each noise given -- position [m],
attitude [rad], world-frame velocity [m/s], standard deviation per axis -- so the noises rise together.  Every robot draws its own
noise (seed = its index).  A table of falls per (impulse, gyro bias, noise level) cell is printed after the tables above, which
then pool them.
--gait NAME[,NAME...], --gait-freq LO HI: the gait axes (qmpc_loop_run_gaits: every robot walks its own gait).  The grid is repeated
for every named gait (trot, pace, bound, trot_overlap, crawl, amble) and for --gait-steps frequencies from LO to HI Hz (without
--gait-freq: the loop's 2.2 Hz).  The six standing ticks put every leg at its gait's starting phase.  The start ticks stay spread over
the 91 ticks of the 2.2 Hz period whatever the frequency.  A table of falls per (impulse, gait, frequency) cell is printed after the
tables above, which then pool them.  Without --gait and --gait-freq the call is the sensing call and the robots trot as before.

--tau-max S: the motor axis (qmpc_loop_run_motors: the foot force a stance leg delivers respects the joint torque limits).  Every robot
gets the Go1's 23.7 / 23.7 / 35.55 N m (hip, thigh, calf) times S.  After the tables above: per leg and joint the share of ticks the
joint saturated and the peak torque it was asked for (median and maximum over the robots).  S = inf limits nothing and reports the
torque the grid needs.
--ctrl-records: every robot also carries a controller record (the handle's values: the same controller) and the handle takes
QMPC_INSTANCES_AUTO, a ConvexMpc handle with qmpc_set_convex_lane_records as well -- the launch a sweep over per-robot controllers
takes: from the switch-over on the lane kernel with per-lane parameters under either controller.
--warm: the loops run warm-started (lp.warm_start = 1, ipm_mu0 = 1e-6).  With --ctrl-records the handle opts in to warm starts with
controller records: a QuatMpc handle with qmpc_set_loop_warm_records, a ConvexMpc handle with qmpc_set_convex_warm_records."""
import argparse
import importlib.util
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
PERIOD = 91      # ticks of 5 ms in one gait period at 2.2 Hz


def load_pkg():
    spec = importlib.util.spec_from_file_location("quaternion_mpc_amd", REPO / "quaternion-mpc_amd" / "__init__.py",
                                                  submodule_search_locations=[str(REPO / "quaternion-mpc_amd")])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["quaternion_mpc_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--impulses", default="2,4,6,8,10", help="N s")
    ap.add_argument("--starts", type=int, default=13, help="start ticks, evenly spread over the gait period")
    ap.add_argument("--length", type=float, default=10.0, help="ticks the shove lasts")
    ap.add_argument("--per-cell", type=int, default=8)
    ap.add_argument("--speed", type=float, default=0.3)
    ap.add_argument("--settle", type=int, default=60)
    ap.add_argument("--recover", type=int, default=200)
    ap.add_argument("--horizon", type=int, default=10)
    ap.add_argument("--json", default=None)
    ap.add_argument("--controller", choices=("quat", "convex", "both"), default="quat")
    ap.add_argument("--ctrl-records", action="store_true")
    ap.add_argument("--warm", action="store_true")
    ap.add_argument("--mu-true", type=float, nargs=2, default=None, metavar=("LO", "HI"))
    ap.add_argument("--mu-steps", type=int, default=5)
    ap.add_argument("--delay", type=int, nargs=2, default=None, metavar=("LO", "HI"))
    ap.add_argument("--tau", type=float, nargs=2, default=None, metavar=("LO", "HI"))
    ap.add_argument("--tau-steps", type=int, default=3)
    ap.add_argument("--gyro-bias", type=float, nargs=2, default=None, metavar=("LO", "HI"))
    ap.add_argument("--pos-noise", type=float, nargs=2, default=None, metavar=("LO", "HI"))
    ap.add_argument("--att-noise", type=float, nargs=2, default=None, metavar=("LO", "HI"))
    ap.add_argument("--vel-noise", type=float, nargs=2, default=None, metavar=("LO", "HI"))
    ap.add_argument("--sense-steps", type=int, default=3)
    ap.add_argument("--gait", default=None, help="names of quaternion_mpc_amd.GAITS, comma-separated")
    ap.add_argument("--gait-freq", type=float, nargs=2, default=None, metavar=("LO", "HI"))
    ap.add_argument("--gait-steps", type=int, default=3)
    ap.add_argument("--tau-max", type=float, default=None, metavar="S", help="the Go1's joint torque limits times S on every robot")
    a = ap.parse_args()
    pkg = load_pkg()
    lib = pkg.load_library()
    results = [run(a, pkg, lib, c) for c in (("quat", "convex") if a.controller == "both" else (a.controller,))]
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(results[0] if len(results) == 1 else results, indent=1) + "\n")


def run(a, pkg, lib, controller):
    impulses = [float(x) for x in a.impulses.split(",")]
    starts = [int(round(k * PERIOD / a.starts)) for k in range(a.starts)]
    angles = np.arange(8) * (np.pi / 4)
    # the grid, robot index = ((impulse, start, direction), member of the cell)
    mus = np.linspace(a.mu_true[0], a.mu_true[1], a.mu_steps) if a.mu_true else np.array([np.inf])
    delays = np.arange(a.delay[0], a.delay[1] + 1) if a.delay else np.array([0])
    taus = np.linspace(a.tau[0], a.tau[1], a.tau_steps) if a.tau else np.array([0.0])
    timed = bool(a.delay or a.tau)
    noises = {k: v for k, v in (("pos", a.pos_noise), ("att", a.att_noise), ("vel", a.vel_noise)) if v}
    gbs = np.linspace(a.gyro_bias[0], a.gyro_bias[1], a.sense_steps) if a.gyro_bias else np.array([0.0])
    levels = np.arange(a.sense_steps) if noises else np.array([0])
    sensed = bool(a.gyro_bias or noises)
    gaited = bool(a.gait or a.gait_freq)
    names = a.gait.split(",") if a.gait else ["trot"]
    unknown = [n for n in names if n not in pkg.GAITS]
    if unknown:
        raise SystemExit(f"--gait: unknown {unknown}; one of {', '.join(pkg.GAITS)}")
    freqs = np.linspace(a.gait_freq[0], a.gait_freq[1], a.gait_steps) if a.gait_freq else np.array([pkg.default_loop_params(lib).gait_freq])
    gi, gs, gd, gm, gl, gt, gb, gn, gg, gf, gk = (g.ravel() for g in np.meshgrid(np.arange(len(impulses)), np.arange(len(starts)), np.arange(8),
                                                                                 np.arange(len(mus)), np.arange(len(delays)), np.arange(len(taus)),
                                                                                 np.arange(len(gbs)), np.arange(len(levels)), np.arange(len(names)),
                                                                                 np.arange(len(freqs)), np.arange(a.per_cell), indexing="ij"))
    inner = len(names) * len(freqs) * a.per_cell      # the robots of one (..., gyro bias, noise level) cell
    tail = len(gbs) * len(levels) * inner      # the robots of one (impulse, start, direction, mu, delay, tau) cell
    members = len(mus) * len(delays) * len(taus) * tail
    B = gi.size
    convex = controller == "convex"
    p = (pkg.default_convex_params if convex else pkg.default_params)(a.horizon, pkg.MODE_CONVERGED, lib)
    lp = pkg.default_loop_params(lib)
    if a.warm:
        p.ipm_mu0 = 1e-6
        lp.warm_start = 1.0
    assert abs(1.0 / (lp.gait_freq * lp.dt) - PERIOD) < 0.5, (lp.gait_freq, lp.dt)
    cmd = [a.speed, 0.0, 0.30, 0.0, 0.0, 0.0, 0.0]
    st = pkg.loop_states([cmd] * B, lp, height=0.3, yaw=0.0, lib=lib)
    # (the same plants under either controller: around QuatMpc's Go1, whose mass is ConvexMpc's too)
    ground = None
    if a.mu_true:
        ground = pkg.ground_params(B)
        ground["mu"] = mus[gm][:, None]
    plant = pkg.random_go1_plants(B, seed=21, base=pkg.default_params(a.horizon, pkg.MODE_CONVERGED, lib), payload=(0.0, 3.0))
    push = pkg.push_params(B)
    t0 = 6 + a.settle
    push["start_tick"][:, 0] = t0 + np.asarray(starts, dtype=np.float64)[gs]
    push["ticks"][:, 0] = a.length
    mag = np.asarray(impulses)[gi] / (a.length * lp.dt)
    push["force_world"][:, 0, 0] = mag * np.cos(angles[gd])
    push["force_world"][:, 0, 1] = mag * np.sin(angles[gd])
    act = line = None
    if timed:
        act = pkg.actuation_params(B, delay_ticks=delays[gl], tau=taus[gt], dt=lp.dt)
        line = pkg.actuation_lines(B, pkg.stand_forces_body(p.mass))
    sense = None
    if sensed:
        signs = np.stack([np.where((gk >> b) & 1, -1.0, 1.0) for b in range(3)], axis=1)
        level = lambda r: np.linspace(r[0], r[1], a.sense_steps)[gn][:, None] * np.ones(3)      # noqa: E731
        sense = pkg.sense_params(B, seed=np.arange(B, dtype=np.float64), gyro_bias=gbs[gb][:, None] * signs,
                                 **{k + "_noise": level(r) for k, r in noises.items()})
    gait = pkg.gait_params(B, [names[k] for k in gg], gait_freq=freqs[gf]) if gaited else None
    op = pkg.default_outcome_params(lib, stop_when_down=True)
    s = pkg.Solver(p, B, device=0, lib=lib)
    if convex:
        s.set_convex_records(True)
    ctrl = None
    if a.ctrl_records:
        ctrl = pkg.instance_params(p, B)
        s.set_instances_policy("auto")
        if convex:
            s.set_convex_lane_records(True)
        if a.warm:
            (s.set_convex_warm_records if convex else s.set_loop_warm_records)(True)
    form = s.loop_instances_plan(B, ctrl is not None, a.warm)
    total = a.settle + PERIOD + a.recover
    w0 = time.perf_counter()
    # (gait = None: the sensing call; sense = None: the actuation call; act = None: the ground call; ground = None: the push call)
    # (motor = None: the gaits call)
    motor = pkg.motor_params(B, a.tau_max * np.asarray(pkg.GO1_TAU_MAX)) if a.tau_max is not None else None
    st, oc, ta, line, seen, mt = s.loop_run_motors(st, 6, motor, None, None, gait, sense, None, act, line, ground, push, lp, ctrl=ctrl, plant=plant,
                                                   op=op)
    st["movement_mode"] = 1.0
    st, oc, ta, line, seen, mt = s.loop_run_motors(st, total, motor, mt, None, gait, sense, seen, act, line, ground, push, lp, ctrl=ctrl,
                                                   plant=plant, op=op, outcomes=oc, tallies=ta)
    wall = time.perf_counter() - w0
    s.close()
    up = (oc["down_tick"] < 0).reshape(len(impulses), len(starts), 8, members)
    share = up.mean(axis=3)
    fell_before = int(((oc["down_tick"] >= 0) & (oc["down_tick"] <= push["start_tick"][:, 0])).sum())
    print(f"push recovery under {'ConvexMpc' if convex else 'QuatMpc'}: {B} robots ({len(impulses)} impulses x {len(starts)} start ticks x 8 directions x {members} plants), N={a.horizon}, "
          f"trot at {a.speed} m/s, shove of {a.length:g} ticks from tick {t0} + start, {6 + total} ticks in all, launch {form}, "
          f"{wall:.2f} s wall with the copies; {fell_before} robots were down before their shove began")
    print(f"solves: {pkg.summarize_outcomes(oc)['mean_iterations']:.2f} iterations on average, "
          f"{int(oc['rejected_ticks'].sum())} rejected, {int((oc['not_ok_ticks'] - oc['rejected_ticks']).sum())} at the iteration cap")
    head = "start " + " ".join(f"{int(np.degrees(x)):4d}d" for x in angles) + "    all"
    for i, imp in enumerate(impulses):
        print(f"\nimpulse {imp:g} N s ({imp / (a.length * lp.dt):.0f} N for {a.length:g} ticks): share still up at the end")
        print(head)
        for j, t in enumerate(starts):
            print(f"{t:5d} " + " ".join(f"{share[i, j, d]:5.2f}" for d in range(8)) + f"  {share[i, j].mean():5.2f}")
        print("  all " + " ".join(f"{share[i, :, d].mean():5.2f}" for d in range(8)) + f"  {share[i].mean():5.2f}")
    print(f"\nsummary, {'ConvexMpc' if convex else 'QuatMpc'}: share still up by impulse " +
          "  ".join(f"{imp:g} N s: {share[i].mean():.3f}" for i, imp in enumerate(impulses)) + f"   all: {share.mean():.3f}\n")
    by_mu = None
    if a.mu_true:
        shape = (len(impulses), len(starts), 8, len(mus), len(delays) * len(taus) * tail)
        down = (oc["down_tick"] >= 0).reshape(shape)
        cell = down.shape[1] * down.shape[2] * down.shape[4]
        print(f"true friction: robots down per (impulse, mu_true) cell, of {cell} (the controller assumes mu = {p.mu:g})")
        print("impulse " + " ".join(f"mu={m:5.2f}" for m in mus))
        for i, imp in enumerate(impulses):
            print(f"{imp:5g}   " + " ".join(f"{int(down[i, :, :, m].sum()):8d}" for m in range(len(mus))))
        print("ground tallies by mu_true, mean per robot (robots that went down stop counting at their down tick):")
        for k in ("clipped_ticks", "friction_leg_ticks", "normal_leg_ticks"):
            v = ta[k].reshape(shape)
            print(f"{k:>20s} " + " ".join(f"{v[:, :, :, m].mean():8.1f}" for m in range(len(mus))))
        first = ta["first_clipped_tick"].reshape(shape)
        print(f"{'never clipped':>20s} " + " ".join(f"{int((first[:, :, :, m] < 0).sum()):8d}" for m in range(len(mus))) + "\n")
        by_mu = {"mu_true": mus.tolist(), "down": down.sum(axis=(1, 2, 4)).tolist(), "cell": cell,
                 "clipped_ticks_mean": ta["clipped_ticks"].reshape(shape).mean(axis=(0, 1, 2, 4)).tolist()}
    by_time = None
    if timed:
        shape = (len(impulses), len(starts), 8, len(mus), len(delays), len(taus), tail)
        down = (oc["down_tick"] >= 0).reshape(shape)
        cell = down[0, :, :, :, 0, 0].size
        alphas = pkg.actuation_params(len(taus), tau=taus, dt=lp.dt)["alpha"]
        print(f"actuation: robots down per (impulse, delay, tau) cell, of {cell}; delay in ticks of {lp.dt * 1e3:g} ms, tau in ms (alpha)")
        print("impulse delay " + " ".join(f"tau={1e3 * t:4.1f} ({al:.3f})" for t, al in zip(taus, alphas)))
        for i, imp in enumerate(impulses):
            for l, d in enumerate(delays):
                print(f"{imp:5g}   {int(d):5d} " + " ".join(f"{int(down[i, :, :, :, l, t].sum()):16d}" for t in range(len(taus))))
        before = ((oc["down_tick"] >= 0) & (oc["down_tick"] <= push["start_tick"][:, 0])).reshape(shape)
        print("  ... of them down before their shove began, by delay: " +
              " ".join(f"{int(d)}: {int(before[:, :, :, :, l].sum())}" for l, d in enumerate(delays)) + "\n")
        by_time = {"delay_ticks": delays.tolist(), "tau_s": taus.tolist(), "alpha": alphas.tolist(), "cell": cell,
                   "down": down.sum(axis=(1, 2, 3, 6)).tolist()}
    by_sense = None
    if sensed:
        shape = (len(impulses), len(starts), 8, len(mus) * len(delays) * len(taus), len(gbs), len(levels), inner)
        down = (oc["down_tick"] >= 0).reshape(shape)
        cell = down[0, :, :, :, 0, 0].size
        what = ", ".join(f"{k} {r[0]:g} .. {r[1]:g}" for k, r in noises.items()) or "none"
        print(f"sensing: robots down per (impulse, gyro bias, noise level) cell, of {cell}; gyro bias in rad/s on every body axis, noise "
              f"levels 0 .. {len(levels) - 1} of: {what}")
        print("impulse gyro_bias " + " ".join(f"level {int(j):d}" for j in levels))
        for i, imp in enumerate(impulses):
            for b, g in enumerate(gbs):
                print(f"{imp:5g}   {g:9.4f} " + " ".join(f"{int(down[i, :, :, :, b, j].sum()):7d}" for j in range(len(levels))))
        before = ((oc["down_tick"] >= 0) & (oc["down_tick"] <= push["start_tick"][:, 0])).reshape(shape)
        print("  ... of them down before their shove began, by gyro bias: " +
              " ".join(f"{g:g}: {int(before[:, :, :, :, b].sum())}" for b, g in enumerate(gbs)) + "; by noise level: " +
              " ".join(f"{int(j)}: {int(before[:, :, :, :, :, j].sum())}" for j in range(len(levels))) + "\n")
        by_sense = {"gyro_bias": gbs.tolist(), "noise": {k: np.linspace(r[0], r[1], a.sense_steps).tolist() for k, r in noises.items()},
                    "cell": cell, "down": down.sum(axis=(1, 2, 3, 6)).tolist(), "measurements": int(seen["ticks"].sum())}
    by_gait = None
    if gaited:
        shape = (len(impulses), len(starts), 8, len(mus) * len(delays) * len(taus) * len(gbs) * len(levels), len(names), len(freqs), a.per_cell)
        down = (oc["down_tick"] >= 0).reshape(shape)
        cell = down[0, :, :, :, 0, 0].size
        print(f"gaits: robots down per (impulse, gait, frequency) cell, of {cell}; frequency in Hz")
        print("impulse         gait " + " ".join(f"{f:7.2f}" for f in freqs))
        for i, imp in enumerate(impulses):
            for g, n in enumerate(names):
                print(f"{imp:5g}   {n:>12s} " + " ".join(f"{int(down[i, :, :, :, g, f].sum()):7d}" for f in range(len(freqs))))
        before = ((oc["down_tick"] >= 0) & (oc["down_tick"] <= push["start_tick"][:, 0])).reshape(shape)
        print("  ... of them down before their shove began, by gait: " +
              " ".join(f"{n}: {int(before[:, :, :, :, g].sum())}" for g, n in enumerate(names)) + "\n")
        by_gait = {"gaits": names, "gait_freq": freqs.tolist(), "cell": cell, "down": down.sum(axis=(1, 2, 3, 6)).tolist(),
                   "down_before_shove": before.sum(axis=(0, 1, 2, 3, 5, 6)).tolist()}
    by_motor = None
    if motor is not None:
        ticks = np.maximum(oc["ticks"], 1.0)[:, None]      # (robots that went down stop counting at their down tick)
        share_sat = (mt["sat_ticks"].reshape(B, 4, 3) / ticks[:, :, None]).mean(axis=0)
        peak = mt["peak_tau"].reshape(B, 4, 3)
        lim = a.tau_max * np.asarray(pkg.GO1_TAU_MAX)
        print(f"motors: the Go1's limits x {a.tau_max:g} = {np.round(lim, 2).tolist()} N m (hip, thigh, calf); {int((mt['clipped_ticks'] > 0).sum())} of {B} "
              f"robots clipped, {mt['clipped_ticks'].mean():.1f} clipped ticks per robot, {int(mt['unreachable_leg_ticks'].sum())} unreachable leg-ticks")
        print("leg    share of ticks saturated (hip thigh calf)    peak torque asked, N m: median (hip thigh calf) | max (hip thigh calf)")
        for l, n in enumerate(("FL", "FR", "RL", "RR")):
            print(f"{n:4s}  " + " ".join(f"{v:7.4f}" for v in share_sat[l]) + "        " +
                  " ".join(f"{v:7.2f}" for v in np.median(peak[:, l], axis=0)) + "  | " + " ".join(f"{v:7.2f}" for v in peak[:, l].max(axis=0)))
        print()
        by_motor = {"tau_max_scale": a.tau_max, "tau_max": lim.tolist(), "robots_clipped": int((mt["clipped_ticks"] > 0).sum()),
                    "sat_share": share_sat.tolist(), "peak_tau_median": np.median(peak, axis=0).tolist(), "peak_tau_max": peak.max(axis=0).tolist()}
    return {"controller": controller, "by_motor": by_motor, "by_mu_true": by_mu, "by_actuation": by_time, "by_sensing": by_sense, "by_gait": by_gait, "impulses": impulses, "starts": starts, "directions_deg": np.degrees(angles).tolist(),
            "per_cell": members, "length_ticks": a.length, "speed": a.speed, "form": form, "share_up": share.tolist()}


if __name__ == "__main__":
    main()
