#!/usr/bin/env python3
"""Switch-over between the wave-per-instance kernels and the lane kernel (+ hand-off) in converged mode: the library's own
choice with QMPC_LANE_MIN huge (wave side) and 1 (lane side), same records, kernel-side time between the handle's events.
GPU box:  python tools/lane_switch_scan.py [--cases N:B,...]
--instances: the same for qmpc_solve_instances_device with random-variant records -- QMPC_INSTANCES_WAVE against
QMPC_INSTANCES_AUTO with QMPC_LANE_INST_MIN=1 on one handle per horizon, batches 8192 ... 65536 in steps of 2048 at N=10 and N=20
(the switch-over lane_min_inst of qmpc_plan_fill.h is the smallest size from which the lane path wins at every larger one).
--loop-instances: the same for the ticks of qmpc_loop_run_instances_device with random-variant controller and plant records -- WAVE
against AUTO with QMPC_LANE_INST_MIN=1 and QMPC_LANE_MIN=1 on one handle per horizon, robots walking with different commands,
--ticks ticks per call timed with device events (the switch-over of plan_loop_instances under QMPC_INSTANCES_AUTO, qmpc_plan.h).
--model convex (with --instances or --loop-instances): ConvexMpc's calls on a handle that opted in to the lane form
(qmpc_set_convex_lane_records; for the loops also qmpc_set_convex_records), QMPC_LANE_CINST_MIN=1 in place of QMPC_LANE_INST_MIN:
the switch-over lane_min_cinst of qmpc_plan_fill.h.
--warm (with --loop-instances): the warm-started ticks (lp.warm_start = 1, ipm_mu0 = 1e-6) on a handle that opted in -- QuatMpc:
qmpc_set_loop_warm_records, ConvexMpc: qmpc_set_convex_warm_records -- the warm switch-over of plan_loop_instances."""
import argparse, os, sys
from pathlib import Path
import numpy as np
REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
import __graft_entry__ as g  # noqa: E402
ap = argparse.ArgumentParser()
ap.add_argument("--cases", default="10:12288,10:16384,10:20480,10:24576,16:12288,16:16384,16:20480,20:12288,20:16384,20:20480,24:12288,24:16384")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--instances", action="store_true")
ap.add_argument("--loop-instances", action="store_true")
ap.add_argument("--ticks", type=int, default=20)
ap.add_argument("--step", type=int, default=2048)
ap.add_argument("--horizons", default="10,20")
ap.add_argument("--model", default="quat", choices=("quat", "convex"))
ap.add_argument("--start", type=int, default=8192)
ap.add_argument("--warm", action="store_true")
a = ap.parse_args()
pkg = g._load_pkg(); lib = pkg.load_library()
convex = a.model == "convex"
default_params = pkg.default_convex_params if convex else pkg.default_params
variants = pkg.random_go1_convex_variants if convex else pkg.random_go1_variants
def opt_in(s):      # noqa: E302
    if convex:
        s.set_convex_records(True); s.set_convex_lane_records(True); s.set_convex_warm_records(a.warm)
    elif a.warm:
        s.set_loop_warm_records(True)
import torch  # noqa: E402
if a.loop_instances:
    os.environ["QMPC_LANE_CINST_MIN" if convex else "QMPC_LANE_INST_MIN"] = "1"
    os.environ["QMPC_LANE_MIN"] = "1"      # (the tick's switch-over is the larger of the two)
    BMAX, T = 65536, a.ticks
    for N in (int(x) for x in a.horizons.split(",")):
        p = default_params(N, 0, lib)
        lp = pkg.default_loop_params(lib)
        if a.warm:
            p.ipm_mu0 = 1e-6
            lp.warm_start = 1.0
        rng = np.random.default_rng(5)
        cmds = np.zeros((BMAX, 7))
        cmds[:, 0] = rng.uniform(-0.4, 0.4, BMAX); cmds[:, 1] = rng.uniform(-0.15, 0.15, BMAX)
        cmds[:, 2] = rng.uniform(0.26, 0.32, BMAX); cmds[:, 5] = rng.uniform(-0.4, 0.4, BMAX)
        cmds[:, 6] = (rng.random(BMAX) < 0.85).astype(float)
        if convex:      # (this controller has no command for a robot that stands)
            cmds[cmds[:, 6] == 0, :2] = 0.0; cmds[cmds[:, 6] == 0, 5] = 0.0
        stand = cmds.copy(); stand[:, 6] = 0.0
        st = pkg.loop_states(stand, lp, height=0.3, yaw=rng.uniform(-3, 3, BMAX), lib=lib)
        ctrl = variants(BMAX, seed=13, base=p); ctrl["mu"] = np.maximum(ctrl["mu"], 0.5)
        plant = pkg.random_go1_plants(BMAX, seed=11, base=p, payload=(-1.0, 3.0), force=(0.0, 10.0))
        s = pkg.Solver(p, BMAX, 0, lib)
        opt_in(s)
        s.set_instances_policy("auto"); s.prepare(BMAX); s.prepare_instances()
        st = s.loop_run_instances(st, 6, lp, ctrl=ctrl, plant=plant)
        st["movement_mode"] = cmds[:, 6]
        st = s.loop_run_instances(st, 10, lp, ctrl=ctrl, plant=plant)      # in gait
        dev = lambda x: torch.from_numpy(x.view(np.uint8).copy()).cuda()  # noqa: E731
        d_st0, d_ctrl, d_plant = dev(st), dev(ctrl), dev(plant)
        d_st = d_st0.clone()
        stream = torch.cuda.Stream(); torch.cuda.synchronize()
        first, wins = None, []
        for B in range(a.start, BMAX + 1, a.step):
            ms = {"wave": [], "auto": []}
            for r in range(a.reps + 1):
                for pol in ms:
                    s.set_instances_policy(pol)
                    with torch.cuda.stream(stream):
                        d_st.copy_(d_st0)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    s.loop_run_instances_device(B, d_st.data_ptr(), T, lp, d_ctrl=d_ctrl.data_ptr(), d_plant=d_plant.data_ptr(), stream=stream.cuda_stream)
                    e1.record(stream); e1.synchronize()
                    if r >= 1: ms[pol].append(e0.elapsed_time(e1))
            form = {}
            for pol in ms:
                s.set_instances_policy(pol); form[pol] = s.loop_instances_plan(B, True, a.warm)[1]
            mw, ml = float(np.median(ms["wave"])), float(np.median(ms["auto"]))
            wins.append((B, ml < mw))
            print(f"N={N} B={B}: wave {form['wave']} {mw:.3f} ms ({B * T / mw / 1e3:.3f} M robot-ticks/s) vs auto {form['auto']} {ml:.3f} ms "
                  f"({B * T / ml / 1e3:.3f} M)  auto/wave x{mw / ml:.3f}", flush=True)
        s.close()
        for B, w in reversed(wins):
            if not w: break
            first = B
        print(f"N={N}{' warm' if a.warm else ''}: the lane ticks are faster at every scanned size from {first} on", flush=True)
    sys.exit(0)
if a.instances:
    os.environ["QMPC_LANE_CINST_MIN" if convex else "QMPC_LANE_INST_MIN"] = "1"
    BMAX = 65536
    for N in (int(x) for x in a.horizons.split(",")):
        p = default_params(N, 0, lib)
        rec = pkg.random_go1_convex_states(BMAX, config_id=13) if convex else pkg.random_go1_trot_states(BMAX, config_id=3 if N == 20 else 2)
        ip = variants(BMAX, seed=13, base=p)
        d_in = torch.from_numpy(rec.view(np.uint8).copy()).cuda(); d_ip = torch.from_numpy(ip.view(np.uint8).copy()).cuda()
        d_f = torch.zeros(BMAX, 12, dtype=torch.float64, device="cuda"); d_i = torch.zeros(BMAX, 5, dtype=torch.float64, device="cuda")
        s = pkg.Solver(p, BMAX, 0, lib)
        opt_in(s)
        s.set_instances_policy("auto"); s.prepare(BMAX); s.prepare_instances()
        solve_dev = s.convex_solve_instances_device if convex else s.solve_instances_device
        kernel_for = s.kernel_for_convex_instances if convex else s.kernel_for_instances
        first = None
        wins = []
        for B in range(a.start, BMAX + 1, a.step):
            ms = {"wave": [], "auto": []}
            for r in range(a.reps + 2):
                for pol in ms:
                    s.set_instances_policy(pol)
                    solve_dev(B, d_in.data_ptr(), d_ip.data_ptr(), d_f.data_ptr(), d_i.data_ptr()); s.wait()
                    if r >= 2: ms[pol].append(s.last_kernel_ms())
            kern = {}
            for pol in ms:
                s.set_instances_policy(pol); kern[pol] = kernel_for(B)
            mw, ml = float(np.median(ms["wave"])), float(np.median(ms["auto"]))
            wins.append((B, ml < mw))
            print(f"N={N} B={B}: wave {kern['wave']} {mw:.3f} ms ({B / mw / 1e3:.3f} M/s) vs auto {kern['auto']} {ml:.3f} ms ({B / ml / 1e3:.3f} M/s)  "
                  f"auto/wave x{mw / ml:.3f}", flush=True)
        s.close()
        for B, w in reversed(wins):
            if not w: break
            first = B
        print(f"N={N}: the lane path is faster at every scanned size from {first} on", flush=True)
    sys.exit(0)
for case in a.cases.split(","):
    N, B = (int(x) for x in case.split(":"))
    p = pkg.default_params(N, 0, lib)
    rec = pkg.random_go1_trot_states(B, config_id=3 if N == 20 else 4)
    d_in = torch.from_numpy(rec.view(np.float64).reshape(B, -1).copy()).cuda()
    out = {}
    for tag, lm in (("wave", str(1 << 30)), ("lane", "1")):
        os.environ["QMPC_LANE_MIN"] = lm
        s = pkg.Solver(p, B, 0, lib)
        d_f = torch.zeros(B, 12, dtype=torch.float64, device="cuda"); d_i = torch.zeros(B, 5, dtype=torch.float64, device="cuda")
        ms = []
        for r in range(a.reps):
            s.solve_device(B, d_in.data_ptr(), d_f.data_ptr(), d_i.data_ptr()); s.wait()
            if r >= 2: ms.append(s.last_kernel_ms())
        out[tag] = (float(np.median(ms)), d_f.cpu().numpy(), s.kernel_for_batch(B))
        s.close()
    os.environ.pop("QMPC_LANE_MIN", None)
    (mw, fw, kw), (ml, fl, kl) = out["wave"], out["lane"]
    print(f"N={N} B={B}: {kw} {mw:.3f} ms ({B / mw / 1e3:.3f} M/s) vs {kl} {ml:.3f} ms ({B / ml / 1e3:.3f} M/s); max |df| {np.abs(fw - fl).max():.1e} N", flush=True)
