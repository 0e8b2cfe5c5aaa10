#!/usr/bin/env python3
"""Robot-ticks per second of the device closed loop: the plain loop (qmpc_loop_run_device), plant records only and controller +
plant records (qmpc_loop_run_instances_device), uniform records (every robot carries the handle's values), cold start, robots
walking with different commands, device buffers, one handle per size.  The three calls alternate on the same states (copied
back before each call), each timed with device events around the call after warm-up; median of the repetitions.  The
per-robot calls include their expansion kernels.
    python tools/loop_instances_bench.py [--reps 5] [--warmup 1] [--ticks 50] [--sizes 10:1024,10:4096,10:65536] [--json FILE]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--sizes", default=DEFAULT_SIZES)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch

    pkg = load_pkg()
    lib = pkg.load_library()
    rows = []
    for item in a.sizes.split(","):
        N, B = (int(x) for x in item.split(":"))
        p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
        lp = pkg.default_loop_params(lib)
        rng = np.random.default_rng(5)
        cmds = np.zeros((B, 7))
        cmds[:, 0] = rng.uniform(-0.4, 0.4, B); cmds[:, 1] = rng.uniform(-0.15, 0.15, B)
        cmds[:, 2] = rng.uniform(0.26, 0.32, B); cmds[:, 5] = rng.uniform(-0.4, 0.4, B)
        cmds[:, 6] = (rng.random(B) < 0.85).astype(float)
        stand = cmds.copy(); stand[:, 6] = 0.0
        st = pkg.loop_states(stand, lp, height=0.3, yaw=rng.uniform(-3, 3, B), lib=lib)
        s = pkg.Solver(p, B, device=0, lib=lib)
        s.prepare(B)
        s.prepare_instances()
        st = s.loop_run(st, 6, lp)
        st["movement_mode"] = cmds[:, 6]
        d_st0 = torch.from_numpy(st.view(np.uint8).copy()).cuda()
        d_st = d_st0.clone()
        d_ctrl = torch.from_numpy(pkg.instance_params(p, B).view(np.uint8).copy()).cuda()
        d_plant = torch.from_numpy(pkg.plant_params(p, B).view(np.uint8).copy()).cuda()
        stream = torch.cuda.Stream()
        sp = stream.cuda_stream
        torch.cuda.synchronize()
        T = a.ticks
        calls = {"plain": lambda: s.loop_run_device(B, d_st.data_ptr(), T, lp, stream=sp),
                 "plant": lambda: s.loop_run_instances_device(B, d_st.data_ptr(), T, lp, d_plant=d_plant.data_ptr(), stream=sp),
                 "ctrl_plant": lambda: s.loop_run_instances_device(B, d_st.data_ptr(), T, lp, d_ctrl=d_ctrl.data_ptr(),
                                                                   d_plant=d_plant.data_ptr(), stream=sp)}
        times = {k: [] for k in calls}
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
        forms = {"plain": None, "plant": s.loop_instances_plan(B, False, False), "ctrl_plant": s.loop_instances_plan(B, True, False)}
        s.close()
        ms = {k: float(np.median(v)) for k, v in times.items()}
        row = {"N": N, "B": B, "ticks": T}
        for k in calls:
            row[k + "_ms"] = ms[k]
            row[k + "_Mrobot_ticks_s"] = B * T / ms[k] / 1e3
            row[k + "_form"] = forms[k]
        row["plant_ratio"] = row["plant_Mrobot_ticks_s"] / row["plain_Mrobot_ticks_s"]
        row["ctrl_plant_ratio"] = row["ctrl_plant_Mrobot_ticks_s"] / row["plain_Mrobot_ticks_s"]
        rows.append(row)
        print(f"N={N:2d} B={B:6d}  plain {row['plain_Mrobot_ticks_s']:7.3f} M/s   plant {row['plant_Mrobot_ticks_s']:7.3f} M/s "
              f"({row['plant_ratio']:.3f}, {forms['plant']})   ctrl+plant {row['ctrl_plant_Mrobot_ticks_s']:7.3f} M/s "
              f"({row['ctrl_plant_ratio']:.3f}, {forms['ctrl_plant']})", flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
