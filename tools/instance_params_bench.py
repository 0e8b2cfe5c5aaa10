#!/usr/bin/env python3
"""Plain solve against the per-instance-parameter solve (qmpc_solve_instances_device) on the same states, device buffers, one
handle per size.  Columns: the plain solve, the per-instance call under QMPC_INSTANCES_WAVE and / or QMPC_INSTANCES_AUTO
(--policy), each with uniform records (every instance carries the handle's values) and with random-variant records
(random_go1_variants).  The calls alternate within a repetition, each timed with device events around the call on the same stream
after warm-up; median of the repetitions.  The per-instance calls include their expansion kernel (one DevParams block per
instance) and, under AUTO, the stance sort and the hand-off.
    python tools/instance_params_bench.py [--policy wave|auto|both] [--reps 10] [--warmup 3] [--sizes 10:1024,...] [--json FILE]"""
import argparse
import importlib.util
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
DEFAULT_SIZES = "10:1024,10:8192,10:32768,10:65536,20:1024,20:8192"


def load_pkg():
    spec = importlib.util.spec_from_file_location("quaternion_mpc_amd", REPO / "quaternion-mpc_amd" / "__init__.py",
                                                  submodule_search_locations=[str(REPO / "quaternion-mpc_amd")])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["quaternion_mpc_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default=DEFAULT_SIZES)
    ap.add_argument("--json", default=None)
    ap.add_argument("--policy", default="both", choices=("wave", "auto", "both"))
    a = ap.parse_args()
    import torch

    pkg = load_pkg()
    lib = pkg.load_library()
    rows = []
    for item in a.sizes.split(","):
        N, B = (int(x) for x in item.split(":"))
        p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
        rec = pkg.random_go1_trot_states(B, config_id=2)
        s = pkg.Solver(p, B, device=0, lib=lib)
        policies = ("wave", "auto") if a.policy == "both" else (a.policy,)
        if "auto" in policies:
            s.set_instances_policy("auto")      # the buffers of every call below are allocated here, not in a timed call
        s.prepare(B)
        s.prepare_instances()
        d_in = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
        records = {"uniform": pkg.instance_params(p, B), "variants": pkg.random_go1_variants(B, seed=13, base=p)}
        d_ip = {k: torch.from_numpy(v.view(np.uint8).copy()).cuda() for k, v in records.items()}
        d_f = torch.zeros((B, 12), dtype=torch.float64, device="cuda")
        d_info = torch.zeros(B * pkg.INFO_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.Stream()      # a stream of its own: the default stream's handle is 0, i.e. the solver's own stream
        st = stream.cuda_stream
        torch.cuda.synchronize()

        def inst(policy, kind):
            s.set_instances_policy(policy)
            s.solve_instances_device(B, d_in.data_ptr(), d_ip[kind].data_ptr(), d_f.data_ptr(), d_info.data_ptr(), stream=st)

        calls = {"plain": lambda: s.solve_device(B, d_in.data_ptr(), d_f.data_ptr(), d_info.data_ptr(), stream=st)}
        for pol in policies:
            for kind in records:
                calls[f"{pol}_{kind}"] = (lambda pol=pol, kind=kind: inst(pol, kind))
        times = {k: [] for k in calls}
        for r in range(a.warmup + a.reps):
            for k, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                if r >= a.warmup:
                    times[k].append(e0.elapsed_time(e1))
        row = {"N": N, "B": B, "plain_kernel": s.kernel_for_batch(B)}
        for pol in policies:
            s.set_instances_policy(pol)
            row[f"{pol}_kernel"] = s.kernel_for_instances(B)
        s.close()
        line = f"N={N:2d} B={B:6d}"
        for k, v in times.items():
            ms = float(np.median(v))
            row[f"{k}_ms"], row[f"{k}_Msolves_s"] = ms, B / ms / 1e3
            row[f"{k}_spread"] = float((np.percentile(v, 75) - np.percentile(v, 25)) / ms)
            line += f"  {k} {ms:7.3f} ms {B / ms / 1e3:6.3f} M/s"
        for pol in policies:
            line += f"  [{pol}: {row[pol + '_kernel']}]"
        if "auto" in policies and "wave" in policies:
            line += f"  auto/wave variants x{row['wave_variants_ms'] / row['auto_variants_ms']:.3f}"
        if "auto" in policies:
            line += f"  auto/plain {row['auto_variants_ms'] / row['plain_ms']:.3f}"
        rows.append(row)
        print(line, flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
