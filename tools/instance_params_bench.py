#!/usr/bin/env python3
"""Plain solve against the per-instance-parameter solve (qmpc_solve_instances_device) on the same records, uniform records
(every instance carries the handle's values), device buffers, one handle per size.  The two calls alternate, each timed with
device events around the call on the same stream after warm-up; median of the repetitions.  The per-instance call includes its
expansion kernel (one DevParams block per instance); run under `rocprofv3 --kernel-trace --stats` for that kernel's own time.
    python tools/instance_params_bench.py [--reps 10] [--warmup 3] [--sizes 10:1024,10:8192,...] [--json FILE]"""
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
        s.prepare(B)
        s.prepare_instances()
        d_in = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
        d_ip = torch.from_numpy(pkg.instance_params(p, B).view(np.uint8).copy()).cuda()
        d_f = torch.zeros((B, 12), dtype=torch.float64, device="cuda")
        d_info = torch.zeros(B * pkg.INFO_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.Stream()      # a stream of its own: the default stream's handle is 0, i.e. the solver's own stream
        st = stream.cuda_stream
        torch.cuda.synchronize()
        calls = {"plain": lambda: s.solve_device(B, d_in.data_ptr(), d_f.data_ptr(), d_info.data_ptr(), stream=st),
                 "instances": lambda: s.solve_instances_device(B, d_in.data_ptr(), d_ip.data_ptr(), d_f.data_ptr(), d_info.data_ptr(),
                                                               stream=st)}
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
        fam = {"plain": s.kernel_for_batch(B), "instances": s.kernel_for_instances(B)}
        s.close()
        ms = {k: float(np.median(v)) for k, v in times.items()}
        row = {"N": N, "B": B, "plain_kernel": fam["plain"], "instances_kernel": fam["instances"], "plain_ms": ms["plain"],
               "instances_ms": ms["instances"], "plain_Msolves_s": B / ms["plain"] / 1e3, "instances_Msolves_s": B / ms["instances"] / 1e3,
               "ratio": ms["instances"] / ms["plain"]}
        rows.append(row)
        print(f"N={N:2d} B={B:6d}  plain {fam['plain']:>12s} {ms['plain']:8.3f} ms {row['plain_Msolves_s']:6.3f} M/s   "
              f"instances {fam['instances']:>9s} {ms['instances']:8.3f} ms {row['instances_Msolves_s']:6.3f} M/s   "
              f"ratio {row['ratio']:.3f}", flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
