#!/usr/bin/env python3
"""Plain solve against the per-instance-parameter solve (qmpc_solve_instances_device) on the same states, device buffers, one
handle per size.  Columns: the plain solve, the per-instance call under QMPC_INSTANCES_WAVE and / or QMPC_INSTANCES_AUTO
(--policy), each with uniform records (every instance carries the handle's values) and with random-variant records
(random_go1_variants).  The calls alternate within a repetition, each timed with device events around the call on the same stream
after warm-up; median of the repetitions.  The per-instance calls include their expansion kernel (one DevParams block per
instance) and, under AUTO, the stance sort and the hand-off.
    python tools/instance_params_bench.py [--policy wave|auto|both] [--reps 10] [--warmup 3] [--sizes 10:1024,...] [--json FILE]
--model convex: ConvexMpc's problem instead -- qmpc_convex_solve_device against qmpc_convex_solve_instances_device on
    random_go1_convex_states, records from random_go1_convex_variants; the handle opts in to the lane form
    (qmpc_set_convex_lane_records), so the AUTO column is qmpc_lane_cinst_kernel from the switch-over on and the WAVE column the
    wave form, as for QuatMpc.
--plain-lib FILE: another build of the library (e.g. the parent revision's) whose plain solve joins the alternation as
    "base_plain", with a handle of its own on the same buffers: the per-instance call over THAT plain solve, in the same job.
--schedule: the solve with a contact schedule over the horizon (qmpc_solve_schedule_device) beside qmpc_solve_instances_device in
    the same alternation, uniform records, sizes 10:1024,10:8192,20:4096 unless --sizes says otherwise: with constant schedules
    (the same problems as the per-instance call, the same bytes: the price of the per-knot predicate) and with the "trot -> four
    -> other" family of schedule_families (other problems: their time and mean iteration count)."""
import argparse
import ctypes as C
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


class BasePlain:
    """the plain device solve of another build of the library, through its C ABI alone (the build may lack newer symbols)"""

    def __init__(self, path, params, batch, convex):
        self.lib = C.CDLL(str(path))
        vp, i32 = C.c_void_p, C.c_int32
        self.lib.qmpc_create.argtypes = [vp, i32, i32, C.POINTER(vp)]
        self.lib.qmpc_create.restype = i32
        self.lib.qmpc_prepare.argtypes = [vp, i32]
        self.lib.qmpc_prepare.restype = i32
        self.lib.qmpc_destroy.argtypes = [vp]
        self.fn = self.lib.qmpc_convex_solve_device if convex else self.lib.qmpc_solve_device
        self.fn.argtypes = [vp, i32, vp, vp, vp, vp]
        self.fn.restype = i32
        self.h = vp()
        rc = self.lib.qmpc_create(C.byref(params), batch, 0, C.byref(self.h))
        assert rc == 0 and self.lib.qmpc_prepare(self.h, batch) == 0, rc

    def solve(self, batch, d_in, d_f, d_info, stream):
        rc = self.fn(self.h, batch, d_in, d_f, d_info, stream)
        assert rc == 0, rc

    def close(self):
        self.lib.qmpc_destroy(self.h)


SCHEDULE_SIZES = "10:1024,10:8192,20:4096"


def schedule_main(a, pkg, lib, torch):
    rows = []
    for item in (a.sizes if a.sizes != DEFAULT_SIZES else SCHEDULE_SIZES).split(","):
        N, B = (int(x) for x in item.split(":"))
        p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
        rec = pkg.random_go1_trot_states(B, config_id=2)
        fam = pkg.schedule_families(rec, N)
        s = pkg.Solver(p, B, device=0, lib=lib)
        s.prepare(B)
        s.prepare_instances()
        d_in = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
        d_ip = torch.from_numpy(pkg.instance_params(p, B).view(np.uint8).copy()).cuda()
        d_sc = {k: torch.from_numpy(fam[k].copy()).cuda() for k in ("constant", "trot_four_other")}
        d_f = torch.zeros((B, 12), dtype=torch.float64, device="cuda")
        d_info = {k: torch.zeros(B * pkg.INFO_DTYPE.itemsize, dtype=torch.uint8, device="cuda") for k in ("instances", "constant", "trot_four_other")}
        stream = torch.cuda.Stream()
        st = stream.cuda_stream
        torch.cuda.synchronize()
        calls = {"instances": lambda: s.solve_instances_device(B, d_in.data_ptr(), d_ip.data_ptr(), d_f.data_ptr(), d_info["instances"].data_ptr(),
                                                               stream=st)}
        for k in d_sc:
            calls[k] = (lambda k=k: s.solve_schedule_device(B, d_in.data_ptr(), d_ip.data_ptr(), d_sc[k].data_ptr(), d_f.data_ptr(),
                                                            d_info[k].data_ptr(), stream=st))
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
        row = {"N": N, "B": B, "kernel": s.kernel_for_schedule(B), "instances_kernel": s.kernel_for_instances(B)}
        s.close()
        line = f"N={N:2d} B={B:6d} [{row['kernel']}]"
        for k, v in times.items():
            info = np.frombuffer(d_info[k].cpu().numpy().tobytes(), dtype=pkg.INFO_DTYPE)
            ms = float(np.median(v))
            row[f"{k}_ms"], row[f"{k}_Msolves_s"] = ms, B / ms / 1e3
            row[f"{k}_spread"] = float((np.percentile(v, 75) - np.percentile(v, 25)) / ms)
            row[f"{k}_mean_iterations"], row[f"{k}_ok"] = float(info["iterations"].mean()), float((info["status"] == 0).mean())
            line += f"  {k} {ms:7.3f} ms {B / ms / 1e3:6.3f} M/s iters {row[f'{k}_mean_iterations']:.2f} ok {row[f'{k}_ok']:.4f}"
        row["constant_over_instances"] = row["constant_ms"] / row["instances_ms"]
        line += f"  constant/instances {row['constant_over_instances']:.3f}  mixed/instances {row['trot_four_other_ms'] / row['instances_ms']:.3f}"
        rows.append(row)
        print(line, flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default=DEFAULT_SIZES)
    ap.add_argument("--json", default=None)
    ap.add_argument("--policy", default="both", choices=("wave", "auto", "both"))
    ap.add_argument("--model", default="quat", choices=("quat", "convex"))
    ap.add_argument("--plain-lib", default=None)
    ap.add_argument("--schedule", action="store_true")
    a = ap.parse_args()
    import torch

    pkg = load_pkg()
    lib = pkg.load_library()
    if a.schedule:
        return schedule_main(a, pkg, lib, torch)
    rows = []
    for item in a.sizes.split(","):
        N, B = (int(x) for x in item.split(":"))
        convex = a.model == "convex"
        if convex:
            p = pkg.default_convex_params(N, pkg.MODE_CONVERGED, lib)
            rec = pkg.random_go1_convex_states(B, config_id=13)
        else:
            p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
            rec = pkg.random_go1_trot_states(B, config_id=2)
        s = pkg.Solver(p, B, device=0, lib=lib)
        policies = ("wave", "auto") if a.policy == "both" else (a.policy,)
        if convex:
            s.set_convex_lane_records(True)      # (takes effect under AUTO only)
        if "auto" in policies:
            s.set_instances_policy("auto")      # the buffers of every call below are allocated here, not in a timed call
        s.prepare(B)
        s.prepare_instances()
        d_in = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
        records = {"uniform": pkg.instance_params(p, B),
                   "variants": (pkg.random_go1_convex_variants if convex else pkg.random_go1_variants)(B, seed=13, base=p)}
        d_ip = {k: torch.from_numpy(v.view(np.uint8).copy()).cuda() for k, v in records.items()}
        d_f = torch.zeros((B, 12), dtype=torch.float64, device="cuda")
        d_info = torch.zeros(B * pkg.INFO_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.Stream()      # a stream of its own: the default stream's handle is 0, i.e. the solver's own stream
        st = stream.cuda_stream
        torch.cuda.synchronize()

        def inst(policy, kind):
            s.set_instances_policy(policy)
            (s.convex_solve_instances_device if convex else s.solve_instances_device)(B, d_in.data_ptr(), d_ip[kind].data_ptr(), d_f.data_ptr(),
                                                                                      d_info.data_ptr(), stream=st)

        calls = {"plain": lambda: (s.convex_solve_device if convex else s.solve_device)(B, d_in.data_ptr(), d_f.data_ptr(), d_info.data_ptr(),
                                                                                        stream=st)}
        base = BasePlain(a.plain_lib, p, B, convex) if a.plain_lib else None
        if base:
            calls["base_plain"] = lambda: base.solve(B, d_in.data_ptr(), d_f.data_ptr(), d_info.data_ptr(), st)
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
        row = {"N": N, "B": B, "model": a.model, "plain_kernel": s.kernel_for_batch(B)}
        for pol in policies:
            s.set_instances_policy(pol)
            row[f"{pol}_kernel"] = s.kernel_for_convex_instances(B) if convex else s.kernel_for_instances(B)
        s.close()
        if base:
            base.close()
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
        if "wave" in policies:
            row["wave_uniform_over_plain"] = row["wave_uniform_ms"] / row["plain_ms"]
            line += f"  [plain: {row['plain_kernel']}]  wave_uniform/plain {row['wave_uniform_over_plain']:.3f}"
            if base:
                row["wave_uniform_over_base_plain"] = row["wave_uniform_ms"] / row["base_plain_ms"]
                line += f"  wave_uniform/base_plain {row['wave_uniform_over_base_plain']:.3f}  plain/base_plain {row['plain_ms'] / row['base_plain_ms']:.3f}"
        rows.append(row)
        print(line, flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
