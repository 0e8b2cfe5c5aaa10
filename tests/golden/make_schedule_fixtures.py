#!/usr/bin/env python3
"""Writes tests/golden/schedule_fixtures.npz: certified points of QuatMpc's problem with a contact schedule over the horizon
(qmpc_solve_schedule*), found by a solver that shares nothing with the oracle or the kernels --
tests/kkt_schedule.py's active-set Newton method on the per-knot stance variables (kkt_independent's, on a torch-autograd
gradient).  The oracle has no per-knot contacts and is not involved.

  n10   the first 8 states of random_go1_trot_states(8, config_id=2), N = 10, under the four families of
        quaternion_mpc_amd.schedule_families (constant, trot -> four -> other, trot -> other, trot -> three)
  n20   the first 2 states of random_go1_trot_states(8, config_id=2), N = 20, under constant and trot -> four -> other

Stored per case: <case>_<family>_U [n][N][12], _iterations [n], _active [n] (size of the final working set), _W (the working
sets, -1 padded), and <case>_families.  About 10 s per point at N = 10, a minute at N = 20; the points are independent and run in
a process pool.    python tests/golden/make_schedule_fixtures.py"""
import os
import sys
import time
from multiprocessing import get_context
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

CASES = (("n10", 10, 8, ("constant", "trot_four_other", "trot_other", "trot_three")),
         ("n20", 20, 2, ("constant", "trot_four_other")))
STATES, CONFIG = 8, 2


def solve_point(job):
    case, N, fam, i = job
    import torch
    torch.set_num_threads(1)
    from conftest import load_pkg
    import kkt_schedule as KS
    pkg = load_pkg()
    rec = pkg.random_go1_trot_states(STATES, config_id=CONFIG)
    par = pkg.default_params(N, pkg.MODE_CONVERGED, pkg.load_library())
    sched = pkg.schedule_families(rec, N)[fam]
    prob = KS.ScheduleProblem(par, rec[i], sched[i])
    t = time.time()
    U, W, _, it = KS.active_set_newton_schedule(prob)
    r = prob.kkt(U)
    print(f"{case} {fam}[{i}]: {it} iterations, |W| = {len(W)}, stationarity_nnls {r['stationarity_nnls']:.2e}, violation "
          f"{r['violation']:.2e}, swing {r['swing_force']:.1e} ({time.time() - t:.0f} s)", flush=True)
    return case, fam, i, U, np.array(sorted(W), dtype=np.int32), it


if __name__ == "__main__":
    jobs = [(case, N, fam, i) for case, N, n, fams in CASES for fam in fams for i in range(n)]
    jobs.sort(key=lambda j: -j[1])      # the long horizons first
    with get_context("spawn").Pool(min(16, os.cpu_count() or 1)) as pool:
        res = pool.map(solve_point, jobs, chunksize=1)
    out = {}
    for case, N, n, fams in CASES:
        out[case + "_families"] = np.array(fams)
        for fam in fams:
            pts = sorted((r for r in res if r[0] == case and r[1] == fam), key=lambda r: r[2])
            assert [r[2] for r in pts] == list(range(n))
            out[f"{case}_{fam}_U"] = np.array([r[3] for r in pts])
            out[f"{case}_{fam}_iterations"] = np.array([r[5] for r in pts], dtype=np.int32)
            out[f"{case}_{fam}_active"] = np.array([r[4].size for r in pts], dtype=np.int32)
            wmax = max(r[4].size for r in pts)
            out[f"{case}_{fam}_W"] = np.array([np.pad(r[4], (0, wmax - r[4].size), constant_values=-1) for r in pts], dtype=np.int32)
    np.savez_compressed(Path(__file__).parent / "schedule_fixtures.npz", **out)
    print({k: v.shape for k, v in out.items()})
