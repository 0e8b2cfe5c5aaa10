#!/usr/bin/env python3
"""Writes tests/golden/motion_fixtures.npz: the certificate of tests/golden/make_stance_fixtures.py for body rates and speeds the
state generators never draw, with the rate fed to the problem (tests/motion_sets.py: 1 ... 12 rad/s about the body's z, x, y
and a random axis, both senses, at the generator's speed, 1 and 3 m/s; drop_ang_vel = 0).

For one record of every (speed, rate, axis, sense) cell of QuatMpc N=10 (120) and for the first 40 records -- every (rate, axis,
sense) cell at the generator's speed -- of QuatMpc N=20 and of the 8-point model at N=16 it stores the oracle's primal-dual point
(U, lambda; multipliers through the oracle-only call qo_solve_one_dual) and, for four QuatMpc N=10 records -- yaw 4 rad/s as
drawn, random axis 8 rad/s as drawn, body x 12 rad/s at 1 m/s and body y 12 rad/s at 3 m/s -- the answer of
tests/kkt_independent.py's primal active-set Newton method, which shares nothing with the oracle.
tests/test_motion_sets_cpu.py re-evaluates the stored points without oracle code and holds today's oracle and the host build of
the lane core to them; tests/test_gpu_motion_sets.py the kernels.

BUILD CONTAINER ONLY (imports the oracle; a few minutes):  python tests/golden/make_motion_fixtures.py"""
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))
from conftest import load_pkg  # noqa: E402

pkg = load_pkg()
from oracle import pyoracle as po  # noqa: E402
import kkt_independent as K  # noqa: E402
import motion_sets as M  # noqa: E402

# name, records, params, model, horizon, instances
CASES = (
    ("quat_n10", lambda: M.quat(pkg, 10), "default_params", "quat", 10, M.GRID),
    ("quat_n20", lambda: M.quat(pkg, 20), "default_params", "quat", 20, 40),
    ("biped8_n16", lambda: M.biped8(pkg, 16), "default_biped8_params", "biped8", 16, 40),
)
# records of quat(10): k = 40 (speed class) + 8 (index of the rate) + 2 (axis kind) + (sense)
INDEPENDENT = (8 * 2 + 2 * 0, 8 * 3 + 2 * 3 + 1, 40 + 8 * 4 + 2 * 1, 80 + 8 * 4 + 2 * 2 + 1)

if __name__ == "__main__":
    out = {}
    for name, recs, dp, model, N, n in CASES:
        rec = recs()[:n]
        par = M.params(po, dp, N, 0)
        U, LAM, IT = [], [], []
        for i in range(n):
            tu, _, lam, _, info = po.solve_dual(par, rec[i:i + 1], model)
            assert info["status"] == 0, (name, i)
            U.append(tu); LAM.append(lam); IT.append(info["iterations"])
        out[name + "_U"] = np.array(U)
        out[name + "_lam"] = np.array(LAM)
        out[name + "_iterations"] = np.array(IT, dtype=np.int32)
        if name == "quat_n10":
            Ui = []
            for i in INDEPENDENT:
                t = time.time()
                Ua, W, _, it = K.active_set_newton(K.QuatProblem(par, rec[i]))
                rate, kind, _, speed = M.cell(i)
                print(f"{name}[{i}] {rate} rad/s, axis {M.AXES[kind]}, speed {M.SPEEDS[speed] or 'as drawn'}: active-set Newton "
                      f"{it} iterations, |W| = {len(W)}, max|U - U_oracle| = {np.abs(Ua - U[i]).max():.2e} N ({time.time() - t:.0f} s)",
                      flush=True)
                Ui.append(Ua)
            out[name + "_U_independent"] = np.array(Ui)
            out[name + "_independent_index"] = np.array(INDEPENDENT, dtype=np.int32)
    np.savez_compressed(Path(__file__).parent / "motion_fixtures.npz", **out)
    print({k: v.shape for k, v in out.items()})
