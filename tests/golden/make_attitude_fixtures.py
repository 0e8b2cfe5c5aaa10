#!/usr/bin/env python3
"""Writes tests/golden/attitude_fixtures.npz: the certificate of tests/golden/make_stance_fixtures.py for attitude errors the
state generators never draw (tests/attitude_sets.py: quat_d up to 3.5 rad from quat about the body's z, x, y and a random axis,
both senses).

For one record of every (angle, axis, sense) cell of QuatMpc N=10 (64), N=20 (24) and of the 8-point model at N=16 (24 up to
1.5 rad and 8 at 2.0 rad) it stores the oracle's primal-dual point (U, lambda; multipliers through the oracle-only call
qo_solve_one_dual) and, for four QuatMpc N=10 records -- yaw 2.0 rad, random axis 3.0 rad, body x 3.1 rad and yaw 3.5 rad --
the answer of tests/kkt_independent.py's primal active-set Newton method, which shares nothing with the oracle.
tests/test_attitude_sets_cpu.py re-evaluates the stored points without oracle code and holds today's oracle and the host build
of the lane core to them; tests/test_gpu_attitude_sets.py the kernels.

BUILD CONTAINER ONLY (imports the oracle; a few minutes):  python tests/golden/make_attitude_fixtures.py"""
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
import attitude_sets as A  # noqa: E402
import kkt_independent as K  # noqa: E402

# name, records, params, model, horizon, instances: the first 8 x (angles of the set) records are one of every cell
CASES = (
    ("quat_n10", lambda: A.quat(pkg, 10), "default_params", "quat", 10, 64),
    ("quat_n20", lambda: A.quat(pkg, 20), "default_params", "quat", 20, 24),
    ("biped8_n16", lambda: A.biped8(pkg, 16), "default_biped8_params", "biped8", 16, 24),
    ("biped8_n16_far", lambda: A.biped8(pkg, 16, far=True), "default_biped8_params", "biped8", 16, 8),
)
# records of quat(10): k = 8 (index of the angle) + 2 (axis kind) + (sense)
INDEPENDENT = (8 * 3 + 2 * 0, 8 * 5 + 2 * 3, 8 * 6 + 2 * 1, 8 * 7 + 2 * 0)     # yaw 2.0, random 3.0, body x 3.1, yaw 3.5 rad

if __name__ == "__main__":
    out = {}
    for name, recs, dp, model, N, n in CASES:
        rec = recs()[:n]
        par = getattr(po, dp)(N, 0)
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
                print(f"{name}[{i}] error angle {A.error_angle(rec[i:i + 1])[0]:.2f} rad, axis {A.AXES[A.cell(i)[1]]}: active-set Newton "
                      f"{it} iterations, |W| = {len(W)}, max|U - U_oracle| = {np.abs(Ua - U[i]).max():.2e} N ({time.time() - t:.0f} s)",
                      flush=True)
                Ui.append(Ua)
            out[name + "_U_independent"] = np.array(Ui)
            out[name + "_independent_index"] = np.array(INDEPENDENT, dtype=np.int32)
    np.savez_compressed(Path(__file__).parent / "attitude_fixtures.npz", **out)
    print({k: v.shape for k, v in out.items()})
