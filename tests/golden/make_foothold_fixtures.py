#!/usr/bin/env python3
"""Writes tests/golden/foothold_fixtures.npz: the certificate of tests/golden/make_motion_fixtures.py for footholds and
references the state generators never draw (tests/foothold_sets.py: ten foothold kinds from a 10 x 7 cm rectangle to feet 0.6 m
below the body, crossed with pos_ref + 0.3 m, vel_ref + 3 m/s and acc_ref + 5 m/s^2 along a random direction).

For the first 40 records -- one of every (kind, class) cell -- of QuatMpc N=10, of ConvexMpc N=10 and of the 8-point model at
N=16 (28 cells), and for the first 36 of QuatMpc N=20 (its reduced grid) it stores the oracle's primal-dual point (U, lambda;
multipliers through the oracle-only call qo_solve_one_dual) and, for four QuatMpc N=10 records -- narrow as drawn, aside with
pos_ref + 0.3 u, stretched with vel_ref + 3 u, crossed with acc_ref + 5 u -- the answer of tests/kkt_independent.py's primal
active-set Newton method, which shares nothing with the oracle.
tests/test_foothold_sets_cpu.py re-evaluates the stored points without oracle code and holds today's oracle and the host build
of the lane core to them; tests/test_gpu_foothold_sets.py the kernels.

BUILD CONTAINER ONLY (imports the oracle; a few minutes):  python tests/golden/make_foothold_fixtures.py"""
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
import foothold_sets as F  # noqa: E402
import kkt_independent as K  # noqa: E402

# name, records, params, model, horizon, instances
CASES = (
    ("quat_n10", lambda: F.quat(pkg, 10), "default_params", "quat", 10, F.GRID),
    ("quat_n20", lambda: F.quat(pkg, 20), "default_params", "quat", 20, 36),
    ("convex_n10", lambda: F.convex(pkg, 10), "default_convex_params", "convex", 10, F.GRID),
    ("biped8_n16", lambda: F.biped8(pkg, 16), "default_biped8_params", "biped8", 16, 40),
)
# records of quat(10): k = 10 (reference class) + (foothold kind)
INDEPENDENT = tuple(10 * c + F.KINDS.index(k) for c, k in enumerate(("narrow", "aside", "stretched", "crossed")))

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
                kind, cls = F.cell(i)
                print(f"{name}[{i}] {F.KINDS[kind]}, references {F.CLASSES[cls]}: active-set Newton {it} iterations, |W| = {len(W)}, "
                      f"max|U - U_oracle| = {np.abs(Ua - U[i]).max():.2e} N ({time.time() - t:.0f} s)", flush=True)
                Ui.append(Ua)
            out[name + "_U_independent"] = np.array(Ui)
            out[name + "_independent_index"] = np.array(INDEPENDENT, dtype=np.int32)
    np.savez_compressed(Path(__file__).parent / "foothold_fixtures.npz", **out)
    print({k: v.shape for k, v in out.items()})
