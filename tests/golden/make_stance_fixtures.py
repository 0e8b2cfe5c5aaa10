#!/usr/bin/env python3
"""Writes tests/golden/stance_fixtures.npz: the certificate of tests/golden/make_kkt_fixtures.py for the stance sets the state
generators never draw (tests/stance_sets.py: all 15 sets of four legs, 16 of the 8-point model, both quaternion signs).

For the first records of each input set it stores the oracle's primal-dual point (U, lambda; multipliers through the
oracle-only call qo_solve_one_dual) and, for four QuatMpc N=10 records -- a one-leg set (0001), the two kinds of two-leg set
the trot never has (0011, 0101) and a three-leg set (0111) -- the answer of tests/kkt_independent.py's primal active-set
Newton method, which shares nothing with the oracle.  tests/test_stance_sets_cpu.py re-evaluates the stored points without
oracle code and holds today's oracle and the host build of the lane core to them; tests/test_gpu_stance_sets.py the kernels.

BUILD CONTAINER ONLY (imports the oracle; a few minutes):  python tests/golden/make_stance_fixtures.py"""
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
import stance_sets as S  # noqa: E402

# name, records, params, model, horizon, instances
CASES = (
    ("quat_n10", lambda: S.quat(pkg, 10), "default_params", "quat", 10, 60),
    ("quat_n20", lambda: S.quat(pkg, 20), "default_params", "quat", 20, 36),
    ("convex_n10", lambda: S.convex(pkg), "default_convex_params", "convex", 10, 60),
    ("convex_n20", lambda: S.convex(pkg), "default_convex_params", "convex", 20, 60),
    ("biped8_n16", lambda: S.biped8(pkg), "default_biped8_params", "biped8", 16, 32),
)
INDEPENDENT = (0, 2, 4, 6)      # records of quat(10) on MASKS4[0, 2, 4, 6] = 0001, 0011, 0101, 0111

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
                print(f"{name}[{i}] contacts {rec['contacts'][i].astype(int).tolist()} active-set Newton: {it} iterations, "
                      f"|W| = {len(W)}, max|U - U_oracle| = {np.abs(Ua - U[i]).max():.2e} N ({time.time() - t:.0f} s)", flush=True)
                Ui.append(Ua)
            out[name + "_U_independent"] = np.array(Ui)
            out[name + "_independent_index"] = np.array(INDEPENDENT, dtype=np.int32)
    np.savez_compressed(Path(__file__).parent / "stance_fixtures.npz", **out)
    print({k: v.shape for k, v in out.items()})
