"""CPU suite: the oracle, its certificate and the host build of the lane core on every stance set (tests/stance_sets.py).

The state generators draw three stance sets (all legs, the two trot diagonals) and quaternions with w > 0, so the oracle was
pinned -- by the reference's goldens and tests/golden/kkt_fixtures.npz -- on those alone.  Here:
  * tests/golden/stance_fixtures.npz (tests/golden/make_stance_fixtures.py) holds the oracle's primal-dual points on all 15
    sets of four legs (QuatMpc N = 10 / 20, ConvexMpc N = 10 / 20), on 16 sets of the 8-point model (N = 16) and on both signs
    of quat and quat_d; they are re-evaluated WITHOUT oracle code by kkt_independent under the tolerances of
    tests/test_kkt_certificate.py, and four of them (a one-leg, two non-trot two-leg and a three-leg set) are reached by the
    independent active-set Newton solver;
  * today's oracle reproduces the stored points, is bit-for-bit indifferent to the sign of either quaternion, and converges on
    every record of the input sets (so the sets cannot drift out of the solver's envelope unnoticed);
  * the host build of quaternion-mpc_amd/csrc/qmpc_lane_core.h (the build of tests/test_lane_core_cpu.py) follows the oracle
    on all of them in both solver modes and through the warm start, under that module's rules.
The kernels are held to the same records on the GPU by tests/test_gpu_stance_sets.py."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import kkt_independent as K
import stance_sets as S
import test_kkt_certificate as KC
import test_lane_core_cpu as LC
from test_lane_core_cpu import lane  # noqa: F401  (the fixture that builds and wraps tests/native/lane_core_host.cpp)

FIX = Path(__file__).parent / "golden" / "stance_fixtures.npz"
CASES = {   # name: (records, params, model, problem class, horizon, stored instances at least)
    "quat_n10": (lambda pkg: S.quat(pkg, 10), "default_params", "quat", "QuatProblem", 10, 60),
    "quat_n20": (lambda pkg: S.quat(pkg, 20), "default_params", "quat", "QuatProblem", 20, 36),
    "convex_n10": (S.convex, "default_convex_params", "convex", "ConvexProblem", 10, 60),
    "convex_n20": (S.convex, "default_convex_params", "convex", "ConvexProblem", 20, 60),
    "biped8_n16": (S.biped8, "default_biped8_params", "biped8", "QuatProblem", 16, 32),
}
# every record set the GPU suite uses: name -> (records, oracle params, oracle call, force components)
SETS = {
    "quat_n5": (lambda pkg: S.quat(pkg, 5), "default_params", "solve", 5, 12),
    "quat_n10": (lambda pkg: S.quat(pkg, 10), "default_params", "solve", 10, 12),
    "quat_n20": (lambda pkg: S.quat(pkg, 20), "default_params", "solve", 20, 12),
    "convex_n10": (S.convex, "default_convex_params", "convex_solve", 10, 12),
    "convex_n20": (S.convex, "default_convex_params", "convex_solve", 20, 12),
    "biped8_n8": (S.biped8, "default_biped8_params", "solve8", 8, 24),
    "biped8_n16": (S.biped8, "default_biped8_params", "solve8", 16, 24),
}


@pytest.fixture(scope="module")
def fix():
    return np.load(FIX)


def test_the_input_sets_are_what_they_claim(pkg):
    assert len(S.MASKS4) == 15 and len(set(S.MASKS4)) == 15 and len(S.MASKS8) == 16 and len(set(S.MASKS8)) == 16
    assert len(S.ENVELOPE_N20) == 9 and set(S.ENVELOPE_N20) < set(S.MASKS4)
    rec, plain = S.quat(pkg, 10), S.quat(pkg, 10, flipped=False)
    assert len(rec) == 480 and len(S.quat(pkg, 20)) == 288 and len(S.convex(pkg)) == 480 and len(S.biped8(pkg)) == 256
    assert np.array_equal(rec["rot"], plain["rot"]) and (plain["quat"][:, 0] > 0).all() and (plain["quat_d"][:, 0] > 0).all()
    # both signs of quat on every set.  quat_d is negated on every third record, and 3 divides 15: the sets MASKS4[0, 3, 6, 9, 12]
    # always carry -quat_d and the other ten never do.  All four combinations on every set come from S.flip of the unflipped
    # records (test_oracle_does_not_see_the_sign_of_a_quaternion; the sign-flip runs of tests/test_gpu_stance_sets.py)
    for r in (rec, S.quat(pkg, 20)):
        seen = {(tuple(c.astype(int)), bool(q[0] < 0), bool(qd[0] < 0)) for c, q, qd in zip(r["contacts"], r["quat"], r["quat_d"])}
        assert len(seen) == 2 * len({tuple(c.astype(int)) for c in r["contacts"]})
        assert all((m, not a, b) in seen for m, a, b in seen)
        assert {b for _, _, b in seen} == {False, True}
    assert ((rec["quat_d"][:, 0] < 0) == (np.arange(480) % 15 % 3 == 0)).all()
    assert {tuple(c.astype(int)) for c in rec["contacts"]} == set(S.MASKS4)
    assert {tuple(c.astype(int)) for c in S.quat(pkg, 20)["contacts"]} == set(S.ENVELOPE_N20)
    assert {tuple(c.astype(int)) for c in S.biped8(pkg)["contacts"]} == set(S.MASKS8)
    first, second = S.warm_pairs(pkg)
    pairs = [(tuple(a.astype(int)), tuple(b.astype(int))) for a, b in zip(first["contacts"], second["contacts"])]
    assert len(pairs) == 450 and all(pairs.count((a, b)) == 2 for a in S.MASKS4 for b in S.MASKS4)
    t = S.tiled(rec, 1025)
    assert len(t) == 1440 and S.copies_identical(t, 480) and not S.copies_identical(np.arange(960.0), 480)


@pytest.mark.parametrize("name", list(CASES))
def test_stored_points_satisfy_kkt_independently(pkg, fix, name):
    """The rule of tests/test_kkt_certificate.py, its tolerances imported.  Measured, worst over the stored points: stationarity
    1.1e-13 (QuatMpc N=10), 1.1e-12 (N=20), 4.9e-14 / 6.2e-12 (ConvexMpc N=10 / 20), 1.4e-14 (8-point); with NNLS multipliers
    <= 1.0e-12; complementarity <= 1.5e-10; violation <= 5.7e-14; lam_min >= 0; 21 / 50 / 42 / 70 / 22 active rows per instance."""
    recs, dp, model, cls, N, n_min = CASES[name]
    U, LAM = fix[name + "_U"], fix[name + "_lam"]
    n = U.shape[0]
    assert n >= n_min
    rec = recs(pkg)[:n]
    par = KC._params(pkg, dp, N)
    worst, active = {}, 0
    for i in range(n):
        r = getattr(K, cls)(par, rec[i]).kkt(U[i], LAM[i])
        for k, v in r.items():
            worst[k] = min(worst.get(k, v), v) if k == "lam_min" else max(worst.get(k, v), v)
        active += int((LAM[i] > 1e-6).sum())
    print(name, {k: f"{v:.2e}" for k, v in worst.items()}, "active rows/instance", active / n)
    assert worst["stationarity"] <= KC.TOL_STATIONARITY
    assert worst["stationarity_nnls"] <= KC.TOL_STATIONARITY
    assert worst["complementarity_min"] <= KC.TOL_COMPLEMENTARITY
    assert worst["violation"] <= KC.TOL_FEASIBILITY
    assert worst["lam_min"] >= -1e-12
    assert worst["swing_force"] == 0.0
    assert active / n >= 4          # the active-constraint regime


def test_independent_solver_reaches_the_same_points(pkg, fix):
    """Active-set Newton (tests/kkt_independent.py) on a one-leg set, on the two kinds of two-leg set the trot never has and on a
    three-leg set of QuatMpc N = 10: measured 1.4e-10 N from the stored points (1.4e-12 / 1.4e-11 / 1.4e-10 / 1.5e-12)."""
    idx, Ui, U = fix["quat_n10_independent_index"], fix["quat_n10_U_independent"], fix["quat_n10_U"]
    masks = [tuple(c.astype(int)) for c in S.quat(pkg, 10)["contacts"][idx]]
    assert (0, 0, 1, 1) in masks or (1, 1, 0, 0) in masks
    assert (0, 1, 0, 1) in masks or (1, 0, 1, 0) in masks
    assert any(sum(m) == 1 for m in masks) and any(sum(m) == 3 for m in masks) and len(masks) >= 4
    d = np.abs(Ui - U[idx]).max()
    print(f"active-set Newton vs stored point on {masks}: {d:.2e} N")
    assert d <= KC.TOL_INDEPENDENT


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_reproduces_the_stored_points(pkg, oracle, fix, name):
    recs, dp, model, cls, N, _ = CASES[name]
    U = fix[name + "_U"]
    rec = recs(pkg)[:U.shape[0]]
    solve = {"quat": oracle.solve, "biped8": oracle.solve8, "convex": oracle.convex_solve}[model]
    f, info, tu, _ = solve(getattr(oracle, dp)(N, 0), rec, threads=4, want_traj=True)
    assert (info["status"] == 0).all()
    assert np.array_equal(info["iterations"], fix[name + "_iterations"])
    assert np.abs(tu - U).max() <= 1e-9


def test_oracle_does_not_see_the_sign_of_a_quaternion(pkg, oracle):
    """q and -q are one attitude, and the cost takes |q_ref' q|: forces, status and iteration words are bit-identical"""
    p = oracle.default_params(10, 0)
    rec = S.quat(pkg, 10, flipped=False)
    f, info = oracle.solve(p, rec, threads=8)
    for kw in ({"quat": True}, {"quat_d": True}, {"quat": True, "quat_d": True}):
        g, ginfo = oracle.solve(p, S.flip(rec, **kw), threads=8)
        assert g.tobytes() == f.tobytes(), kw
        assert np.array_equal(ginfo["status"], info["status"]) and np.array_equal(ginfo["iterations"], info["iterations"]), kw


@pytest.mark.parametrize("name", list(SETS))
def test_every_record_is_inside_the_solvers_envelope(pkg, oracle, name):
    """Converged mode: status 0 on every record.  Measured iterations at most: N=5 25, N=10 31, N=20 48 (QuatMpc; cap 120),
    ConvexMpc 23 / 26, 8-point 21."""
    recs, dp, call, N, _ = SETS[name]
    f, info = getattr(oracle, call)(getattr(oracle, dp)(N, 0), recs(pkg), threads=8)
    print(name, "iterations at most", int(info["iterations"].max()), "violation at most", float(info["max_violation"].max()))
    assert (info["status"] == 0).all(), np.bincount(info["status"])
    if name == "quat_n20":
        assert info["iterations"].max() <= 60          # a factor of two below the cap


@pytest.mark.parametrize("mode", [0, 1], ids=["converged", "reference"])
@pytest.mark.parametrize("name", [n for n in SETS if n != "biped8_n8"])
def test_lane_core_matches_oracle_on_every_stance_set(pkg, oracle, lane, fix, name, mode):  # noqa: F811
    """The rules of tests/test_lane_core_cpu.py.  Converged mode: status words equal and all 0, forces within 1e-6 N (8-point: corner
    forces 1e-5), iteration counts equal on >= 95 % and within one on >= 97 %, swing forces exactly 0, first-knot forces of the
    stored points within the same bound.  Reference mode: status and iteration words identical, forces within 1e-7 N.
    Measured, worst force difference: converged 2.2e-10 (quat N=5), 3.5e-10 (N=10), 1.4e-9 (N=20), 4.6e-11 / 1.6e-10 (convex N=10 /
    20), 9.6e-11 (8-point); reference 3.8e-10 (quat N=5), 2.3e-10 (N=10), 3.0e-10 (N=20), 4.3e-11 / 8.1e-11 (convex), 3.0e-10
    (8-point).  Iteration words identical except: converged quat N=20 equal on 279 of 288 (96.9 %), 8-point on 255 of 256."""
    recs, dp, call, N, nu = SETS[name]
    p = getattr(oracle, dp)(N, mode)
    rec = recs(pkg)
    f, info = lane(p, rec, nu=nu)
    fo, io = getattr(oracle, call)(p, rec, threads=8)
    d = np.abs(f - fo).max()
    di = np.abs(info["iterations"].astype(int) - io["iterations"].astype(int))
    print(f"lane core {name} mode {mode}: worst {d:.2e} N, iteration counts equal on {(di == 0).mean():.4f}, "
          f"status counts {np.bincount(info['status'], minlength=6).tolist()}")
    assert np.array_equal(info["status"], io["status"])
    assert np.abs(f[S.swing_rows(rec, nu // 3)]).max() == 0.0
    if mode == 1:
        assert np.array_equal(info["iterations"], io["iterations"])
        assert d < 1e-7
        return
    assert (info["status"] == 0).all()
    assert d < (1e-5 if nu == 24 else 1e-6)
    assert (di == 0).mean() >= 0.95 and (di <= 1).mean() >= 0.97, np.bincount(di)
    if name in CASES:
        U = fix[name + "_U"]
        assert np.abs(f[:len(U)] - U[:, 0, :]).max() < (1e-5 if nu == 24 else 1e-6)


@pytest.fixture(scope="module")
def lane_warm(pkg, lane):  # noqa: F811
    lib = C.CDLL(str(LC.LIB))          # built by the fixture `lane`
    lib.lane_host_solve_warm.restype = C.c_int

    def warm(p, rec, u_init):
        B, N = rec.shape[0], p.horizon
        f = np.zeros((B, 12)); tu = np.zeros((B, N, 12))
        info = np.zeros(B, dtype=pkg.INFO_DTYPE)
        ui = None if u_init is None else np.ascontiguousarray(u_init)
        rc = lib.lane_host_solve_warm(C.byref(p), B, np.ascontiguousarray(rec).ctypes.data_as(C.c_void_p),
                                      None if ui is None else ui.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p),
                                      info.ctypes.data_as(C.c_void_p), tu.ctypes.data_as(C.c_void_p))
        assert rc == 0, rc
        return f, info, tu
    return warm


@pytest.mark.parametrize("N,mu0", [(10, 0.0), (10, 1e-6), (5, 1e-6)])
def test_lane_core_warm_start_between_every_pair_of_stance_sets(pkg, oracle, lane_warm, N, mu0):
    """A previous solution on one set, the new contacts another -- every ordered pair of the 15 sets twice -- under the rules of
    test_lane_core_warm_start_matches_oracle: status equal and all 0, forces within 1e-6 N (measured 1.1e-9), iteration counts
    equal on >= 90 % (measured >= 99.1 %) and within one on >= 95 %; swing forces of the new set exactly 0."""
    p = oracle.default_params(N, 0)
    if mu0:
        p.ipm_mu0 = mu0
    first, second = S.warm_pairs(pkg)
    f0, i0, tu = lane_warm(p, first, None)
    fo0, io0, tuo = oracle.solve_warm(p, first, None, threads=8)
    assert np.array_equal(i0["status"], io0["status"]) and (i0["status"] == 0).all() and np.abs(f0 - fo0).max() < 1e-6
    assert np.abs(tu - tuo.reshape(tu.shape)).max() < 1e-6
    f1, i1, tu1 = lane_warm(p, second, tuo.reshape(tu.shape))
    fo1, io1, tuo1 = oracle.solve_warm(p, second, tuo, threads=8)
    di = np.abs(i1["iterations"].astype(int) - io1["iterations"].astype(int))
    print(f"N={N} mu0={mu0}: warm start between stance sets, worst {np.abs(f1 - fo1).max():.2e} N, iteration counts equal on {(di == 0).mean():.4f}")
    assert np.array_equal(i1["status"], io1["status"]) and (i1["status"] == 0).all()
    assert np.abs(f1 - fo1).max() < 1e-6
    assert (di == 0).mean() >= 0.9 and (di <= 1).mean() >= 0.95, np.bincount(di)
    assert np.abs(tu1 - tuo1.reshape(tu1.shape)).max() < 1e-5
    assert np.abs(f1[S.swing_rows(second)]).max() == 0.0
    assert np.abs(tu1[np.repeat(S.swing_rows(second)[:, None, :], N, axis=1)]).max() == 0.0
