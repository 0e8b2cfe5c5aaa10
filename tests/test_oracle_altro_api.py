"""The reference solver's C++ call surface over the CPU restatement (oracle/altro_compat.hpp).

oracle/altro_compat_check.cpp poses the reference's generic solver tests through that API; the expectations are
the ones those tests state:
  TestDoubleIntegrator.cpp:129-167  unconstrained, iterations_max = 3: Success, closer to the goal than x0, not within 1e-3
  TestDoubleIntegrator.cpp:242-255  goal constraint: Success, |x_N| < 1e-4, GetIterations() == 3
  TestDoubleIntegrator.cpp:353-374  control bounds: Success, |x_N| < 1e-4, u_0 = -u_bnd to 1e-4, GetIterations() == 5
  TestPendulum.cpp:194-202          terminal goal: Success, |x_N - x_f| < 1e-4, GetIterations() <= 10
  TestDoubleIntegrator.cpp:470-491  second-order cone |u| <= 1: Success, |x_N| < 1e-4, |u_0| = 1 to 1e-2 (9 iterations upstream, 10 here)
CPU only (test infrastructure)."""
import subprocess
from pathlib import Path

import pytest

ORACLE = Path(__file__).resolve().parents[1] / "oracle"


@pytest.fixture(scope="module")
def cases():
    subprocess.run(["make", "-C", str(ORACLE), "altro_compat_check"], check=True, capture_output=True)
    out = subprocess.run([str(ORACLE / "altro_compat_check")], check=True, capture_output=True, text=True).stdout
    res = {}
    for line in out.splitlines():
        name, *kv = line.split()
        res[name] = {k: float(v) for k, v in (item.split("=") for item in kv)}
    return res


def test_double_integrator_unconstrained(cases):
    c = cases["di_unconstrained"]
    assert c["bad"] == 0 and c["initialized"] == 1 and c["status"] == 0          # every call NoError, Success
    assert c["cost0"] == 27.5                                                     # 0.5 x0'Qx0 over 11 knots
    assert c["cost"] < c["cost0"] and 1e-3 < c["dist"] < c["dist0"]


def test_double_integrator_goal_constraint(cases):
    c = cases["di_goal"]
    assert c["bad"] == 0 and c["status"] == 0 and c["dist"] < 1e-4 and c["iterations"] == 3
    assert c["feas"] < 1e-4


def test_double_integrator_control_bounds(cases):
    c = cases["di_bounds"]
    assert c["bad"] == 0 and c["status"] == 0 and c["dist"] < 1e-4 and c["iterations"] == 5
    assert abs(c["u0"] + 1.0) < 1e-4 and abs(c["u1"] + 1.0) < 1e-4
    assert c["ncon_idx"] == 10                                                    # one index per knot of [0, N)


def test_pendulum_goal_constraint(cases):
    c = cases["pendulum_goal"]
    assert c["bad"] == 0 and c["status"] == 0 and c["dist"] < 1e-4 and c["iterations"] <= 10


def test_double_integrator_second_order_cone(cases):
    """TestDoubleIntegrator.cpp:377-492: |u| <= 1 as the cone (u, 1): Success, |x_N| < 1e-4, |u_0| = 1 to 1e-2.
    The reference also asserts GetIterations() == 9; the restatement needs 10.  Where the iteration goes: this KAT (like
    the other DoubleIntegrator / Pendulum tests) leaves AltroOptions::use_backtracking_linesearch at its default, i.e.
    it runs the fork's OTHER line search (interpolating), and it is the only KAT in which steps shorter than 1 are
    taken (alpha = 0.5 twice at penalty 100 in the restatement's trace); every caller on the path sets
    use_backtracking_linesearch = true (QuatMpc.cpp:23, ConvexMpc.cpp:38, TestBicycle.cpp:154, the golden generators),
    which is the search restated here.  The KATs that only ever take full steps reproduce exactly (3 and 5)."""
    c = cases["di_soc"]
    assert c["bad"] == 0 and c["status"] == 0 and c["dist"] < 1e-4 and abs(c["unorm"] - 1.0) < 1e-2
    assert c["feas"] < 1e-4 and 9 <= c["iterations"] <= 10


def test_recalled_interpolating_line_search_is_recorded_not_pinned(cases):
    """Round 5 (the round-4 review's item 8: close the row or bound it).  Upstream's DEFAULT line search -- bracketing + cubic
    interpolation on the merit and its slope, strong Wolfe conditions (c1 = 1e-4, c2 = 0.9) -- restated as recalled behind
    use_backtracking_linesearch = false (oracle/qo_altro.c: linesearch_cubic; the slope through expansions at the candidate
    and the d(x,u)/d(alpha) recursion).  What it does to the generic known-answer tests: the ones that only take full steps
    reproduce as before (3 and 5 iterations: a full Newton step of an LQ problem has slope 0); the second-order-cone KAT takes
    alpha = 0.446 and 0.531 where backtracking takes 0.5 twice and STILL needs 10 iterations (upstream asserts 9,
    TestDoubleIntegrator.cpp:489-491); the goal-constrained pendulum needs 13 where backtracking needs 9.  So the missing
    iteration is not explained by the search as recalled, the fork itself is not in the tree (CMakeLists.txt:34-40), and
    SURVEY 8f rank 4 stays 'partial, unpinnable'.  The path is unaffected: every caller on it selects backtracking."""
    assert cases["di_goal_cubic"]["iterations"] == 3 and cases["di_goal_cubic"]["status"] == 0
    assert cases["di_bounds_cubic"]["iterations"] == 5 and abs(cases["di_bounds_cubic"]["u0"] + 1.0) < 1e-4
    c = cases["di_soc_cubic"]
    assert c["bad"] == 0 and c["status"] == 0 and c["dist"] < 1e-4 and abs(c["unorm"] - 1.0) < 1e-2 and c["feas"] < 1e-4
    assert c["iterations"] == 10                       # recorded: not upstream's 9
    p = cases["pendulum_goal_cubic"]
    assert p["status"] == 0 and p["dist"] < 1e-4 and p["iterations"] == 13       # recorded: backtracking needs 9


def test_error_codes(cases):
    c = cases["api_errors"]
    # DimensionUnknown, SolverNotInitialized, DimensionMismatch, BadIndex, NotSupported (cone with > 8 rows), DimensionUnknown
    assert [c[k] for k in ("e1", "e2", "e3", "e4", "e5", "e6")] == [1, 4, 3, 2, 7, 1]
    assert c["unsolved"] == 1                                                     # Solve() before Initialize()


def test_quatmpc_call_pattern_reproduces_the_golden_forces(cases):
    """QuatMpc.cpp:179-265 written against the API (quaternion cost per knot, 24-row INEQUALITY block, error-state
    Jacobians, X = x_ref / U = u_ref guess) on the stand-pose problem of TestAltroQuatMpc.cpp: u_0 against the
    reference's own output (tests/golden/quat_mpc_test.json, input_trajectory[0])."""
    import json

    import numpy as np

    gold = np.array(json.loads((ORACLE.parent / "tests" / "golden" / "quat_mpc_test.json").read_text())["input_trajectory"][0])
    for name, tol in (("quatmpc_stand", 5e-4), ("quatmpc_stand_tight", 1e-5)):
        c = cases[name]
        u0 = np.array([c[f"u{j}"] for j in range(12)])
        assert c["bad"] == 0 and c["status"] == 0 and c["feas"] == 0.0
        assert np.abs(u0 - gold).max() < tol, (name, np.abs(u0 - gold).max())
    assert cases["quatmpc_stand"]["iterations"] <= 10          # opts.iterations_max of QuatMpc.cpp:22


def test_bicycle_mpc_loop_against_the_references_closed_loop_golden():
    """TestBicycle.cpp:25-200 through the compat API -- SetLQRCost per knot, a state inequality on every knot, then 200
    closed-loop MPC steps of Solve / GetInput / UpdateLinearCosts x31 / SetInitialState / ShiftTrajectory -- against
    the two data files the reference commits for that program: scotty.json (reference trajectory) and scotty_mpc.json
    (its OUTPUT: closed-loop states, inputs, solver iterations and tracking error per step); byte-identical copies sit
    in tests/golden/.  Pins: (i) bicycle model + midpoint rule + float h = 0.1f (the golden's states reproduce from
    its inputs to 3e-17); (ii) the restated AL-iLQR scheme in a warm-started receding-horizon loop: closed-loop states
    within 2e-3 m / rad of the reference's over 200 steps, the iteration profile (1 ... 15 per solve) within a few
    iterations everywhere and exact on half of the steps.  Multipliers and penalty are re-initialised by every
    Solve(): carrying them over (tried: SetWarmStart) moves the loop far from the golden."""
    import hashlib

    golden = Path(__file__).parent / "golden"
    # the fixtures are the reference's own data files, untouched: SHA-256 of legged_ctrl/src/test/test_altro/<name>
    for name, sha in (("scotty.json", "66246041e9f77a1d376fdb0a3ea16ae5861a9a6595cc5722d37bd068a15e05da"),
                      ("scotty_mpc.json", "3849a1571528af5e9700572b80f5c9b0be2566d49155ebe5fec7b875c20269ed")):
        assert hashlib.sha256((golden / name).read_bytes()).hexdigest() == sha, name
    subprocess.run(["make", "-C", str(ORACLE), "altro_compat_check"], check=True, capture_output=True)
    out = subprocess.run([str(ORACLE / "altro_compat_check"), str(golden)], check=True, capture_output=True, text=True).stdout
    name, *kv = out.split()
    c = {k: float(v) for k, v in (item.split("=") for item in kv)}
    print(out)
    assert name == "bicycle_mpc" and c["bad"] == 0
    assert c["pin"] < 1e-12
    assert c["xdiff"] < 2e-3 and c["udiff"] < 2e-2 and c["terr_diff"] < 2e-3
    assert c["iters_match"] >= 100 and c["iters_maxdiff"] <= 4
    assert abs(c["iters_sum"] - c["golden_iters_sum"]) <= 0.1 * c["golden_iters_sum"]
