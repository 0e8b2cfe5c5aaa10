"""GPU suite (-m gpu): the one-wave rollouts load the next knot's operands into the registers the knot has just freed.

rollout_closed_w<..., LN> (qmpc_wform.h) keeps one RollLoadsL and one gain row; once the gain row's sum of knot k exists they
are dead, and the operands of knot min(k + 1, N - 1) are loaded into the same registers, unconditionally: the clamp stands in
for a branch, and the last knot reloads its own operands, which nothing reads.  What can go wrong is the index (an operand of
the wrong knot, or one past the horizon) and the order (a register overwritten before its last use), and both show in the
states of the knots behind the first reload.  The workspace forms keep a set of operands per knot, loaded at the knot's head,
so on the device they are an independent reference for X_{k+1}: their forces, status words, iteration words and -- with
want_traj -- the state and input trajectories of EVERY knot must be the all-LDS form's BYTES.
  QuatMpc, N = 1, 2, 3, 10, 11   the clamp reloads the only knot; exactly one real reload; the first reload behind a
                                 reload; bench.py's kernel; a horizon past it (a second trip of the lane loops) -- record k
                                 on stance set k mod 15 of stance_sets.MASKS4
  8-point model, N = 1, 2, 8     the same body with 24 inputs (k mod 16 of MASKS8)
  ConvexMpc, N = 1, 10           its rollouts keep their text: the control
  attitude sets, N = 10          records 6 k of attitude_sets.quat (0.5 ... 3.5 rad)
  motion sets, N = 10            records 45 k mod 360 + k // 8 of motion_sets.quat (up to 12 rad/s)
  far footholds, N = 10          the 64 `ahead` / `aside` records of foothold_sets.quat: 13 to 36 oracle iterations, 21 on
                                 average, steps are shortened in most of them, so rollout_scaled_w runs as well
  warm start, N = 10             a cold solve on one stance set, then a warm-started one on another (stance_sets.warm_pairs)
64 records per case, every one of which the CPU oracle ends with status 0.  Rules, those of tests/test_gpu_wave_lane_rollout.py
whose helpers this module takes: status words equal to the oracle's and all 0; forces within 1e-6 N (8-point model: corner
forces 1e-5, foot wrench 1e-7); swing forces exactly 0; iteration words equal to the oracle's on EVERY record; the workspace
form on the tiled records the all-LDS form's bytes.  No case is left out."""
import numpy as np
import pytest

import foothold_sets as F
import stance_sets as S
import motion_sets as M
from test_gpu_stance_sets import _first_batch_beyond, _handle, _same
from test_gpu_wave_lane_rollout import _both_forms_traj, attitude_records, motion_records
from test_gpu_wave_straightline_steps import CAP, MODELS, NREC, _rules

pytestmark = pytest.mark.gpu

CASES = [("quat", 1), ("quat", 2), ("quat", 3), ("quat", 10), ("quat", 11), ("biped8", 1), ("biped8", 2), ("biped8", 8),
         ("convex", 1), ("convex", 10)]


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


@pytest.mark.parametrize("model,N", CASES, ids=[f"{m}-N{N}" for m, N in CASES])
def test_every_model_on_every_stance_set(pkg, lib, oracle, model, N):
    gen, config, params, call, masks, nl = MODELS[model]
    rec = getattr(pkg, gen)(NREC, config_id=config)
    rec["contacts"] = np.array(masks, dtype=np.float64)[np.arange(NREC) % len(masks)]
    assert len(set(map(tuple, rec["contacts"].tolist()))) == len(masks)
    fo, io = getattr(oracle, call)(getattr(oracle, params)(N, 0), rec, threads=8)
    tag = f"operands, {model} N={N}"
    f, info = _both_forms_traj(pkg, lib, getattr(pkg, params)(N, pkg.MODE_CONVERGED, lib), rec, call, tag)
    _rules(tag + ", all LDS", nl, rec, f, info, fo, io)


def test_attitude_errors_up_to_and_beyond_pi(pkg, lib, oracle):
    rec = attitude_records(pkg)
    fo, io = oracle.solve(oracle.default_params(10, 0), rec, threads=8)
    f, info = _both_forms_traj(pkg, lib, pkg.default_params(10, pkg.MODE_CONVERGED, lib), rec, "solve", "operands, quat N=10, attitude sets")
    _rules("operands, quat N=10, attitude sets, all LDS", 4, rec, f, info, fo, io)


def test_body_rates_up_to_12_rad_per_s(pkg, lib, oracle):
    rec = motion_records(pkg)
    fo, io = oracle.solve(M.params(oracle, "default_params", 10, 0), rec, threads=8)
    f, info = _both_forms_traj(pkg, lib, M.params(pkg, "default_params", 10, pkg.MODE_CONVERGED, lib), rec, "solve", "operands, quat N=10, motion sets")
    _rules("operands, quat N=10, motion sets, all LDS", 4, rec, f, info, fo, io)


def test_footholds_far_from_nominal_shorten_steps(pkg, lib, oracle):
    N = 10
    far = np.isin(F.cells("quat", N)[0], [F.KINDS.index("ahead"), F.KINDS.index("aside")])
    rec = F.quat(pkg, N)[far]
    assert len(rec) == NREC
    fo, io = oracle.solve(oracle.default_params(N, 0), rec, threads=8)
    print(f"operands | far footholds | oracle iterations {int(io['iterations'].min())} .. {int(io['iterations'].max())}, "
          f"mean {float(io['iterations'].mean()):.1f}")
    f, info = _both_forms_traj(pkg, lib, pkg.default_params(N, pkg.MODE_CONVERGED, lib), rec, "solve", "operands, quat N=10, far from nominal")
    _rules("operands, quat N=10, far from nominal, all LDS", 4, rec, f, info, fo, io)


def test_warm_started_second_solve_on_another_stance_set(pkg, lib, oracle):
    N = 10
    first, second = S.warm_pairs(pkg)
    pick = (5 * np.arange(NREC) + 3) % len(first)
    first, second = first[pick], second[pick]
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    p.ipm_mu0 = 1e-6
    with _handle(pkg, lib, p, CAP) as s:
        assert s.kernel_for_batch(NREC) == "wform_lds"
        f0, i0, tu0 = s.solve_warm(first, None)
        f1, i1, tu1 = s.solve_warm(second, tu0)
        b1 = _first_batch_beyond(s, "wform_lds", CAP)
        t0, t1 = S.tiled(first, b1), S.tiled(second, b1)
        assert len(t0) <= CAP and s.kernel_for_batch(len(t0)) == "wform_ws"
        g0, j0, tv0 = s.solve_warm(t0, None)
        g1, j1, tv1 = s.solve_warm(t1, tv0)
    for a, b in ((g0, f0), (j0["status"], i0["status"]), (j0["iterations"], i0["iterations"]), (tv0, tu0),
                 (g1, f1), (j1["status"], i1["status"]), (j1["iterations"], i1["iterations"]), (tv1, tu1)):
        assert S.copies_identical(a, NREC) and _same(a[:NREC], b)
    po = oracle.default_params(N, 0)
    po.ipm_mu0 = 1e-6
    fo0, io0, _ = oracle.solve_warm(po, first, None, threads=8)
    fo1, io1, _ = oracle.solve_warm(po, second, tu0, threads=8)
    print(f"operands | warm start | workspace form at {len(t0)}: the all-LDS form's bytes on both ticks")
    _rules("operands, quat N=10, cold tick, all LDS", 4, first, f0, i0, fo0, io0)
    _rules("operands, quat N=10, warm tick on another stance set, all LDS", 4, second, f1, i1, fo1, io1)
