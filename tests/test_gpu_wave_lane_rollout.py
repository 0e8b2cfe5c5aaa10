"""GPU suite (-m gpu): the rollouts of the all-LDS one-wave kernels with the translation held one component per lane.

rollout_closed_w<..., LN> and rollout_scaled_w<..., ONEW> (qmpc_wform.h) keep p_a and v_a on lane a < 3 of a 16-lane row, form the
attitude error's component a and row 3 + a of e = Abar dx there, and pin every sum to the pairing the scalar knot compiles to.
The workspace forms run the scalar knot unchanged, so on the device they are the bit oracle: their forces, status words,
iteration words and -- with want_traj -- the state and input trajectories of every knot must be the all-LDS form's BYTES.
The cases are the ones in which the lane form takes another path or its operands leave the generators' range:
  QuatMpc, N = 1, 2, 3, 10, 11   a single knot; one pass through the paired knot loop and its odd tail; bench.py's kernel; a
                                 second trip of the lane loops -- record k on stance set k mod 15 of stance_sets.MASKS4
  8-point model, N = 1, 8        srbd_step_w is shared (k mod 16 of MASKS8)
  ConvexMpc, N = 1, 10           its rollouts are untouched: the control
  attitude sets, N = 10          records 6 k of attitude_sets.quat (all eight angles, 0.5 ... 3.5 rad: the reciprocal of q_o'q_c)
  motion sets, N = 10            records 45 k mod 360 + k // 8 of motion_sets.quat (all five rates up to 12 rad/s, all three
                                 speed classes; drop_ang_vel = 0): the midpoint quaternion far from unit norm
  far footholds, N = 10          the 64 `ahead` / `aside` records of foothold_sets.quat: steps are shortened in most
                                 iterations (rollout_scaled_w)
  warm start, N = 10             a cold solve on one stance set, then a warm-started one on another (stance_sets.warm_pairs)
64 records per case.  Rules, those of tests/test_gpu_wave_straightline_steps.py whose helpers this module takes: status words
equal to the oracle's and all 0; forces within 1e-6 N (8-point model: corner forces 1e-5, foot wrench 1e-7); swing forces exactly
0; iteration words equal to the oracle's on EVERY record; the workspace form on the tiled records the all-LDS form's bytes.  No
case is left out."""
import numpy as np
import pytest

import attitude_sets as A
import foothold_sets as F
import motion_sets as M
import stance_sets as S
from test_gpu_stance_sets import _first_batch_beyond, _handle, _last, _same
from test_gpu_wave_straightline_steps import CAP, MODELS, NREC, _rules

pytestmark = pytest.mark.gpu

CASES = [("quat", 1), ("quat", 2), ("quat", 3), ("quat", 10), ("quat", 11), ("biped8", 1), ("biped8", 8), ("convex", 1), ("convex", 10)]


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


def _both_forms_traj(pkg, lib, p, rec, call, tag):
    """(forces, info) of the all-LDS form on rec, after holding the workspace form on the tiled records to its bytes: the
    plain call and the one that returns the trajectories"""
    n = len(rec)
    with _handle(pkg, lib, p, CAP) as s:
        assert s.kernel_for_batch(n) == "wform_lds"
        f, info = getattr(s, call)(rec)
        assert _last(pkg, s) == "wform_lds"
        f2, info2, tu, tx = getattr(s, call)(rec, want_traj=True)
        assert _last(pkg, s) == "wform_lds"
        t = S.tiled(rec, _first_batch_beyond(s, "wform_lds", CAP))
        assert len(t) <= CAP and s.kernel_for_batch(len(t)) == "wform_ws"
        ft, it_ = getattr(s, call)(t)
        assert _last(pkg, s) == "wform_ws"
        ft2, it2, ttu, ttx = getattr(s, call)(t, want_traj=True)
        assert _last(pkg, s) == "wform_ws"
    nd = int((np.abs(ft[:n] - f).max(axis=1) > 0).sum())
    ndx = int((np.abs(ttx[:n] - tx).reshape(n, -1).max(axis=1) > 0).sum())
    print(f"lane-rollout | {tag} | workspace form at {len(t)} instances against the all-LDS form: forces of {nd} instances differ "
          f"(largest {float(np.abs(ft[:n] - f).max()):.2e} N), state trajectories of {ndx} (largest {float(np.abs(ttx[:n] - tx).max()):.2e}), "
          f"input trajectories largest {float(np.abs(ttu[:n] - tu).max()):.2e}, iteration words equal "
          f"{np.array_equal(it_['iterations'][:n], info['iterations'])}")
    assert np.isfinite(tx).all() and np.isfinite(tu).all(), tag
    for a in (ft, it_["status"], it_["iterations"], ft2, it2["status"], it2["iterations"], ttu, ttx):
        assert S.copies_identical(a, n), tag
    for a, b in ((ft, f), (it_["status"], info["status"]), (it_["iterations"], info["iterations"]), (ft2, f2),
                 (it2["status"], info2["status"]), (it2["iterations"], info2["iterations"]), (ttu, tu), (ttx, tx)):
        assert _same(a[:n], b), tag
    assert _same(f2, f) and _same(info2["status"], info["status"]) and _same(info2["iterations"], info["iterations"]), tag
    return f, info


@pytest.mark.parametrize("model,N", CASES, ids=[f"{m}-N{N}" for m, N in CASES])
def test_every_model_on_every_stance_set(pkg, lib, oracle, model, N):
    gen, config, params, call, masks, nl = MODELS[model]
    rec = getattr(pkg, gen)(NREC, config_id=config)
    rec["contacts"] = np.array(masks, dtype=np.float64)[np.arange(NREC) % len(masks)]
    fo, io = getattr(oracle, call)(getattr(oracle, params)(N, 0), rec, threads=8)
    tag = f"{model} N={N}"
    f, info = _both_forms_traj(pkg, lib, getattr(pkg, params)(N, pkg.MODE_CONVERGED, lib), rec, call, tag)
    _rules(tag + ", all LDS", nl, rec, f, info, fo, io)


def attitude_records(pkg):
    rec = A.quat(pkg, 10)[6 * np.arange(NREC)]
    assert sorted(set(A.grid_angle(rec).tolist())) == sorted(A.ANGLES)
    return rec


def motion_records(pkg):
    k = np.arange(NREC)
    rec = M.quat(pkg, 10)[(45 * k) % 360 + k // 8]
    assert sorted(set(M.grid_rate(rec).tolist())) == sorted(M.RATES) and len(np.unique(M.cell((45 * k) % 360 + k // 8)[3])) == len(M.SPEEDS)
    return rec


def test_attitude_errors_up_to_and_beyond_pi(pkg, lib, oracle):
    rec = attitude_records(pkg)
    fo, io = oracle.solve(oracle.default_params(10, 0), rec, threads=8)
    f, info = _both_forms_traj(pkg, lib, pkg.default_params(10, pkg.MODE_CONVERGED, lib), rec, "solve", "quat N=10, attitude sets")
    _rules("quat N=10, attitude sets, all LDS", 4, rec, f, info, fo, io)


def test_body_rates_up_to_12_rad_per_s(pkg, lib, oracle):
    rec = motion_records(pkg)
    fo, io = oracle.solve(M.params(oracle, "default_params", 10, 0), rec, threads=8)
    f, info = _both_forms_traj(pkg, lib, M.params(pkg, "default_params", 10, pkg.MODE_CONVERGED, lib), rec, "solve", "quat N=10, motion sets")
    _rules("quat N=10, motion sets, all LDS", 4, rec, f, info, fo, io)


def test_footholds_far_from_nominal(pkg, lib, oracle):
    N = 10
    far = np.isin(F.cells("quat", N)[0], [F.KINDS.index("ahead"), F.KINDS.index("aside")])
    rec = F.quat(pkg, N)[far]
    assert len(rec) == NREC
    fo, io = oracle.solve(oracle.default_params(N, 0), rec, threads=8)
    f, info = _both_forms_traj(pkg, lib, pkg.default_params(N, pkg.MODE_CONVERGED, lib), rec, "solve", "quat N=10, far from nominal")
    _rules("quat N=10, far from nominal, all LDS", 4, rec, f, info, fo, io)


def test_warm_started_second_solve_on_another_stance_set(pkg, lib, oracle):
    N = 10
    first, second = S.warm_pairs(pkg)
    pick = (7 * np.arange(NREC)) % len(first)
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
    print(f"lane-rollout | warm start | workspace form at {len(t0)}: the all-LDS form's bytes on both ticks")
    _rules("quat N=10, cold tick, all LDS", 4, first, f0, i0, fo0, io0)
    _rules("quat N=10, warm tick on another stance set, all LDS", 4, second, f1, i1, fo1, io1)
