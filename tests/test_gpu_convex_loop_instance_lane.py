"""GPU suite (-m gpu): lane-kernel ticks for the closed loops with per-robot controller records on a ConvexMpc handle
(qmpc_set_convex_records + qmpc_set_convex_lane_records under QMPC_INSTANCES_AUTO, include/qmpc.h).

From the switch-over on the tick's solve is the stance sort (with a last class for robots that will not solve) and
qmpc_lane_cinst_kernel.  The bit contract of tests/test_gpu_convex_instance_lane.py carried over the ticks: uniform records give
the plain ConvexMpc loop's bytes on its lane tick, a mixed fleet equals its parts and its permutations, outcome records,
stop_when_down and push windows equal the same call with plant records only; against the wave family statuses are equal and
forces agree to the cross-family 1e-7 N.

Sizes: QMPC_LANE_CINST_MIN=1, QMPC_LANE_MIN=1 and QMPC_LOOP_FUSED=0 (read by qmpc_create) bring the lane tick down to 65 robots (a
tail across a wavefront) and 2500 (79 half-masked wavefronts); 24576 robots is the default switch-over at N = 10 (the larger of
the solve's 24576 and the cold loop's own 18432)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T0 = 6      # standing ticks before the robots walk


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


@pytest.fixture
def lane_everywhere(monkeypatch):
    monkeypatch.setenv("QMPC_LANE_CINST_MIN", "1")
    monkeypatch.setenv("QMPC_LANE_MIN", "1")
    monkeypatch.setenv("QMPC_LOOP_FUSED", "0")


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _all_same(got, want):
    return len(got) == len(want) and all(_same(a, b) for a, b in zip(got, want))


def _last(pkg, s):
    return pkg.KERNEL_FAMILY[s.query(pkg.QUERY_LAST_KERNEL)]


def _fleet(pkg, lib, B, seed=29):
    """the commands of the ConvexMpc loop tests (tests/test_gpu_convex_records.py): no roll / pitch rate command"""
    rng = np.random.default_rng(seed)
    lp = pkg.default_loop_params(lib)
    cmds = np.zeros((B, 7))
    cmds[:, 0] = 0.6 * rng.uniform(-0.5, 0.5, B); cmds[:, 1] = rng.uniform(-0.2, 0.2, B); cmds[:, 2] = rng.uniform(0.26, 0.32, B)
    cmds[:, 5] = rng.uniform(-0.5, 0.5, B); cmds[:, 6] = (rng.random(B) < 0.9).astype(float)
    cmds[cmds[:, 6] == 0, :2] = 0.0
    cmds[cmds[:, 6] == 0, 5] = 0.0
    stand = cmds.copy(); stand[:, 6] = 0.0
    return lp, pkg.loop_states(stand, lp, height=0.3, yaw=rng.uniform(-3, 3, B), lib=lib), cmds


def _walk(run, st, cmds, t0, t):
    st0 = run(st, t0, False)
    st0["movement_mode"] = cmds[:, 6]
    return run(st0, t, True)


def _solver(pkg, lib, p, B, lane=True):
    s = pkg.Solver(p, B, device=0, lib=lib)
    s.set_convex_records(True)
    if lane:
        s.set_instances_policy("auto")
        s.set_convex_lane_records(True)
    return s


@pytest.mark.parametrize("B,T,knobs", [(65, 20, True), (2500, 20, True), (24576, 15, False)])
def test_uniform_records_equal_the_plain_lane_tick(pkg, lib, monkeypatch, B, T, knobs):
    if knobs:
        for k, v in (("QMPC_LANE_CINST_MIN", "1"), ("QMPC_LANE_MIN", "1"), ("QMPC_LOOP_FUSED", "0")):
            monkeypatch.setenv(k, v)
    N = 10
    p = pkg.default_convex_params(N, pkg.MODE_CONVERGED, lib)
    lp, st, cmds = _fleet(pkg, lib, B)
    s = _solver(pkg, lib, p, B)
    assert s.loop_instances_plan(B, True, False) == ("per_tick", "lane")
    if not knobs:      # the default switch-over: one robot fewer stays on the wave kernels
        assert s.loop_instances_plan(B - 1, True, False) == ("per_tick", "wform_ws")
    ref = _walk(lambda x, t, tr: s.loop_run(x, t, lp, trace=tr), st, cmds, T0, T)
    assert _last(pkg, s) == "lane"
    ctrl, plant = pkg.instance_params(p, B), pkg.plant_params(p, B)
    got = _walk(lambda x, t, tr: s.loop_run_instances(x, t, lp, ctrl=ctrl, plant=plant, trace=tr), st, cmds, T0, T)
    assert _last(pkg, s) == "lane"
    only_ctrl = _walk(lambda x, t, tr: s.loop_run_instances(x, t, lp, ctrl=ctrl, trace=tr), st, cmds, T0, T)
    s.close()
    assert (ref[0]["tick"] == T0 + T).all() and (ref[0]["status"] == 0).mean() > 0.95 and (ref[2] == 0).any() and (ref[1] != 0).any()
    assert _all_same(got, ref) and _all_same(only_ctrl, ref)


def test_a_mixed_fleet_equals_its_parts_and_its_permutation(pkg, lib, lane_everywhere):
    B, T, N = 260, 20, 10
    p = pkg.default_convex_params(N, pkg.MODE_CONVERGED, lib)
    lp, st, cmds = _fleet(pkg, lib, B, seed=5)
    sets = pkg.random_go1_convex_variants(2, seed=9, base=p)
    sets["mu"] = np.maximum(sets["mu"], 0.5)
    ctrl = sets[np.arange(B) % 2]
    s = _solver(pkg, lib, p, B)
    run = lambda c: (lambda x, t, tr: s.loop_run_instances(x, t, lp, ctrl=c, trace=tr))      # noqa: E731
    fleet = _walk(run(ctrl), st, cmds, T0, T)
    assert _last(pkg, s) == "lane" and (fleet[0]["status"] == 0).mean() > 0.95 and (fleet[2] == 0).any()
    perm = np.random.default_rng(2).permutation(B)
    shuf = _walk(run(ctrl[perm]), st[perm], cmds[perm], T0, T)
    s.close()
    assert _same(shuf[0], fleet[0][perm]) and _same(shuf[1], fleet[1][:, perm]) and _same(shuf[2], fleet[2][:, perm])
    for g in range(2):      # a plain loop on a handle carrying the set: controller and plant are the set's robot
        idx = np.arange(g, B, 2)
        one = pkg.Solver(pkg.params_with(p, sets[g]), len(idx), device=0, lib=lib)
        want = _walk(lambda x, t, tr: one.loop_run(x, t, lp, trace=tr), st[idx], cmds[idx], T0, T)
        assert _last(pkg, one) == "lane"
        one.close()
        assert _same(want[0], fleet[0][idx]) and _same(want[1], fleet[1][:, idx]) and _same(want[2], fleet[2][:, idx]), g
    assert not _same(fleet[1][:, 0::2], fleet[1][:, 1::2])


def test_outcomes_halting_and_pushes_equal_the_plain_lane_tick(pkg, lib, lane_everywhere):
    """With uniform controller records the calls with outcome records, stop_when_down and push windows give the bytes of the same
    calls with plant records only, whose tick is the plain ConvexMpc lane tick."""
    B, TT, N = 130, 30, 10
    p = pkg.default_convex_params(N, pkg.MODE_CONVERGED, lib)
    lp, st, cmds = _fleet(pkg, lib, B, seed=17)
    st["movement_mode"] = cmds[:, 6]
    ctrl = pkg.instance_params(p, B)
    plant = pkg.random_go1_plants(B, seed=8, base=p)
    push = pkg.push_params(B, 2)
    push["start_tick"][:, 0], push["ticks"][:, 0] = 8.0, 3.0
    push["force_world"][:, 0, 1] = np.linspace(-40.0, 40.0, B)
    fall = np.arange(B) % 16 == 7
    push["start_tick"][fall, 1], push["ticks"][fall, 1], push["force_world"][fall, 1] = 2.0, 60.0, [0.0, 0.0, -2500.0]
    s = _solver(pkg, lib, p, B)
    for stop in (True, False):
        op = pkg.default_outcome_params(lib, stop_when_down=stop)
        want = s.loop_run_pushes(st, TT, push, lp, plant=plant, op=op, trace=True)
        assert _last(pkg, s) == "lane" and s.loop_instances_plan(B, False, False) == ("per_tick", "lane")
        got = s.loop_run_pushes(st, TT, push, lp, ctrl=ctrl, plant=plant, op=op, trace=True)
        assert _last(pkg, s) == "lane" and s.loop_instances_plan(B, True, False) == ("per_tick", "lane")
        assert _all_same(got, want)
        dt = got[1]["down_tick"]
        assert (dt[fall] > 2).all() and (dt[fall] < TT).all() and (dt[~fall] == -1).mean() > 0.9
        if stop:
            assert (got[0]["tick"][fall] == dt[fall]).all() and (got[0]["tick"][dt < 0] == TT).all()
        else:
            assert (got[0]["tick"] == TT).all()
        want = s.loop_run_outcomes(st, TT, lp, plant=plant, op=op, trace=True)
        got = s.loop_run_outcomes(st, TT, lp, ctrl=ctrl, plant=plant, op=op, trace=True)
        assert _last(pkg, s) == "lane" and _all_same(got, want)
    s.close()


@pytest.mark.parametrize("B", [65, 2500])
def test_rejected_records_frozen_plants_and_nan_states(pkg, lib, lane_everywhere, B):
    N = 10
    p = pkg.default_convex_params(N, pkg.MODE_CONVERGED, lib)
    lp, st, cmds = _fleet(pkg, lib, B, seed=31)
    ctrl = pkg.random_go1_convex_variants(B, seed=30, base=p)
    ctrl["mu"] = np.maximum(ctrl["mu"], 0.5)
    plant = pkg.random_go1_plants(B, seed=32, base=p, force=(0.0, 10.0))
    bad_c, bad_p, nan_s = 3, 8, 20
    ctrl["mu"][bad_c] = -1.0
    plant["inertia"][bad_p] = 0.0
    s = _solver(pkg, lib, p, B, lane=False)
    run = lambda x, t, tr: s.loop_run_instances(x, t, lp, ctrl=ctrl, plant=plant, trace=tr)      # noqa: E731
    st0 = run(st, T0, False)
    st0["movement_mode"] = cmds[:, 6]
    st0["pos_world"][nan_s, 0] = np.nan
    wave = run(st0, 12, True)
    assert s.loop_instances_plan(B, True, False) == ("per_tick", _last(pkg, s)) and _last(pkg, s).startswith("wform")
    s.set_instances_policy("auto")
    assert s.loop_instances_plan(B, True, False)[1].startswith("wform")      # (the lane form is a setting of its own)
    s.set_convex_lane_records(True)
    auto = run(st0, 12, True)
    assert s.loop_instances_plan(B, True, False) == ("per_tick", "lane") == ("per_tick", _last(pkg, s))
    s.close()
    frozen = [bad_c, bad_p]
    for i in frozen:
        a, b = st0[i].copy(), auto[0][i]
        assert b["status"] == pkg.BAD_PARAMS and b["iterations"] == 0
        a["status"], a["iterations"] = b["status"], b["iterations"]
        assert a.tobytes() == b.tobytes() == wave[0][i].tobytes()
        assert (auto[1][:, i] == 0).all() and (auto[2][:, i] == 0).all()
    assert np.array_equal(auto[0]["status"], wave[0]["status"])
    assert auto[0]["status"][nan_s] == pkg.NAN_INPUT and auto[0][nan_s].tobytes() == wave[0][nan_s].tobytes()
    assert _same(auto[1][:, nan_s], wave[1][:, nan_s]) and _same(auto[2][:, nan_s], wave[2][:, nan_s])
    rest = np.setdiff1d(np.arange(B), frozen + [nan_s])
    assert (auto[0]["status"][rest] == pkg.OK).mean() > 0.95 and _same(auto[2][:, rest], wave[2][:, rest])
    err = np.abs(auto[1][:, rest] - wave[1][:, rest]).max()
    print(f"B={B}: neighbours' forces within {err:.2e} N of the wave tick's over 12 ticks")
    assert err <= 1e-7


def test_refusals_keep_their_codes(pkg, lib, lane_everywhere):
    B = 65
    p = pkg.default_convex_params(10, pkg.MODE_CONVERGED, lib)
    lp, st, _ = _fleet(pkg, lib, B)
    ctrl, plant = pkg.instance_params(p, B), pkg.plant_params(p, B)

    def refused(call):
        with pytest.raises(pkg.QmpcError) as e:
            call()
        return e.value.code == pkg.UNSUPPORTED

    # ctrl with the warm start, whatever qmpc_set_loop_warm_records says
    s = _solver(pkg, lib, p, B)
    lib.qmpc_set_loop_warm_records(s._h, 1)
    warm = pkg.default_loop_params(lib)
    warm.warm_start = 1.0
    assert s.loop_instances_plan(B, True, True) is None and s.loop_instances_plan(B, True, False) == ("per_tick", "lane")
    assert refused(lambda: s.loop_run_instances(st, 2, warm, ctrl=ctrl, plant=plant))
    s.loop_run_instances(st, 2, lp, ctrl=ctrl, plant=plant)
    assert _last(pkg, s) == "lane"
    # a ConvexMpc handle without qmpc_set_convex_records: the lane setting alone accepts nothing
    s.set_convex_records(False)
    assert s.loop_instances_plan(B, True, False) is None
    assert refused(lambda: s.loop_run_instances(st, 2, lp, ctrl=ctrl, plant=plant))
    s.close()
    # the reference mode
    pr = pkg.default_convex_params(10, pkg.MODE_REFERENCE, lib)
    r = _solver(pkg, lib, pr, B)
    assert r.loop_instances_plan(B, True, False) is None and r.kernel_for_convex_instances(B) == "none"
    assert refused(lambda: r.loop_run_instances(st, 2, lp, ctrl=ctrl, plant=plant))
    assert refused(lambda: r.convex_solve_instances(pkg.random_go1_convex_states(B, config_id=13), ctrl))
    r.close()
