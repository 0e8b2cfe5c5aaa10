"""GPU suite (-m gpu): lane-kernel ticks for the closed loop with per-robot controller records (qmpc_loop_run_instances* and
qmpc_loop_run_outcomes* under QMPC_INSTANCES_AUTO, include/qmpc.h).

From the switch-over on the tick's solve is the stance sort (with a last class for robots that will not solve), the lane kernel
with per-lane parameters to the loop's cap and the per-instance list kernel on the stragglers.  The bit contract of
tests/test_gpu_instance_lane.py carried over the ticks: uniform records give the plain loop's bytes, a mixed fleet equals its
parts, its shards and its permutations; against the wave family statuses are equal and forces agree to the cross-family 1e-7 N.
Sizes: 20480 robots is the smallest default-threshold size on the pair forms, 40960 reaches the plain 64-lane forms."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T0, T = 6, 24      # standing ticks, then walking ticks: swing phases occur

COMMANDS = [   # joy.{velx, vely, body_height, roll_rate, pitch_rate, yaw_rate}, movement_mode
    [0.0, 0.0, 0.30, 0.0, 0.0, 0.0, 0.0],
    [0.3, 0.0, 0.30, 0.0, 0.0, 0.0, 1.0],
    [0.2, -0.1, 0.28, 0.0, 0.0, 0.3, 1.0],
    [0.0, 0.0, 0.30, 0.1, -0.1, 0.0, 1.0],
    [-0.2, 0.05, 0.32, 0.0, 0.0, -0.2, 1.0],
    [0.0, 0.0, 0.27, 0.0, 0.0, 0.0, 0.0],
]


def _fleet(pkg, lib, B, seed=1):
    """B robots standing at their initial poses (movement 0) and the commands they walk with afterwards (the fleet of
    tests/test_gpu_loop_instances.py)"""
    lp = pkg.default_loop_params(lib)
    rng = np.random.default_rng(seed)
    cmds = np.array([COMMANDS[i % len(COMMANDS)] for i in range(B)])
    cmds[:, 0] += rng.uniform(-0.1, 0.1, B) * cmds[:, 6]
    stand = cmds.copy(); stand[:, 6] = 0.0
    st = pkg.loop_states(stand, lp, height=0.3, yaw=rng.uniform(-3, 3, B), lib=lib)
    return lp, st, cmds


def _walk(run, st, cmds, t0, t):
    st0 = run(st, t0, False)
    st0["movement_mode"] = cmds[:, 6]
    return run(st0, t, True)


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _falling(pkg, lib, B):
    """The falling population of tests/test_gpu_loop_outcome.py: every second robot carries ext_force_world[2] = -1000 N (weight
    126 N, 4 x fz_max = 400 N of lift at most: 0.15 m of drop take 11.7 .. 14.6 ticks), the others are their controller's robot"""
    p = pkg.default_params(10, pkg.MODE_CONVERGED, lib)
    assert abs(p.mass - 12.84) < 1e-12 and p.fz_max == 100.0
    lp = pkg.default_loop_params(lib)
    st = pkg.loop_states([[0.0, 0.0, 0.30, 0.0, 0.0, 0.0, 0.0]] * B, lp, height=0.3, yaw=np.linspace(-3, 3, B), lib=lib)
    plant = pkg.plant_params(p, B)
    loaded = np.arange(B) % 2 == 1
    plant["ext_force_world"][loaded, 2] = -1000.0
    return p, lp, st, plant, loaded


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


def _last(pkg, s):
    return pkg.KERNEL_FAMILY[s.query(pkg.QUERY_LAST_KERNEL)]


def _auto(pkg, lib, p, B):
    s = pkg.Solver(p, B, device=0, lib=lib)
    s.set_instances_policy("auto")
    return s


def _pressed(st, cmds):
    """In-gait states of _fleet stay below the loop's cap (10 iterations at the cuts measured on the device), so every 8th robot
    is pressed: it walks with a fast diagonal command with roll, pitch and yaw rates, from a state with a 0.6 m/s sideways and
    0.4 m/s downward velocity and a 1.5 rad/s roll rate"""
    sub = np.arange(len(st)) % 8 == 5
    cmds[sub] = [0.5, -0.2, 0.26, 0.3, -0.3, 0.6, 1.0]
    st["lin_vel_world"][sub] = [0.0, 0.6, -0.4]
    st["ang_vel_body"][sub] = [1.5, 0.0, 0.0]
    return sub


def test_plan_and_family_follow_the_policy(pkg, lib):
    N, B, S = 10, 20480, 3000
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    lp, st, cmds = _fleet(pkg, lib, B, seed=21)
    ctrl = pkg.random_go1_variants(B, seed=22, base=p)
    ctrl["mu"] = np.maximum(ctrl["mu"], 0.5)
    s = pkg.Solver(p, B, device=0, lib=lib)
    run = lambda x, t, tr: s.loop_run_instances(x, t, lp, ctrl=ctrl[:len(x)], trace=tr)      # noqa: E731
    assert s.instances_policy() == "wave" and s.loop_instances_plan(B, True, False) == ("per_tick", "wform_ws")
    plain = s.loop_instances_plan(B, False, False)
    w0 = _walk(run, st, cmds, T0, T)
    assert _last(pkg, s) == "wform_ws"
    s.set_instances_policy("auto")
    assert s.loop_instances_plan(B, True, False) == ("per_tick", "lane_handoff")
    # nothing else moves: no controller records, the warm start's refusal, the sizes below the switch-over
    assert s.loop_instances_plan(B, False, False) == plain and s.loop_instances_plan(B, True, True) is None
    assert s.loop_instances_plan(S, True, False) == ("per_tick", "wform_ws") and s.loop_instances_plan(1024, True, False)[0] == "persistent"
    a0 = _walk(run, st, cmds, T0, T)
    assert _last(pkg, s) == "lane_handoff"
    assert np.array_equal(a0[0]["status"], w0[0]["status"]) and (a0[0]["tick"] == T0 + T).all() and (a0[2] == 0).any()
    assert not _same(a0[1], w0[1])      # (another rounding family)
    # below the switch-over AUTO is the wave form, bit for bit
    sa = _walk(run, st[:S], cmds[:S], T0, T)
    assert _last(pkg, s) == "wform_ws"
    s.set_instances_policy("wave")
    assert s.loop_instances_plan(B, True, False) == ("per_tick", "wform_ws")
    w1 = _walk(run, st, cmds, T0, T)
    assert _last(pkg, s) == "wform_ws"
    for a, b in zip(w0, w1):
        assert _same(a, b)
    sw = _walk(run, st[:S], cmds[:S], T0, T)
    s.close()
    for a, b in zip(sa, sw):
        assert _same(a, b)


@pytest.mark.parametrize("N,B", [(10, 20480), (10, 40960), (20, 20480)])
def test_uniform_records_equal_the_plain_loop(pkg, lib, N, B):
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    lp, st, cmds = _fleet(pkg, lib, B, seed=23)
    sub = _pressed(st, cmds)
    s = _auto(pkg, lib, p, B)
    cap = s.query(pkg.QUERY_LANE_CAP, 2)
    ref = _walk(lambda x, t, tr: s.loop_run(x, t, lp, trace=tr), st, cmds, T0, T)
    assert _last(pkg, s) == "lane_handoff"
    ctrl, plant = pkg.instance_params(p, B), pkg.plant_params(p, B)
    got = _walk(lambda x, t, tr: s.loop_run_instances(x, t, lp, ctrl=ctrl, plant=plant, trace=tr), st, cmds, T0, T)
    assert _last(pkg, s) == "lane_handoff" and s.loop_instances_plan(B, True, False) == ("per_tick", "lane_handoff")
    # every robot's largest iteration count over all ticks: the outcome records of the same run (they change nothing else)
    x0, oc = s.loop_run_outcomes(st, T0, lp, ctrl=ctrl, plant=plant)
    x0["movement_mode"] = cmds[:, 6]
    x1, oc = s.loop_run_outcomes(x0, T, lp, ctrl=ctrl, plant=plant, outcomes=oc)
    s.close()
    its = oc["iterations_max"]
    print(f"N={N} B={B}: cap {cap}, {int((its > cap).sum())} robots beyond it in some tick ({int((its[sub] > cap).sum())} of the pressed "
          f"{int(sub.sum())}), most iterations {int(its.max())}, final status words {np.unique(ref[0]['status']).tolist()}")
    assert cap > 0 and (its > cap).any()      # the hand-off's list kernel took part
    assert (ref[0]["status"][~sub] == 0).all() and (ref[0]["tick"] == T0 + T).all() and (ref[2] == 0).any()
    assert _same(x1, ref[0])
    for a, b in zip(ref, got):
        assert _same(a, b)


def test_a_mixed_fleet_equals_its_parts(pkg, lib):
    N, B, H = 10, 40960, 20480
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    lp, st, cmds = _fleet(pkg, lib, B, seed=24)
    v = pkg.random_go1_variants(2, seed=25, base=p)
    v["mu"] = np.maximum(v["mu"], 0.5)
    ctrl = v[np.arange(B) % 2]
    s = _auto(pkg, lib, p, B)
    run = lambda c: (lambda x, t, tr: s.loop_run_instances(x, t, lp, ctrl=c, trace=tr))      # noqa: E731
    fleet = _walk(run(ctrl), st, cmds, T0, T)
    assert _last(pkg, s) == "lane_handoff" and (fleet[0]["status"] == 0).all() and (fleet[2] == 0).any()
    shard = _walk(run(ctrl[:H]), st[:H], cmds[:H], T0, T)
    assert _last(pkg, s) == "lane_handoff"
    perm = np.random.default_rng(3).permutation(B)
    shuf = _walk(run(ctrl[perm]), st[perm], cmds[perm], T0, T)
    s.close()
    assert _same(shard[0], fleet[0][:H]) and _same(shard[1], fleet[1][:, :H]) and _same(shard[2], fleet[2][:, :H])
    assert _same(shuf[0], fleet[0][perm]) and _same(shuf[1], fleet[1][:, perm]) and _same(shuf[2], fleet[2][:, perm])
    for k in range(2):
        one = pkg.Solver(pkg.params_with(p, v[k]), H, device=0, lib=lib)
        r = _walk(lambda x, t, tr: one.loop_run(x, t, lp, trace=tr), st[k::2], cmds[k::2], T0, T)
        assert _last(pkg, one) == "lane_handoff"
        one.close()
        assert _same(r[0], fleet[0][k::2]) and _same(r[1], fleet[1][:, k::2]) and _same(r[2], fleet[2][:, k::2]), k


def test_one_walking_tick_against_the_wave_family(pkg, lib):
    N, B = 10, 20480
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    lp, st, cmds = _fleet(pkg, lib, B, seed=26)
    ctrl = pkg.random_go1_variants(B, seed=27, base=p)
    ctrl["mu"] = np.maximum(ctrl["mu"], 0.5)
    plant = pkg.random_go1_plants(B, seed=28, base=p, force=(0.0, 10.0))
    s = pkg.Solver(p, B, device=0, lib=lib)
    run = lambda x, t, tr: s.loop_run_instances(x, t, lp, ctrl=ctrl, plant=plant, trace=tr)      # noqa: E731
    x = _walk(run, st, cmds, T0, 13)[0]      # walking: some feet swing
    xw, fw, cw = run(x, 1, True)
    assert _last(pkg, s) == "wform_ws"
    s.set_instances_policy("auto")
    xa, fa, ca = run(x, 1, True)
    assert _last(pkg, s) == "lane_handoff"
    s.close()
    assert (cw == 0).any() and _same(ca, cw)
    limit = (xa["iterations"] == p.iterations_max) | (xw["iterations"] == p.iterations_max)
    both = (xa["status"] == pkg.OK) & (xw["status"] == pkg.OK)
    err = np.abs(fa[0] - fw[0]).max(axis=1)
    print(f"one tick, {B} robots: {int(limit.sum())} robots at the iteration limit left out, {int(both.sum())} converged in both, "
          f"worst force difference there {err[both & ~limit].max():.2e} N (all robots: {err.max():.2e})")
    assert limit.sum() <= B // 100
    assert np.array_equal(xa["status"][~limit], xw["status"][~limit])
    assert both.mean() > 0.9 and err[both & ~limit].max() <= 1e-7


def test_outcome_records_and_halting(pkg, lib):
    B, TT = 20480, 40
    p, lp, st, plant, loaded = _falling(pkg, lib, B)
    ctrl = pkg.instance_params(p, B)
    s = _auto(pkg, lib, p, B)
    for stop in (True, False):
        op = pkg.default_outcome_params(lib, stop_when_down=stop)
        want = s.loop_run_outcomes(st, TT, lp, plant=plant, op=op, trace=True)      # no controller records: the plain lane tick
        assert _last(pkg, s) == "lane_handoff"
        got = s.loop_run_outcomes(st, TT, lp, ctrl=ctrl, plant=plant, op=op, trace=True)
        assert _last(pkg, s) == "lane_handoff"
        for a, b in zip(want, got):
            assert _same(a, b)
        dt = got[1]["down_tick"]
        assert ((10 <= dt[loaded]) & (dt[loaded] <= 18)).all() and (dt[~loaded] == -1).all()
        if stop:
            assert (got[0]["tick"][loaded] == dt[loaded]).all() and (got[0]["tick"][~loaded] == TT).all()
            assert all((got[2][int(dt[i]):, i] == 0).all() for i in np.flatnonzero(loaded)[:64])
        else:
            assert (got[0]["tick"] == TT).all()
        a = s.loop_run_outcomes(st, 15, lp, ctrl=ctrl, plant=plant, op=op, trace=True)      # (some robots are down by tick 15, some not)
        b = s.loop_run_outcomes(a[0], TT - 15, lp, ctrl=ctrl, plant=plant, op=op, outcomes=a[1], trace=True)
        assert _same(got[0], b[0]) and _same(got[1], b[1])
        assert _same(got[2], np.concatenate([a[2], b[2]])) and _same(got[3], np.concatenate([a[3], b[3]]))
    # ... and with no records at all on the other side: controller records alone (nobody falls)
    op = pkg.default_outcome_params(lib, stop_when_down=True)
    want = s.loop_run_outcomes(st, 8, lp, op=op, trace=True)
    got = s.loop_run_outcomes(st, 8, lp, ctrl=ctrl, op=op, trace=True)
    s.close()
    for a, b in zip(want, got):
        assert _same(a, b)


@pytest.mark.parametrize("B,variant", [(1, None), (65, None), (2500, None), (65, "4")])
def test_rejected_records_and_tails(pkg, lib, monkeypatch, B, variant):
    monkeypatch.setenv("QMPC_LANE_INST_MIN", "1")
    monkeypatch.setenv("QMPC_LANE_MIN", "1")
    monkeypatch.setenv("QMPC_LOOP_FUSED", "0")
    if variant:
        monkeypatch.setenv("QMPC_VARIANT", variant)
    N = 10
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    lp, st, cmds = _fleet(pkg, lib, B, seed=29)
    ctrl = pkg.random_go1_variants(B, seed=30, base=p)
    ctrl["mu"] = np.maximum(ctrl["mu"], 0.5)
    plant = pkg.random_go1_plants(B, seed=31, base=p, force=(0.0, 10.0))
    # (the sort takes a robot that will not solve from its index to the end of the order)
    bad_c, bad_p, nan_s = (0, None, None) if B == 1 else (3, 8, 20)
    ctrl["mu"][bad_c] = -1.0
    if bad_p is not None:
        plant["inertia"][bad_p] = 0.0
    s = pkg.Solver(p, B, device=0, lib=lib)
    run = lambda x, t, tr: s.loop_run_instances(x, t, lp, ctrl=ctrl, plant=plant, trace=tr)      # noqa: E731
    st0 = run(st, T0, False)
    st0["movement_mode"] = cmds[:, 6]
    if nan_s is not None:
        st0["pos_world"][nan_s, 0] = np.nan
    wave = run(st0, 12, True)
    assert s.loop_instances_plan(B, True, False) == ("per_tick", _last(pkg, s)) and _last(pkg, s).startswith("wform")
    s.set_instances_policy("auto")
    auto = run(st0, 12, True)
    assert s.loop_instances_plan(B, True, False) == ("per_tick", "lane" if variant else "lane_handoff") == ("per_tick", _last(pkg, s))
    s.close()
    frozen = [i for i in (bad_c, bad_p) if i is not None]
    for i in frozen:
        a, b = st0[i].copy(), auto[0][i]
        assert b["status"] == pkg.BAD_PARAMS and b["iterations"] == 0
        a["status"], a["iterations"] = b["status"], b["iterations"]
        assert a.tobytes() == b.tobytes() == wave[0][i].tobytes()
        assert (auto[1][:, i] == 0).all() and (auto[2][:, i] == 0).all()
    assert np.array_equal(auto[0]["status"], wave[0]["status"])
    if nan_s is not None:
        assert auto[0]["status"][nan_s] == pkg.NAN_INPUT
    rest = np.setdiff1d(np.arange(B), frozen + ([nan_s] if nan_s is not None else []))
    if len(rest):
        assert (auto[0]["status"][rest] == pkg.OK).all() and _same(auto[2][:, rest], wave[2][:, rest])
        err = np.abs(auto[1][:, rest] - wave[1][:, rest]).max()
        print(f"B={B} variant {variant}: neighbours' forces within {err:.2e} N of the wave family's over 12 ticks")
        assert err <= 1e-7


def test_device_entry_and_buffers(pkg, lib):
    import torch

    N, B, TT = 10, 20480, 8
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    lp, st, cmds = _fleet(pkg, lib, B, seed=32)
    st["movement_mode"] = cmds[:, 6]
    ctrl = pkg.random_go1_variants(B, seed=33, base=p)
    ctrl["mu"] = np.maximum(ctrl["mu"], 0.5)
    plant = pkg.random_go1_plants(B, seed=34, base=p)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1).copy()).cuda()      # noqa: E731

    def device_run(s):
        d_st, d_ctrl, d_plant = dev(st), dev(ctrl), dev(plant)
        d_tf = torch.full((TT, B, 12), 7.0, dtype=torch.float64, device="cuda")
        d_tc = torch.full((TT, B, 4), 7.0, dtype=torch.float64, device="cuda")
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        s.loop_run_instances_device(B, d_st.data_ptr(), TT, lp, d_ctrl=d_ctrl.data_ptr(), d_plant=d_plant.data_ptr(),
                                    d_trace_forces=d_tf.data_ptr(), d_trace_contacts=d_tc.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        return d_st.cpu().numpy().tobytes(), d_tf.cpu().numpy(), d_tc.cpu().numpy()

    s = _auto(pkg, lib, p, B)
    s.prepare(B)
    held = s.query(pkg.QUERY_DEVICE_BYTES)
    got = device_run(s)
    assert _last(pkg, s) == "lane_handoff"
    assert s.query(pkg.QUERY_DEVICE_BYTES) == held and s.query(pkg.QUERY_HANDOFF_ALLOC_FAILED) == 0
    # a call with ticks = 0 on a fresh handle allocates the same buffers and launches nothing
    z = _auto(pkg, lib, p, B)
    z.prepare(B)
    z_held = z.query(pkg.QUERY_DEVICE_BYTES)
    z.close()
    z = _auto(pkg, lib, p, B)
    before = z.query(pkg.QUERY_DEVICE_BYTES)
    assert _same(z.loop_run_instances(st, 0, lp, ctrl=ctrl, plant=plant), st)
    grown = z.query(pkg.QUERY_DEVICE_BYTES) - before
    z.close()
    want = s.loop_run_instances(st, TT, lp, ctrl=ctrl, plant=plant, trace=True)
    s.close()
    assert got[0] == want[0].tobytes() and _same(got[1], want[1]) and _same(got[2], want[2])
    assert (want[0]["status"] == 0).all()
    # under the default policy prepare and a run allocate what they allocated before there was a lane form: on a handle whose
    # policy was never set and on one that went to AUTO and back, the per-instance and plant blocks (1028 B per robot) only
    counts = []
    for back in (False, True):
        w = pkg.Solver(p, B, device=0, lib=lib)
        if back:
            w.set_instances_policy("auto")
            w.set_instances_policy("wave")
        w.prepare(B)
        prepared = w.query(pkg.QUERY_DEVICE_BYTES)
        device_run(w)
        assert _last(pkg, w) == "wform_ws"
        counts.append((prepared, w.query(pkg.QUERY_DEVICE_BYTES)))
        w.close()
    assert counts[0] == counts[1] and counts[0][1] - counts[0][0] == 1028 * B
    # AUTO holds what WAVE holds plus the lane kernel's parameter rows (the other lane buffers a prepared handle has anyway)
    print(f"device bytes: AUTO prepared {held}, ticks=0 call grew {grown}, fresh prepared {z_held - before}, WAVE {counts[0]}")
    assert held > counts[0][1] and grown > 1028 * B
