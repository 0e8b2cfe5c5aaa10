"""GPU suite (-m gpu): the closed loop with per-robot controller and plant records (qmpc_loop_run_instances*, include/qmpc.h).

Robot i runs the handle's controller with the seven fields of its controller record in place, and its plant integrates with its
own mass, inertia and constant disturbance wrench.  Uniform records reproduce the plain loop bit for bit, the two launch forms
agree bit for bit, a fleet equals one robot per handle, and under model mismatch the device loop follows the host twin
(host/ClosedLoopHost.h) tick for tick."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COMMANDS = [   # joy.{velx, vely, body_height, roll_rate, pitch_rate, yaw_rate}, movement_mode
    [0.0, 0.0, 0.30, 0.0, 0.0, 0.0, 0.0],
    [0.3, 0.0, 0.30, 0.0, 0.0, 0.0, 1.0],
    [0.2, -0.1, 0.28, 0.0, 0.0, 0.3, 1.0],
    [0.0, 0.0, 0.30, 0.1, -0.1, 0.0, 1.0],
    [-0.2, 0.05, 0.32, 0.0, 0.0, -0.2, 1.0],
    [0.0, 0.0, 0.27, 0.0, 0.0, 0.0, 0.0],
]


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


def _fleet(pkg, lib, B, seed=1):
    """B robots standing at their initial poses (movement 0) and the commands they walk with afterwards"""
    lp = pkg.default_loop_params(lib)
    rng = np.random.default_rng(seed)
    cmds = np.array([COMMANDS[i % len(COMMANDS)] for i in range(B)])
    cmds[:, 0] += rng.uniform(-0.1, 0.1, B) * cmds[:, 6]
    stand = cmds.copy(); stand[:, 6] = 0.0
    st = pkg.loop_states(stand, lp, height=0.3, yaw=rng.uniform(-3, 3, B), lib=lib)
    return lp, st, cmds


def _walk(run, st, cmds, T0, T):
    st0 = run(st, T0, False)
    st0["movement_mode"] = cmds[:, 6]
    return run(st0, T, True)


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.mark.parametrize("N,B,warm", [(10, 96, False), (10, 1024, False), (20, 40, False), (10, 3000, False), (10, 256, True)])
def test_uniform_records_give_the_plain_loop_bits(pkg, lib, N, B, warm):
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    lp, st, cmds = _fleet(pkg, lib, B)
    lp.warm_start = 1.0 if warm else 0.0
    s = pkg.Solver(p, B, device=0, lib=lib)
    ref = _walk(lambda x, t, tr: s.loop_run(x, t, lp, trace=tr), st, cmds, 6, 40)
    ctrl = None if warm else pkg.instance_params(p, B)      # (controller records are refused with the warm start)
    plant = pkg.plant_params(p, B)
    got = _walk(lambda x, t, tr: s.loop_run_instances(x, t, lp, ctrl=ctrl, plant=plant, trace=tr), st, cmds, 6, 40)
    form = s.loop_instances_plan(B, ctrl is not None, warm)
    if B > 2048:
        # the per-tick form: the per-instance solve takes the variant of the plain loop's tick
        assert form[0] == "per_tick" and form == s.loop_instances_plan(B, False, warm)
    else:
        assert form[0] == "persistent"
    # ... and so do the controller records alone and the plant records alone
    only = [(None, plant)] + ([] if warm else [(ctrl, None)])
    outs = [_walk(lambda x, t, tr: s.loop_run_instances(x, t, lp, ctrl=c, plant=q, trace=tr), st, cmds, 6, 40) for c, q in only]
    s.close()
    assert (ref[0]["status"] == 0).all() and (ref[0]["tick"] == 46).all() and (ref[2] == 0).any()
    for out in [got] + outs:
        for a, b in zip(ref, out):
            assert _same(a, b)


@pytest.mark.parametrize("robots,ticks,horizon,ctrl,warm", [(200, 60, 10, "ctrl", "cold"), (200, 60, 10, "noctrl", "warm"),
                                                           (96, 40, 20, "ctrl", "cold")])
def test_launch_forms_give_the_same_bits(robots, ticks, horizon, ctrl, warm):
    worker = Path(__file__).resolve().parent / "_loop_instances_worker.py"
    out = {}
    for fused in ("0", "1"):
        env = dict(os.environ, QMPC_LOOP_FUSED=fused)
        r = subprocess.run([sys.executable, str(worker), str(robots), str(ticks), str(horizon), ctrl, warm], env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.splitlines()
        out[fused] = ([l for l in lines if l.startswith("FORM")][0], [l for l in lines if l.startswith("SHA")][0])
    print(out)
    f0, f1 = eval(out["0"][0][5:]), eval(out["1"][0][5:])
    assert f0[0] == "per_tick" and f1[0] == "persistent" and f0[1] == f1[1]      # the same solve variant in both forms
    assert out["0"][1] == out["1"][1]
    assert int(out["1"][1].split()[3]) > 0          # swing phases happened


def test_a_fleet_equals_one_robot_per_handle(pkg, lib):
    N, B = 10, 64
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    lp, st, cmds = _fleet(pkg, lib, B, seed=2)
    ctrl = pkg.random_go1_variants(B, seed=5, base=p)
    ctrl["mu"] = np.maximum(ctrl["mu"], 0.5)
    s = pkg.Solver(p, B, device=0, lib=lib)
    fleet = _walk(lambda x, t, tr: s.loop_run_instances(x, t, lp, ctrl=ctrl, trace=tr), st, cmds, 6, 50)
    perm = np.random.default_rng(0).permutation(B)
    shuf = _walk(lambda x, t, tr: s.loop_run_instances(x, t, lp, ctrl=ctrl[perm], trace=tr), st[perm], cmds[perm], 6, 50)
    s.close()
    assert _same(shuf[0], fleet[0][perm]) and _same(shuf[1], fleet[1][:, perm]) and _same(shuf[2], fleet[2][:, perm])
    for i in (0, 1, 7, 22, 41, 63):
        one = pkg.Solver(pkg.params_with(p, ctrl[i]), 1, device=0, lib=lib)
        r = _walk(lambda x, t, tr: one.loop_run(x, t, lp, trace=tr), st[i:i + 1], cmds[i:i + 1], 6, 50)
        one.close()
        assert _same(r[0], fleet[0][i:i + 1]) and _same(r[1], fleet[1][:, i:i + 1]) and _same(r[2], fleet[2][:, i:i + 1]), i


def _host(pkg):
    import __graft_entry__ as g

    host = C.CDLL(str(g.build_host()))
    vp = C.c_void_p
    host.qh_loop_create_robot.argtypes = [C.c_char_p, C.c_int, vp, vp, vp, vp]
    host.qh_loop_create_robot.restype = vp
    for f in ("qh_loop_tick", "qh_loop_destroy", "qh_loop_device_status"):
        getattr(host, f).argtypes = [vp]
    host.qh_loop_export.argtypes = [vp, vp]
    host.qh_loop_set_command.argtypes = [vp, vp, C.c_double]
    return host


def _against_host(pkg, host, st_init, cmds, N, lp, ctrl, plant, robots, T0, T, tf, tc, final):
    """robots `robots` of a device run against the host twin, every tick; returns (worst force, worst state difference)"""
    worst_f = worst_x = 0.0
    for i in robots:
        cp = None if ctrl is None else ctrl[i:i + 1].ctypes.data
        pp = None if plant is None else plant[i:i + 1].ctypes.data
        h = host.qh_loop_create_robot(str(pkg.LIB_PATH).encode(), N, C.addressof(lp), st_init[i:i + 1].ctypes.data, cp, pp)
        assert h and host.qh_loop_device_status(h) == 0
        e = np.zeros(1, dtype=pkg.LOOP_STATE_DTYPE)
        for _ in range(T0):
            assert host.qh_loop_tick(h) == 1
        host.qh_loop_set_command(h, np.ascontiguousarray(cmds[i, :6]).ctypes.data, float(cmds[i, 6]))
        for t in range(T):
            assert host.qh_loop_tick(h) == 1, (i, t)
            host.qh_loop_export(h, e.ctypes.data)
            assert np.array_equal(e[0]["contacts"], tc[t, i]), (i, t)
            worst_f = max(worst_f, float(np.abs(e[0]["forces_body"] - tf[t, i]).max()))
        host.qh_loop_destroy(h)
        d, r = final[i], e[0]
        for k in ("pos_world", "quat", "lin_vel_world", "ang_vel_body", "foot_pos_world", "pos_d_world", "quat_d", "grf_world"):
            worst_x = max(worst_x, float(np.abs(d[k] - r[k]).max()))
        for k in ("gait_phase", "state", "pattern_index"):
            assert np.array_equal(d["leg"][k], r["leg"][k]), (i, k)
    return worst_f, worst_x


def test_device_equals_the_host_twin_under_model_mismatch(pkg, lib):
    N, T0, T = 10, 6, 130
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    lp, st, cmds = _fleet(pkg, lib, 6, seed=3)
    cmds[:, 6] = 1.0
    ctrl = pkg.instance_params(p, 6)
    plant = pkg.plant_params(p, 6)
    plant["mass"][0] += 3.0                                        # heavier plant
    plant["mass"][1] -= 2.0                                        # lighter plant
    plant["inertia"][2] = (np.asarray(p.inertia[:]).reshape(3, 3) * np.array([1.3, 0.8, 1.1])[:, None] ** 0.5
                           * np.array([1.3, 0.8, 1.1])[None, :] ** 0.5).ravel()
    plant["inertia"][2][[1, 3]] = 0.002                            # skewed inertia
    plant["ext_force_world"][3] = [0.0, 12.0, 0.0]                 # lateral disturbance
    plant["ext_torque_body"][4] = [0.0, 0.0, 0.8]                  # yaw disturbance
    v = pkg.random_go1_variants(6, seed=9, base=p)[5]              # a controller record AND a mismatched plant
    v["mu"] = 0.6
    ctrl[5] = v
    plant["mass"][5] = v["mass"] + 1.5
    s = pkg.Solver(p, 6, device=0, lib=lib)
    fin, tf, tc = _walk(lambda x, t, tr: s.loop_run_instances(x, t, lp, ctrl=ctrl, plant=plant, trace=tr), st, cmds, T0, T)
    s.close()
    assert (fin["status"] == 0).all() and (fin["tick"] == T0 + T).all()
    wf, wx = _against_host(pkg, _host(pkg), st, cmds, N, lp, ctrl, plant, range(6), T0, T, tf, tc, fin)
    print(f"model mismatch, 6 robots x {T} ticks: worst force difference {wf:.2e} N, worst state difference {wx:.2e}")
    assert wf <= 1e-6 and wx <= 1e-8
    assert (tc == 0).sum() > 100 and ((0.2 < fin["pos_world"][:, 2]) & (fin["pos_world"][:, 2] < 0.4)).all()


def test_the_plant_really_is_the_plant(pkg, lib):
    p = pkg.default_params(10, pkg.MODE_CONVERGED, lib)
    lp = pkg.default_loop_params(lib)
    st = pkg.loop_states([[0.0, 0.0, 0.30, 0.0, 0.0, 0.0, 0.0]] * 4, lp, height=0.3, yaw=0.0, lib=lib)
    plant = pkg.plant_params(p, 4)
    plant["mass"][1] += 2.0
    plant["mass"][2] += 4.0
    plant["ext_force_world"][3] = [20.0, 0.0, 0.0]                 # +x push on the nominal robot
    s = pkg.Solver(p, 4, device=0, lib=lib)
    out = s.loop_run_instances(st, 400, lp, plant=plant)
    s.close()
    z = out["pos_world"][:, 2]
    err = 0.3 - z[:3]
    print("height error at +0 / +2 / +4 kg:", err, "x drift under the push:", out["pos_world"][3, 0] - out["pos_world"][0, 0])
    assert (out["status"] == 0).all() and ((0.2 < z) & (z < 0.4)).all()
    assert err[0] < err[1] < err[2]
    assert out["pos_world"][3, 0] > out["pos_world"][0, 0] + 1e-3


def test_bad_records_freeze_only_their_robot(pkg, lib):
    N, B = 10, 12
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    lp, st, cmds = _fleet(pkg, lib, B, seed=6)
    ctrl = pkg.random_go1_variants(B, seed=7, base=p)
    ctrl["mu"] = np.maximum(ctrl["mu"], 0.5)
    plant = pkg.random_go1_plants(B, seed=8, base=p, force=(0.0, 10.0))
    s = pkg.Solver(p, B, device=0, lib=lib)
    st0 = s.loop_run_instances(st, 6, lp, ctrl=ctrl, plant=plant)
    st0["movement_mode"] = cmds[:, 6]
    good = s.loop_run_instances(st0, 30, lp, ctrl=ctrl, plant=plant, trace=True)
    bc, bp = ctrl.copy(), plant.copy()
    bc["mu"][3] = -1.0                 # invalid controller record
    bp["inertia"][8] = 0.0             # invalid (singular) plant record
    bad = s.loop_run_instances(st0, 30, lp, ctrl=bc, plant=bp, trace=True)
    s.close()
    others = [i for i in range(B) if i not in (3, 8)]
    assert _same(bad[0][others], good[0][others]) and _same(bad[1][:, others], good[1][:, others])
    assert _same(bad[2][:, others], good[2][:, others])
    for i in (3, 8):
        a, b = st0[i].copy(), bad[0][i]
        assert b["status"] == pkg.BAD_PARAMS and b["iterations"] == 0 and b["tick"] == st0[i]["tick"]
        a["status"], a["iterations"] = b["status"], b["iterations"]
        assert a.tobytes() == b.tobytes()
        assert (bad[1][:, i] == 0).all() and (bad[2][:, i] == 0).all()


def test_large_batches(pkg, lib):
    N, B, T0, T = 10, 32768, 6, 20
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    lp, st, cmds = _fleet(pkg, lib, B, seed=10)
    plant = pkg.random_go1_plants(B, seed=11, base=p, payload=(-1.0, 3.0), force=(0.0, 10.0))
    s = pkg.Solver(p, B, device=0, lib=lib)
    form = s.loop_instances_plan(B, False, False)
    assert form[0] == "per_tick" and form[1] in ("lane", "lane_handoff")
    fin, tf, tc = _walk(lambda x, t, tr: s.loop_run_instances(x, t, lp, plant=plant, trace=tr), st, cmds, T0, T)
    assert pkg.KERNEL_FAMILY[s.query(pkg.QUERY_LAST_KERNEL)] == form[1]
    assert (fin["status"] == 0).all() and (fin["tick"] == T0 + T).all()
    ctrl = pkg.random_go1_variants(B, seed=12, base=p)
    ctrl["mu"] = np.maximum(ctrl["mu"], 0.5)
    assert s.loop_instances_plan(B, True, False) == ("per_tick", "wform_ws")
    fc, tfc, tcc = _walk(lambda x, t, tr: s.loop_run_instances(x, t, lp, ctrl=ctrl, plant=plant, trace=tr), st, cmds, T0, T)
    assert pkg.KERNEL_FAMILY[s.query(pkg.QUERY_LAST_KERNEL)] == "wform_ws"
    assert (fc["status"] == 0).all()
    s.close()
    host = _host(pkg)
    sample = np.random.default_rng(1).choice(B, 16, replace=False)
    wf, wx = _against_host(pkg, host, st, cmds, N, lp, None, plant, sample, T0, T, tf, tc, fin)
    print(f"32768 robots, plant records, lane kernel: worst force {wf:.2e} N, state {wx:.2e}")
    assert wf <= 1e-5 and wx <= 1e-7
    wf, wx = _against_host(pkg, host, st, cmds, N, lp, ctrl, plant, sample, T0, T, tfc, tcc, fc)
    print(f"32768 robots, controller + plant records, wave workspace kernel: worst force {wf:.2e} N, state {wx:.2e}")
    assert wf <= 1e-6 and wx <= 1e-8


def test_refusals_and_buffers(pkg, lib, monkeypatch):
    lp = pkg.default_loop_params(lib)
    st = pkg.loop_states([[0.0, 0.0, 0.3, 0.0, 0.0, 0.0, 0.0]] * 4, lp, lib=lib)
    p = pkg.default_params(10, pkg.MODE_CONVERGED, lib)
    ctrl, plant = pkg.instance_params(p, 4), pkg.plant_params(p, 4)

    def code(s, **kw):
        try:
            s.loop_run_instances(st, 3, kw.pop("lp", lp), **kw)
            return pkg.OK
        except pkg.QmpcError as e:
            return e.code

    sc = pkg.Solver(pkg.default_convex_params(20, pkg.MODE_CONVERGED, lib), 4, device=0, lib=lib)
    assert code(sc, plant=plant) == pkg.UNSUPPORTED and code(sc, ctrl=ctrl) == pkg.UNSUPPORTED
    assert sc.loop_instances_plan(4, False, False) is None
    sc.close()
    sr = pkg.Solver(pkg.default_params(10, pkg.MODE_REFERENCE, lib), 4, device=0, lib=lib)
    assert code(sr, plant=plant) == pkg.UNSUPPORTED
    sr.close()
    s8 = pkg.Solver(pkg.default_biped8_params(16, pkg.MODE_CONVERGED, lib), 4, device=0, lib=lib)
    assert code(s8, plant=plant) == pkg.BAD_ARGUMENT
    s8.close()
    s = pkg.Solver(p, 4, device=0, lib=lib)
    warm = pkg.default_loop_params(lib); warm.warm_start = 1.0
    assert code(s, ctrl=ctrl, lp=warm) == pkg.UNSUPPORTED and s.loop_instances_plan(4, True, True) is None
    assert code(s, plant=plant, lp=warm) == pkg.OK
    big = pkg.loop_states([[0.0, 0.0, 0.3, 0.0, 0.0, 0.0, 0.0]] * 5, lp, lib=lib)
    with pytest.raises(pkg.QmpcError) as e:
        s.loop_run_instances(big, 3, lp, plant=pkg.plant_params(p, 5))
    assert e.value.code == pkg.BATCH_TOO_LARGE
    s.close()
    # the buffers: a call with ticks = 0 allocates the per-instance blocks (764 B per robot of max_batch, as
    # qmpc_prepare_instances) and the plant blocks (264 B), launches nothing; later calls allocate nothing
    s = pkg.Solver(p, 1000, device=0, lib=lib)
    s.prepare(4)
    s.loop_run(st, 3, lp)
    before = s.query(pkg.QUERY_DEVICE_BYTES)
    assert _same(s.loop_run_instances(st, 0, lp, ctrl=ctrl, plant=plant), st)
    assert s.query(pkg.QUERY_DEVICE_BYTES) - before == 1028 * 1000
    after = s.query(pkg.QUERY_DEVICE_BYTES)
    s.loop_run_instances(st, 3, lp, ctrl=ctrl, plant=plant)
    assert s.query(pkg.QUERY_DEVICE_BYTES) == after
    s.close()
    s = pkg.Solver(p, 1000, device=0, lib=lib)
    before = s.query(pkg.QUERY_DEVICE_BYTES)
    s.prepare_instances()
    grown = s.query(pkg.QUERY_DEVICE_BYTES) - before
    s.loop_run_instances(st, 0, lp, plant=plant)
    assert grown == 764 * 1000 and s.query(pkg.QUERY_DEVICE_BYTES) - before == 1028 * 1000
    s.close()
    monkeypatch.setenv("QMPC_WFORM", "0")
    s0 = pkg.Solver(p, 4, device=0, lib=lib)
    assert code(s0, ctrl=ctrl) == pkg.UNSUPPORTED and code(s0, plant=plant) == pkg.OK
    s0.close()
