"""GPU suite (-m gpu): motor torque limits and joint torque peaks per robot in the closed loop (qmpc_loop_run_motors*,
include/qmpc.h).

The call is qmpc_loop_run_gaits* in which the foot force a stance leg delivers respects the joint torque limits of the robot's
motors.  +inf limits and motor = None give that call's bytes, with every other record present and with none, in both launch
forms, for both models and on the lane tick, while the tally still records every joint's peak torque; calf limits of 0.6 x a
robot's own unlimited peak on every fourth robot change those robots alone.  The rule is checked tick by tick without the host
class, in both forced launch forms (tests/_loop_motor_worker.py), and against the host class with set_motors beside a delay line
with lag and a binding fz_max.  Device buffers and split calls give one host-buffer call's bytes; an invalid record or tally
freezes its robot alone; refusals and buffers behave as in the gait suite.  Every case is N = 10."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from test_gpu_loop_actuation import (COMMANDS, COUNTERS, FORMS, MODELS, G, _all_same, _binding, _fleet, _mixed, _params, _records, _same, _shoves,
                                     _solver, _standing)
from test_gpu_loop_actuation import lib  # noqa: F401  (the fixture: raises if the HIP extension is missing, no fallback)
from test_gpu_loop_gait import _host_bounds, _mixed_gaits

pytestmark = pytest.mark.gpu

HERE = Path(__file__).resolve().parent
WORKER = HERE / "_loop_motor_worker.py"


@pytest.fixture(scope="module")
def shim():
    import __graft_entry__ as g

    host = C.CDLL(str(g.build_host()))
    vp = C.c_void_p
    host.qh_loop_create_robot.argtypes = [C.c_char_p, C.c_int, vp, vp, vp, vp]
    host.qh_loop_create_robot.restype = vp
    for f in ("qh_loop_tick", "qh_loop_destroy", "qh_loop_device_status"):
        getattr(host, f).argtypes = [vp]
    for f in ("qh_loop_outcome", "qh_loop_export", "qh_loop_set_ground", "qh_loop_ground_tally", "qh_loop_actuation_line", "qh_loop_motor_tally"):
        getattr(host, f).argtypes = [vp, vp]
    host.qh_loop_set_actuation.argtypes = [vp, vp, vp]
    host.qh_loop_set_motors.argtypes = [vp, vp, vp, vp]
    host.qh_loop_set_command.argtypes = [vp, vp, C.c_double]
    return host


def _calf_limits(pkg, free_tally, rows):
    """+inf limits everywhere, but on the robots of `rows` calf limits of 0.6 x that robot's own peak of the unlimited run"""
    motor = pkg.motor_params(len(free_tally))
    for i in np.flatnonzero(rows):
        motor["tau_max"][i, 2::3] = 0.6 * free_tally["peak_tau"][i, 2::3].max()
    return motor


# ---- 1. +inf limits give the gaits call ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,form", FORMS)
@pytest.mark.parametrize("kind", ["both", "neither"])
@pytest.mark.parametrize("model", MODELS)
def test_infinite_limits_give_the_gaits_call(pkg, lib, B, form, kind, model):
    """With +inf limits, and with motor = None, states, outcome records, ground tallies, lines, seen and both traces are the gaits
    call's bytes -- with every other record present and with none of them -- and the motor tally holds a peak torque > 0 for
    every robot and no saturated tick.  With calf limits of 0.6 x its own unlimited peak on every fourth robot those robots alone
    change."""
    T = 20
    p = _params(pkg, lib, model)
    lp, st = _fleet(pkg, lib, B, model=model)
    ctrl, plant = _records(pkg, p, B, kind, model=model)
    op = pkg.default_outcome_params(lib)
    push = _shoves(pkg, lp, B, 40, (3.0, 9.0), (4.0, 5.0))
    ground = _binding(pkg, p, B)
    act, line = _mixed(pkg, p, lp, B)
    sense = pkg.random_go1_senses(B, seed=3)
    sense["bias"][::2], sense["sigma"][::2] = 0.0, 0.0
    gait = _mixed_gaits(pkg, lp, B)
    free_m = pkg.motor_params(B)
    s = _solver(pkg, lib, p, B, model)
    assert s.loop_instances_plan(B, ctrl is not None, False)[0] == form
    kw = dict(gait=gait, sense=sense, act=act, lines=line, ground=ground, push=push, lp=lp, ctrl=ctrl, plant=plant, op=op, trace=True)
    bare_kw = dict(lp=lp, ctrl=ctrl, plant=plant, op=op, trace=True)
    want = s.loop_run_gaits(st, T, gait, sense, None, act, line, ground, push, lp, ctrl=ctrl, plant=plant, op=op, trace=True)
    got = s.loop_run_motors(st, T, free_m, **kw)
    none = s.loop_run_motors(st, T, None, **kw)
    bare_want = s.loop_run_gaits(st, T, None, **bare_kw)
    bare = s.loop_run_motors(st, T, free_m, **bare_kw)
    limited = np.arange(B) % 4 == 1
    some = _calf_limits(pkg, got[5], limited)
    part = s.loop_run_motors(st, T, some, **kw)
    s.close()
    strip = lambda r: r[:5] + r[6:]      # noqa: E731  (without the motor tallies)
    assert (want[0]["tick"] == T).all() and not _same(want[0], bare_want[0])
    assert _all_same(strip(got), want) and _all_same(strip(none), want) and _all_same(strip(bare), bare_want)
    assert _same(none[5], pkg.motor_tallies(B, lib))      # motor = None: the tally is not looked at
    for r in (got, bare):
        mt = r[5]
        assert (mt["peak_tau"].max(axis=1) > 0).all() and (mt["sat_ticks"] == 0).all() and (mt["clipped_ticks"] == 0).all()
        assert (mt["first_clipped_tick"] == -1).all() and (mt["unreachable_leg_ticks"] == 0).all() and np.isfinite(mt["joint_pos"]).all()
    assert all(_same(a[~limited], b[~limited]) for a, b in zip(part[:6], got[:6]))
    assert _same(part[6][:, ~limited], got[6][:, ~limited]) and _same(part[7][:, ~limited], got[7][:, ~limited])
    assert (part[5]["clipped_ticks"][limited] > 0).all() and (part[5]["sat_ticks"][limited][:, 2::3].sum(axis=1) > 0).all()
    assert (part[5]["sat_ticks"][limited][:, 0::3] == 0).all() and (part[5]["sat_ticks"][limited][:, 1::3] == 0).all()
    assert all(part[0][i].tobytes() != got[0][i].tobytes() for i in np.flatnonzero(limited))


def test_identity_on_the_lane_tick_with_uniform_controller_records(pkg, lib):
    """20480 robots under QMPC_INSTANCES_AUTO with uniform controller records, as the gait suite's test of that name: the motor
    call with +inf limits against the gaits call, on the lane kernel -- and calf limits on every fourth robot move that robot
    alone."""
    B, T = 20480, 10
    p, lp, st = _standing(pkg, lib, B, np.linspace(-3, 3, B))
    st["joy"][:, 0] = 0.2
    st["movement_mode"] = 1.0
    cls = np.arange(B) % 4
    ground = pkg.ground_params(B)
    ground["fz_max"][cls == 1] = p.mass * G / 8.0
    ctrl = pkg.instance_params(p, B)
    act = pkg.actuation_params(B, delay_ticks=cls.astype(float))
    op = pkg.default_outcome_params(lib, stop_when_down=True)
    s = _solver(pkg, lib, p, B)
    s.set_instances_policy("auto")
    assert s.loop_instances_plan(B, True, False)[0] == "per_tick" and s.loop_instances_plan(B, True, False)[1].startswith("lane")
    want = s.loop_run_gaits(st, T, None, None, None, act, None, ground, None, lp, ctrl=ctrl, op=op, trace=True)
    got = s.loop_run_motors(st, T, pkg.motor_params(B), act=act, ground=ground, lp=lp, ctrl=ctrl, op=op, trace=True)
    assert pkg.KERNEL_FAMILY[s.query(pkg.QUERY_LAST_KERNEL)].startswith("lane")
    some = _calf_limits(pkg, got[5], cls == 2)
    part = s.loop_run_motors(st, T, some, act=act, ground=ground, lp=lp, ctrl=ctrl, op=op)
    s.close()
    assert _all_same(got[:5] + got[6:], want)
    assert (got[5]["peak_tau"].max(axis=1) > 0).all() and (got[5]["sat_ticks"] == 0).all()
    assert all(_same(a[cls != 2], b[cls != 2]) for a, b in zip(part[:6], got[:6]))
    assert (part[5]["clipped_ticks"][cls == 2] > 0).all()
    assert np.mean([part[0][i].tobytes() != got[0][i].tobytes() for i in np.flatnonzero(cls == 2)]) > 0.9


# ---- 2. the rule, tick by tick ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_rule_tick_by_tick_in_both_launch_forms(model):
    """24 walking robots with mixed gaits and a shove, limits 0.6 x the unlimited peaks per joint type, one tick per call for 40
    ticks, in each forced launch form: the worker asserts the rule after every tick (see its docstring) and prints the worst
    figures; here: the two forms end in the same bytes."""
    out = {}
    for fused in ("0", "1"):
        env = dict(os.environ, QMPC_LOOP_FUSED=fused)
        r = subprocess.run([sys.executable, str(WORKER), "rule", "24", "40", "10", model], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        out[fused] = {l.split(" ", 1)[0]: l.split(" ", 1)[1] for l in r.stdout.splitlines() if l.split(" ", 1)[0] in ("FORM", "WORST", "SHA")}
    print(out)
    assert eval(out["0"]["FORM"])[0] == "per_tick" and eval(out["1"]["FORM"])[0] == "persistent"
    assert out["0"]["SHA"] == out["1"]["SHA"]


# ---- 3. the host class -----------------------------------------------------------------------------------------------------
def test_host_class_with_set_motors(pkg, lib, shim):
    """Six robots, 6 ticks standing and 40 on their commands, with binding limits beside a delay line with lag and a binding
    fz_max, against the host twin with set_motors: schedule fields bit-exact, counters equal, peak_tau to 1e-8 and joint_pos to
    1e-6 (host and device differ through their sincos / acos and the single-precision atan2), the outcome figures within the
    bounds of the actuation, sensing and gait suites' host-class tests."""
    N, T0, T, B = 10, 6, 40, 6
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    lp = pkg.default_loop_params(lib)
    cmds = np.array(COMMANDS)[:B].copy()
    cmds[:, 6] = 1.0
    stand = cmds.copy(); stand[:, 6] = 0.0
    st = pkg.loop_states(stand, lp, height=0.3, yaw=np.linspace(-2, 2, B), lib=lib)
    act = pkg.actuation_params(B, delay_ticks=[0, 1, 2, 0, 1, 3], tau=[0.0, 0.01, 0.01, 0.02, 0.0, 0.01], dt=lp.dt)
    line = pkg.actuation_lines(B, pkg.stand_forces_body(p.mass))
    ground = pkg.ground_params(B)
    ground["fz_max"] = 50.0
    # the stand asks a calf for about 5.5 N m (a quarter of the weight at the knee's lever), the trot for twice that: limits of
    # 4 to 9 N m on the calves bind while standing on some robots and in the trot on all; the thighs bind on the last two
    motor = pkg.motor_params(B, pkg.GO1_TAU_MAX)
    motor["tau_max"][:, 2::3] = np.array([4.0, 5.0, 6.0, 7.0, 8.0, 9.0])[:, None]
    motor["tau_max"][4:, 1::3] = 2.0
    s = pkg.Solver(p, B, device=0, lib=lib)
    x, oc, ta, li, sn, mt = s.loop_run_motors(st, T0, motor, act=act, lines=line, ground=ground, lp=lp)
    x["movement_mode"] = cmds[:, 6]
    fin, oc, ta, li, sn, mt = s.loop_run_motors(x, T, motor, mt, act=act, lines=li, ground=ground, lp=lp, outcomes=oc, tallies=ta)
    s.close()
    ho, hs = pkg.loop_outcomes(B, lib), np.zeros(B, dtype=pkg.LOOP_STATE_DTYPE)
    ht, hm, hl = pkg.ground_tallies(B), pkg.motor_tallies(B, lib), pkg.actuation_lines(B)
    mt0 = pkg.motor_tallies(B, lib)
    for i in range(B):
        h = shim.qh_loop_create_robot(str(pkg.LIB_PATH).encode(), N, C.addressof(lp), st[i:i + 1].ctypes.data, None, None)
        assert h and shim.qh_loop_device_status(h) == 0
        shim.qh_loop_set_ground(h, ground[i:i + 1].ctypes.data)
        shim.qh_loop_set_actuation(h, act[i:i + 1].ctypes.data, line[i:i + 1].ctypes.data)
        shim.qh_loop_set_motors(h, None, motor[i:i + 1].ctypes.data, mt0[i:i + 1].ctypes.data)
        for _ in range(T0):
            assert shim.qh_loop_tick(h) == 1
        shim.qh_loop_set_command(h, np.ascontiguousarray(cmds[i, :6]).ctypes.data, float(cmds[i, 6]))
        for t in range(T):
            assert shim.qh_loop_tick(h) == 1, (i, t)
        shim.qh_loop_outcome(h, ho[i:i + 1].ctypes.data)
        shim.qh_loop_export(h, hs[i:i + 1].ctypes.data)
        shim.qh_loop_ground_tally(h, ht[i:i + 1].ctypes.data)
        shim.qh_loop_motor_tally(h, hm[i:i + 1].ctypes.data)
        shim.qh_loop_actuation_line(h, hl[i:i + 1].ctypes.data)
        shim.qh_loop_destroy(h)
    assert np.isin(fin["status"], (pkg.OK, pkg.MAX_ITER)).all() and (fin["contacts"] == 0).any()
    assert (mt["clipped_ticks"] > 0).all() and (mt["sat_ticks"][:, 2::3].sum(axis=1) > 0).all() and (mt["sat_ticks"][4:, 1::3].sum(axis=1) > 0).all()
    assert (ta["clipped_ticks"] > 0).any() and (mt["unreachable_leg_ticks"] == 0).all()
    for k in ("sat_ticks", "clipped_ticks", "first_clipped_tick", "unreachable_leg_ticks"):
        assert np.array_equal(mt[k], hm[k]), (k, mt[k], hm[k])
    for k in ("clipped_ticks", "first_clipped_tick", "friction_leg_ticks", "normal_leg_ticks"):
        assert np.array_equal(ta[k], ht[k]), k
    assert np.array_equal(li["count"], hl["count"])
    worst_peak, worst_q = float(np.abs(mt["peak_tau"] - hm["peak_tau"]).max()), float(np.abs(mt["joint_pos"] - hm["joint_pos"]).max())
    print("device against host: peak_tau", worst_peak, "joint_pos", worst_q)
    assert worst_peak <= 1e-8 and worst_q <= 1e-6
    _host_bounds(fin, oc, hs, ho, T0 + T)


# ---- 4. device buffers, calls split ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_device_buffers_and_split_calls_give_the_host_call(pkg, lib, model):
    """48 robots with binding limits, 30 ticks: device buffers give the host-buffer call's bytes, calls of 1, 10, 6 and 13 ticks
    that hand on states, tallies and lines give one call's, and the records are read in place."""
    import torch

    B, T = 48, 30
    p = _params(pkg, lib, model)
    lp, st = _fleet(pkg, lib, B, seed=6, model=model)
    ctrl, plant = _records(pkg, p, B, "both", seed=2, model=model)
    push = _shoves(pkg, lp, B, 43, (2.0, 6.0, 15.0), (5.0, 3.0, 6.0))
    ground = _binding(pkg, p, B)
    act, line = _mixed(pkg, p, lp, B)
    sense = pkg.random_go1_senses(B, seed=9)
    gait = _mixed_gaits(pkg, lp, B)
    motor = pkg.random_go1_motors(B, seed=5, scale=(0.15, 0.6))
    op = pkg.default_outcome_params(lib, stop_when_down=True)
    s = _solver(pkg, lib, p, B, model)
    run = lambda x, t, li, sn=None, oc=None, ta=None, mt=None: s.loop_run_motors(      # noqa: E731
        x, t, motor, mt, gait=gait, sense=sense, seen=sn, act=act, lines=li, ground=ground, push=push, lp=lp, ctrl=ctrl, plant=plant, op=op,
        outcomes=oc, tallies=ta, trace=True)
    want = run(st, T, line)
    assert (want[5]["clipped_ticks"] > 0).mean() > 0.5
    parts, x = [], (st, None, None, line, None, None)
    for n in (1, 10, 6, T - 17):
        x = run(x[0], n, x[3], x[4], x[1], x[2], x[5])
        parts.append(x)
    assert _all_same(want[:6], x[:6])
    assert _same(want[6], np.concatenate([q[6] for q in parts])) and _same(want[7], np.concatenate([q[7] for q in parts]))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1).copy()).cuda()      # noqa: E731
    d_st, d_oc, d_ta, d_ctrl, d_plant = dev(st), dev(pkg.loop_outcomes(B, lib)), dev(pkg.ground_tallies(B)), dev(ctrl), dev(plant)
    d_push, d_ground, d_act, d_line, d_sense, d_seen, d_gait = dev(push), dev(ground), dev(act), dev(line), dev(sense), dev(pkg.sense_seen(B)), dev(gait)
    d_motor, d_mt = dev(motor), dev(pkg.motor_tallies(B, lib))
    d_tf = torch.full((T, B, 12), 7.0, dtype=torch.float64, device="cuda")
    d_tc = torch.full((T, B, 4), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s.loop_run_motors_device(B, d_st.data_ptr(), T, d_oc.data_ptr(), d_motor.data_ptr(), d_mt.data_ptr(), None, d_gait.data_ptr(), d_sense.data_ptr(),
                             d_seen.data_ptr(), d_act.data_ptr(), d_line.data_ptr(), d_ground.data_ptr(), d_ta.data_ptr(), d_push.data_ptr(), 3, lp,
                             op, d_ctrl=d_ctrl.data_ptr(), d_plant=d_plant.data_ptr(), d_trace_forces=d_tf.data_ptr(),
                             d_trace_contacts=d_tc.data_ptr())
    s.wait()
    s.close()
    assert d_st.cpu().numpy().tobytes() == want[0].tobytes() and d_oc.cpu().numpy().tobytes() == want[1].tobytes()
    assert d_ta.cpu().numpy().tobytes() == want[2].tobytes() and d_line.cpu().numpy().tobytes() == want[3].tobytes()
    assert d_seen.cpu().numpy().tobytes() == want[4].tobytes() and d_mt.cpu().numpy().tobytes() == want[5].tobytes()
    assert _same(d_tf.cpu().numpy(), want[6]) and _same(d_tc.cpu().numpy(), want[7])
    assert d_motor.cpu().numpy().tobytes() == motor.tobytes() and d_gait.cpu().numpy().tobytes() == gait.tobytes()      # read in place


# ---- 5. refusals and buffers -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,form", FORMS)
def test_an_invalid_record_freezes_its_robot_alone(pkg, lib, B, form):
    T = 6
    p = pkg.default_params(10, pkg.MODE_CONVERGED, lib)
    lp, st = _fleet(pkg, lib, B, seed=9)
    ground = _binding(pkg, p, B)
    act, line = _mixed(pkg, p, lp, B)
    gait = _mixed_gaits(pkg, lp, B)
    # 2 N m on every joint binds from the first tick: a quarter of the weight (31 N) at the stand pose's knee lever,
    # 0.213 m sin(1.3 - 0.67), asks a calf for 3.9 N m
    motor = pkg.motor_params(B, 2.0)
    mt0 = pkg.motor_tallies(B, lib)
    bad_motor, bad_mt = motor.copy(), mt0.copy()
    cases = ([("m", "tau_max", c, v) for c, v in ((0, np.nan), (4, 0.0), (8, -3.0), (11, -np.inf))] + [("m", "reserved", c, 1.0) for c in range(4)]
             + [("t", "joint_pos", 5, np.nan), ("t", "joint_pos", 0, np.inf), ("t", "sat_ticks", 3, 0.5), ("t", "sat_ticks", 9, -1.0),
                ("t", "clipped_ticks", None, 1.5), ("t", "unreachable_leg_ticks", None, 2.0 ** 53)])
    for i, (which, k, c, v) in enumerate(cases):
        rec = bad_motor if which == "m" else bad_mt
        if c is None:
            rec[k][i] = v
        else:
            rec[k][i, c] = v
    bad = np.zeros(B, dtype=bool)
    bad[:len(cases)] = True
    op = pkg.default_outcome_params(lib)
    oc0, ta0 = pkg.loop_outcomes(B, lib), pkg.ground_tallies(B)
    s = _solver(pkg, lib, p, B)
    assert s.loop_instances_plan(B, False, False)[0] == form
    kw = dict(gait=gait, act=act, lines=line, ground=ground, lp=lp, op=op, trace=True)
    ref = s.loop_run_motors(st, T, motor, mt0, **kw)
    got = s.loop_run_motors(st, T, bad_motor, bad_mt, **kw)
    s.close()
    x, oc, ta, li, sn, mt, tf, tc = got
    frozen = st[bad].copy()
    frozen["status"], frozen["iterations"] = pkg.BAD_PARAMS, 0
    assert _same(x[bad], frozen) and (tf[:, bad] == 0).all() and (tc[:, bad] == 0).all()
    assert _same(oc[bad], oc0[bad]) and _same(ta[bad], ta0[bad]) and _same(li[bad], line[bad]) and _same(mt[bad], bad_mt[bad])
    assert all(_same(a[~bad], b[~bad]) for a, b in zip(got[:6], ref[:6])) and _same(tf[:, ~bad], ref[6][:, ~bad]) and _same(tc[:, ~bad], ref[7][:, ~bad])
    assert (ref[0]["tick"] == T).all() and (ref[5]["clipped_ticks"] > 0).any()


def test_refusals_and_buffers(pkg, lib):
    lp = pkg.default_loop_params(lib)
    st = pkg.loop_states([[0.0, 0.0, 0.3, 0.0, 0.0, 0.0, 0.0]] * 4, lp, lib=lib)
    p = pkg.default_params(10, pkg.MODE_CONVERGED, lib)
    ctrl, plant = pkg.instance_params(p, 4), pkg.plant_params(p, 4)
    ground = pkg.ground_params(4)
    ground["mu"] = 0.4
    act = pkg.actuation_params(4, 2, 0.01)
    sense = pkg.sense_params(4, seed=1, gyro_bias=0.01, pos_noise=0.003)
    gait = pkg.gait_params(4, ["pace", "crawl", "trot", "amble"], gait_freq=2.0)
    motor = pkg.motor_params(4, 4.0)

    def code(s, mo=motor, ga=gait, se=sense, a=act, g=ground, pu=None, **kw):
        try:
            s.loop_run_motors(kw.pop("st", st), 3, mo, None, None, ga, se, None, a, None, g, pu, kw.pop("lp", lp), **kw)
            return pkg.OK
        except pkg.QmpcError as e:
            return e.code

    sr = pkg.Solver(pkg.default_params(10, pkg.MODE_REFERENCE, lib), 4, device=0, lib=lib)
    assert code(sr, plant=plant) == pkg.UNSUPPORTED and code(sr) == pkg.UNSUPPORTED and code(sr, ga=None, se=None, a=None, g=None) == pkg.UNSUPPORTED
    sr.close()
    s8 = pkg.Solver(pkg.default_biped8_params(16, pkg.MODE_CONVERGED, lib), 4, device=0, lib=lib)
    assert code(s8, plant=plant) == pkg.BAD_ARGUMENT and code(s8) == pkg.BAD_ARGUMENT
    s8.close()
    pc = pkg.default_convex_params(10, pkg.MODE_CONVERGED, lib)      # a ConvexMpc handle that did not opt in is refused
    sc = pkg.Solver(pc, 4, device=0, lib=lib)
    for kw in ({}, {"plant": pkg.plant_params(pc, 4)}, {"ga": None, "se": None, "a": None, "g": None}):
        assert code(sc, **kw) == pkg.UNSUPPORTED, kw
    sc.set_convex_records(True)
    assert code(sc) == pkg.OK and code(sc, ga=None, se=None, a=None, g=None) == pkg.OK
    sc.close()
    s = pkg.Solver(p, 4, device=0, lib=lib)
    assert code(s) == pkg.OK and code(s, ctrl=ctrl) == pkg.OK and code(s, ga=None, se=None, a=None, g=None) == pkg.OK
    assert code(s, want_motor_tallies=False) == pkg.BAD_ARGUMENT      # motor without a tally
    big = pkg.loop_states([[0.0, 0.0, 0.3, 0.0, 0.0, 0.0, 0.0]] * 5, lp, lib=lib)
    assert code(s, st=big, mo=pkg.motor_params(5), ga=None, g=None, a=None, se=None) == pkg.BATCH_TOO_LARGE
    s.close()
    # buffers: the host-buffer motor call stages records and tallies in a buffer of its own ((128 + 320) B x max_batch), allocated
    # by ticks = 0 too; no other call allocates it, a call with motor = None is the gaits call
    s = pkg.Solver(p, 1000, device=0, lib=lib)
    s.prepare(4)
    s.loop_run(st, 3, lp)
    kw = dict(gait=gait, sense=sense, act=act, ground=ground, push=pkg.push_params(4, 2), lp=lp, ctrl=ctrl, plant=plant)
    s.loop_run_gaits(st, 3, gait, sense, None, act, None, ground, pkg.push_params(4, 2), lp, ctrl=ctrl, plant=plant)
    before = s.query(pkg.QUERY_DEVICE_BYTES)
    s.loop_run_motors(st, 3, None, **kw)
    assert s.query(pkg.QUERY_DEVICE_BYTES) == before
    s.loop_run_motors(st, 0, motor, **kw)
    first = s.query(pkg.QUERY_DEVICE_BYTES)
    got = s.loop_run_motors(st, 0, motor, trace=True, **kw)
    assert _same(got[0], st) and _same(got[1], pkg.loop_outcomes(4, lib)) and _same(got[5], pkg.motor_tallies(4, lib))      # nothing was launched
    assert first - before == 448 * 1000 and s.query(pkg.QUERY_DEVICE_BYTES) == first
    s.loop_run_motors(st, 3, motor, lp=lp, plant=plant)
    s.loop_run_gaits(st, 3, gait, sense, None, act, None, ground, pkg.push_params(4, 2), lp, ctrl=ctrl, plant=plant)
    s.loop_run_instances(st, 3, lp, ctrl=ctrl, plant=plant)
    assert s.query(pkg.QUERY_DEVICE_BYTES) - before == 448 * 1000
    s.close()
    # ... on the first host-buffer call with motor, whichever it is: here one with ticks > 0 on a handle that made a push call
    s = pkg.Solver(p, 1000, device=0, lib=lib)
    s.prepare(4)
    s.loop_run_pushes(st, 3, pkg.push_params(4, 2), lp, ctrl=ctrl, plant=plant)
    before = s.query(pkg.QUERY_DEVICE_BYTES)
    s.loop_run_motors(st, 3, motor, push=pkg.push_params(4, 2), lp=lp, ctrl=ctrl, plant=plant)
    assert s.query(pkg.QUERY_DEVICE_BYTES) - before == 448 * 1000
    s.close()
