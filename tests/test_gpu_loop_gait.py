"""GPU suite (-m gpu): gait frequency and contact pattern per robot in the closed loop (qmpc_loop_run_gaits*, include/qmpc.h;
DESIGN.md section 3x).

The call is qmpc_loop_run_sensing* in which every robot walks its own gait.  Identity records and gait = None give that call's
bytes, with every other record present and with none, in both launch forms, for both models and on the lane tick; one robot in
four on the pace changes those robots alone.  The schedule fields read back after every tick equal, bit for bit, the FSM restated
in Python floats (tests/test_loop_gait_cpu.py: Leg) driven by the contact flags of the state before the tick, for the six named
gaits at 1.7 / 2.2 / 3.0 Hz, in both forced launch forms and for both models (tests/_loop_gait_worker.py).  The host class with
set_gait agrees with the device: schedule fields bit-exact, outcome figures within the bounds of the actuation and sensing
suites' host-class tests.  Launch forms, device buffers and calls split give the same bytes; qmpc_loop_state_set_gait starts the
legs in their pattern's state; an invalid record freezes its robot alone; refusals and buffers behave as in the sensing suite.
Every case is N = 10; the schedule test walks 70 ticks -- the crawl's cycle at 3 Hz is 67 ticks, and it must reach all four of
its three-leg sets."""
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
from test_loop_gait_cpu import FREQS, SCHEDULE, TABLE, Leg

pytestmark = pytest.mark.gpu

HERE = Path(__file__).resolve().parent
WORKER = HERE / "_loop_gait_worker.py"
TWO_LEG = {"pace": {(1, 0, 1, 0), (0, 1, 0, 1)}, "bound": {(1, 1, 0, 0), (0, 0, 1, 1)}, "trot": {(1, 0, 0, 1), (0, 1, 1, 0)}}
THREE_LEG = {(0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)}


@pytest.fixture(scope="module")
def shim():
    import __graft_entry__ as g

    host = C.CDLL(str(g.build_host()))
    vp = C.c_void_p
    host.qh_loop_create_robot.argtypes = [C.c_char_p, C.c_int, vp, vp, vp, vp]
    host.qh_loop_create_robot.restype = vp
    for f in ("qh_loop_tick", "qh_loop_destroy", "qh_loop_device_status"):
        getattr(host, f).argtypes = [vp]
    for f in ("qh_loop_outcome", "qh_loop_export", "qh_loop_set_ground", "qh_loop_ground_tally", "qh_loop_actuation_line", "qh_loop_set_sense",
              "qh_loop_sense_seen", "qh_loop_set_gait"):
        getattr(host, f).argtypes = [vp, vp]
    host.qh_loop_set_actuation.argtypes = [vp, vp, vp]
    host.qh_loop_set_pushes.argtypes = [vp, vp, C.c_int]
    host.qh_loop_set_command.argtypes = [vp, vp, C.c_double]
    return host


def _mixed_gaits(pkg, lp, B):
    """gait records by i mod 7: the identity, then the six named gaits, at 1.7 / 2.2 / 3.0 Hz by i mod 3"""
    k = np.arange(B) % 7
    names = ["trot" if q == 0 else list(TABLE)[q - 1] for q in k]
    return pkg.gait_params(B, names, gait_freq=np.where(k == 0, lp.gait_freq, np.array(FREQS)[np.arange(B) % 3]))


def _sched(x):
    return np.stack([x["leg"][k] for k in SCHEDULE], axis=-1)


# ---- 1. identity records give the sensing call -----------------------------------------------------------------------------
@pytest.mark.parametrize("B,form", FORMS)
@pytest.mark.parametrize("kind", ["both", "neither"])
@pytest.mark.parametrize("model", MODELS)
def test_identity_records_give_the_sensing_call(pkg, lib, B, form, kind, model):
    """With identity records, and with gait = None, states, outcome records, tallies, lines, seen and both traces are the sensing
    call's bytes -- with every other record present and with none of them.  With every fourth robot on the pace at 3 Hz those
    robots alone change."""
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
    ident = pkg.gait_params(B, lp=lp)
    some = ident.copy()
    paced = np.arange(B) % 4 == 1
    some[paced] = pkg.gait_params(int(paced.sum()), "pace", gait_freq=3.0)
    st[paced] = pkg.loop_states_set_gait(st[paced], some[paced], lib)      # those robots start on the pace's first two legs
    s = _solver(pkg, lib, p, B, model)
    assert s.loop_instances_plan(B, ctrl is not None, False)[0] == form
    want = s.loop_run_sensing(st, T, sense, None, act, line, ground, push, lp, ctrl=ctrl, plant=plant, op=op, trace=True)
    got = s.loop_run_gaits(st, T, ident, sense, None, act, line, ground, push, lp, ctrl=ctrl, plant=plant, op=op, trace=True)
    none = s.loop_run_gaits(st, T, None, sense, None, act, line, ground, push, lp, ctrl=ctrl, plant=plant, op=op, trace=True)
    bare_want = s.loop_run_sensing(st, T, None, None, None, None, None, None, lp, ctrl=ctrl, plant=plant, op=op, trace=True)
    bare = s.loop_run_gaits(st, T, ident, None, None, None, None, None, None, lp, ctrl=ctrl, plant=plant, op=op, trace=True)
    part = s.loop_run_gaits(st, T, some, sense, None, act, line, ground, push, lp, ctrl=ctrl, plant=plant, op=op, trace=True)
    s.close()
    assert (want[0]["tick"] == T).all() and not _same(want[0], bare_want[0])
    assert _all_same(got, want) and _all_same(none, want) and _all_same(bare, bare_want)
    walking = st["movement_mode"] != 0
    assert all(_same(a[~paced], b[~paced]) for a, b in zip(part[:5], want[:5])) and _same(part[5][:, ~paced], want[5][:, ~paced])
    assert np.mean([part[0][i].tobytes() != want[0][i].tobytes() for i in np.flatnonzero(paced & walking)]) > 0.95
    assert (part[6][:, paced & walking].reshape(-1, 4)[:, None, :] == np.array(sorted(TWO_LEG["pace"]))[None]).all(axis=2).any()


def test_identity_on_the_lane_tick_with_uniform_controller_records(pkg, lib):
    """20480 robots under QMPC_INSTANCES_AUTO with uniform controller records, as the sensing suite's test of that name: the gait
    call with identity records against the sensing call, on the lane kernel -- and the pace on every fourth robot moves that robot
    alone (it fills other stance-sort classes of the lane tick)."""
    B, T = 20480, 10
    p, lp, st = _standing(pkg, lib, B, np.linspace(-3, 3, B))
    st["joy"][:, 0] = 0.2
    st["movement_mode"] = 1.0
    cls = np.arange(B) % 4
    pace = pkg.gait_params(int((cls == 2).sum()), "pace", gait_freq=3.0)
    st[cls == 2] = pkg.loop_states_set_gait(st[cls == 2], pace, lib)      # those robots start on two legs
    ground = pkg.ground_params(B)
    ground["fz_max"][cls == 1] = p.mass * G / 8.0
    ctrl = pkg.instance_params(p, B)
    act = pkg.actuation_params(B, delay_ticks=cls.astype(float))
    op = pkg.default_outcome_params(lib, stop_when_down=True)
    some = pkg.gait_params(B, lp=lp)
    some[cls == 2] = pace
    s = _solver(pkg, lib, p, B)
    s.set_instances_policy("auto")
    assert s.loop_instances_plan(B, True, False)[0] == "per_tick" and s.loop_instances_plan(B, True, False)[1].startswith("lane")
    want = s.loop_run_sensing(st, T, None, None, act, None, ground, None, lp, ctrl=ctrl, op=op, trace=True)
    got = s.loop_run_gaits(st, T, pkg.gait_params(B, lp=lp), None, None, act, None, ground, None, lp, ctrl=ctrl, op=op, trace=True)
    assert pkg.KERNEL_FAMILY[s.query(pkg.QUERY_LAST_KERNEL)].startswith("lane")
    part = s.loop_run_gaits(st, T, some, None, None, act, None, ground, None, lp, ctrl=ctrl, op=op)
    s.close()
    assert _all_same(got, want)
    assert _same(part[0][cls != 2], want[0][cls != 2])
    assert np.mean([part[0][i].tobytes() != want[0][i].tobytes() for i in np.flatnonzero(cls == 2)]) > 0.9
    assert {tuple(int(c) for c in r) for r in part[0]["contacts"][cls == 2]} == {(1, 0, 1, 0)}


# ---- 2. the schedule -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_schedule_equals_the_python_fsm_in_both_launch_forms(model):
    """The six gaits x three frequencies, one tick per call for 70 ticks, in each forced launch form: the worker asserts the
    schedule fields, contacts and gait_counter against the Python FSM after every tick and that every status is OK or MAX_ITER;
    here: the two forms end in the same bytes, pace and bound reach their two-leg sets, the crawl all four three-leg sets and
    never fewer than three legs."""
    out = {}
    for fused in ("0", "1"):
        env = dict(os.environ, QMPC_LOOP_FUSED=fused)
        r = subprocess.run([sys.executable, str(WORKER), "schedule", "18", "70", "10", model], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        out[fused] = {l.split(" ", 1)[0]: l.split(" ", 1)[1] for l in r.stdout.splitlines() if l.split(" ", 1)[0] in ("FORM", "SETS", "SHA")}
    print(out)
    assert eval(out["0"]["FORM"])[0] == "per_tick" and eval(out["1"]["FORM"])[0] == "persistent"
    assert out["0"]["SHA"] == out["1"]["SHA"] and out["0"]["SETS"] == out["1"]["SETS"]
    sets = {n: set(v) for n, v in eval(out["0"]["SETS"]).items()}
    for n in ("pace", "bound", "trot"):
        assert TWO_LEG[n] <= sets[n], (n, sets[n])
    assert THREE_LEG <= sets["crawl"] and min(sum(c) for c in sets["crawl"]) == 3
    assert all(min(sum(c) for c in v) >= 2 for v in sets.values())


# ---- 3. the host class -----------------------------------------------------------------------------------------------------
def _host_run(shim, pkg, lib, N, lp, st, cmds, T0, T, gait, push=None, ground=None, act=None, line=None, sense=None):
    B = len(st)
    ho, hs = pkg.loop_outcomes(B, lib), np.zeros(B, dtype=pkg.LOOP_STATE_DTYPE)
    for i in range(B):
        h = shim.qh_loop_create_robot(str(pkg.LIB_PATH).encode(), N, C.addressof(lp), st[i:i + 1].ctypes.data, None, None)
        assert h and shim.qh_loop_device_status(h) == 0
        if push is not None:
            shim.qh_loop_set_pushes(h, push[i].ctypes.data, push.shape[1])
        if ground is not None:
            shim.qh_loop_set_ground(h, ground[i:i + 1].ctypes.data)
        if act is not None:
            shim.qh_loop_set_actuation(h, act[i:i + 1].ctypes.data, line[i:i + 1].ctypes.data)
        if sense is not None:
            shim.qh_loop_set_sense(h, sense[i:i + 1].ctypes.data)
        shim.qh_loop_set_gait(h, gait[i:i + 1].ctypes.data)
        for _ in range(T0):
            assert shim.qh_loop_tick(h) == 1
        shim.qh_loop_set_command(h, np.ascontiguousarray(cmds[i, :6]).ctypes.data, float(cmds[i, 6]))
        for t in range(T):
            assert shim.qh_loop_tick(h) == 1, (i, t)
        shim.qh_loop_outcome(h, ho[i:i + 1].ctypes.data)
        shim.qh_loop_export(h, hs[i:i + 1].ctypes.data)
        shim.qh_loop_destroy(h)
    return hs, ho


def _host_bounds(fin, oc, hs, ho, ticks):
    """the bounds of test_host_class_behind_delay_and_lag / test_host_class_with_a_sensing_record, and the schedule bit for bit"""
    assert _same(_sched(fin), _sched(hs)) and _same(fin["contacts"], hs["contacts"]) and _same(fin["gait_counter"], hs["gait_counter"])
    for k in COUNTERS:
        assert np.array_equal(oc[k], ho[k]), k
    worst = {k: float(np.abs(oc[k] - ho[k]).max()) for k in ("min_height", "min_upright", "max_height_err", "max_vel_err", "max_ang_vel",
                                                            "max_force_z", "sum_vel_err_sq")}
    worst_state = {k: float(np.abs(fin[k] - hs[k]).max()) for k in ("pos_world", "quat", "lin_vel_world", "ang_vel_body", "grf_world",
                                                                    "forces_body", "foot_target_world", "foot_pos_world")}
    print("device against host, worst differences:", worst, "final states:", worst_state)
    for k in ("min_height", "min_upright", "max_height_err", "max_vel_err", "max_ang_vel"):
        assert worst[k] <= 1e-8, (k, worst)
    assert worst["max_force_z"] <= 1e-6
    assert (np.abs(oc["sum_vel_err_sq"] - ho["sum_vel_err_sq"]) <= oc["ticks"] * 2 * oc["max_vel_err"] * 1e-8).all()
    assert (fin["tick"] == ticks).all() and (oc["ticks"][oc["down_tick"] < 0] == ticks).all()
    # the targets at the bound those suites put on the plant's figures (the final states themselves are printed, as there)
    assert worst_state["foot_target_world"] <= 1e-8, worst_state


def test_host_class_with_set_gait(pkg, lib, shim):
    """Six robots, 6 ticks standing (the reset runs every tick: the legs sit at their starting phases) and 40 on their commands, a
    shove on robot 1: crawl, pace and trot_overlap at 3.0 and 2.2 Hz, against the host twin with set_gait."""
    N, T0, T, B = 10, 6, 40, 6
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    lp = pkg.default_loop_params(lib)
    cmds = np.array(COMMANDS)[:B].copy()
    cmds[:, 6] = 1.0
    stand = cmds.copy(); stand[:, 6] = 0.0
    st = pkg.loop_states(stand, lp, height=0.3, yaw=np.linspace(-2, 2, B), lib=lib)
    gait = pkg.gait_params(B, ["crawl", "pace", "trot_overlap"] * 2, gait_freq=[3.0, 3.0, 3.0, 2.2, 2.2, 2.2])
    push = pkg.push_params(B, 2)
    push[1, 0] = (20.0, 6.0, [0.0, 30.0, 0.0], [0.0, 0.0, 0.0])
    s = pkg.Solver(p, B, device=0, lib=lib)
    x, oc, *_ = s.loop_run_gaits(st, T0, gait, push=push, lp=lp)
    for i in range(B):      # standing: every leg at its starting phase, in its pattern's state
        for l in range(4):
            want = Leg(*(TABLE[["crawl", "pace", "trot_overlap"][i % 3]][k][l] for k in range(3)))
            assert tuple(float(x["leg"][i, l][k]) for k in SCHEDULE) == want.fields() and x["contacts"][i, l] == 1.0
    x["movement_mode"] = cmds[:, 6]
    fin, oc, *_ = s.loop_run_gaits(x, T, gait, push=push, lp=lp, outcomes=oc)
    s.close()
    hs, ho = _host_run(shim, pkg, lib, N, lp, st, cmds, T0, T, gait, push=push)
    assert np.isin(fin["status"], (pkg.OK, pkg.MAX_ITER)).all() and (fin["contacts"] == 0).any()
    _host_bounds(fin, oc, hs, ho, T0 + T)


def test_composition_with_sensing_delay_line_and_binding_ground(pkg, lib, shim):
    """Crawl robots at three frequencies with a sensing bias, behind a delay line with a lag, on ground that binds, walking from
    tick 0 from qmpc_loop_state_set_gait, three ticks of one call each, against the host class."""
    N, B = 10, 3
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    lp = pkg.default_loop_params(lib)
    cmds = np.tile([0.2, 0.05, 0.30, 0.0, 0.0, 0.2, 1.0], (B, 1))
    gait = pkg.gait_params(B, "crawl", gait_freq=list(FREQS))
    st = pkg.loop_states_set_gait(pkg.loop_states(cmds, lp, height=0.3, yaw=[-1.0, 0.3, 2.0], lib=lib), gait, lib)
    sense = pkg.sense_params(B, gyro_bias=[0.03, -0.02, 0.04], pos_bias=[0.01, -0.015, 0.008])
    act = pkg.actuation_params(B, delay_ticks=[1, 2, 1], tau=[0.0, 0.01, 0.01], dt=lp.dt)
    line = pkg.actuation_lines(B, pkg.stand_forces_body(p.mass) * 1.3)
    ground = pkg.ground_params(B)
    ground["fz_max"] = 30.0
    s = pkg.Solver(p, B, device=0, lib=lib)
    x, oc, ta, li, sn = st, None, None, line, None
    for _ in range(3):
        x, oc, ta, li, sn = s.loop_run_gaits(x, 1, gait, sense, sn, act, li, ground, None, lp, outcomes=oc, tallies=ta)
    s.close()
    assert (ta["clipped_ticks"] > 0).all() and (sn["ticks"] == 3).all() and (x["contacts"].sum(axis=1) == 3).all()
    hs, ho = _host_run(shim, pkg, lib, N, lp, st, cmds, 0, 3, gait, ground=ground, act=act, line=line, sense=sense)
    _host_bounds(x, oc, hs, ho, 3)


# ---- 4. launch forms, device buffers, calls split --------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_launch_forms_give_the_same_bytes(model):
    out = {}
    for fused in ("0", "1"):
        env = dict(os.environ, QMPC_LOOP_FUSED=fused)
        r = subprocess.run([sys.executable, str(WORKER), "fleet", "64", "40", "10", model], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.splitlines()
        out[fused] = tuple([l for l in lines if l.startswith(k)][0] for k in ("FORM", "OUTCOMES", "SHA"))
    print(out)
    f0, f1 = eval(out["0"][0][5:]), eval(out["1"][0][5:])
    assert f0[0] == "per_tick" and f1[0] == "persistent"
    assert out["0"][1] == out["1"][1] and out["0"][2] == out["1"][2]


@pytest.mark.parametrize("model", MODELS)
def test_device_buffers_and_split_calls_give_the_host_call(pkg, lib, model):
    """48 robots with mixed gaits, 30 ticks: device buffers give the host-buffer call's bytes (with every record, and with the gait
    record alone), and calls of 1, 10, 6 and 13 ticks that hand on states and records give one call's."""
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
    op = pkg.default_outcome_params(lib, stop_when_down=True)
    s = _solver(pkg, lib, p, B, model)
    run = lambda x, t, li, sn=None, oc=None, ta=None: s.loop_run_gaits(x, t, gait, sense, sn, act, li, ground, push, lp, ctrl=ctrl, plant=plant,      # noqa: E731
                                                                       op=op, outcomes=oc, tallies=ta, trace=True)
    want = run(st, T, line)
    parts, x = [], (st, None, None, line, None)
    for n in (1, 10, 6, T - 17):
        x = run(x[0], n, x[3], x[4], x[1], x[2])
        parts.append(x)
    assert _all_same(want[:5], x[:5])
    assert _same(want[5], np.concatenate([q[5] for q in parts])) and _same(want[6], np.concatenate([q[6] for q in parts]))
    bare = s.loop_run_gaits(st, T, gait, lp=lp, plant=plant, op=op)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1).copy()).cuda()      # noqa: E731
    d_st, d_oc, d_ta, d_ctrl, d_plant = dev(st), dev(pkg.loop_outcomes(B, lib)), dev(pkg.ground_tallies(B)), dev(ctrl), dev(plant)
    d_push, d_ground, d_act, d_line, d_sense, d_seen, d_gait = dev(push), dev(ground), dev(act), dev(line), dev(sense), dev(pkg.sense_seen(B)), dev(gait)
    d_tf = torch.full((T, B, 12), 7.0, dtype=torch.float64, device="cuda")
    d_tc = torch.full((T, B, 4), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s.loop_run_gaits_device(B, d_st.data_ptr(), T, d_oc.data_ptr(), d_gait.data_ptr(), d_sense.data_ptr(), d_seen.data_ptr(), d_act.data_ptr(),
                            d_line.data_ptr(), d_ground.data_ptr(), d_ta.data_ptr(), d_push.data_ptr(), 3, lp, op, d_ctrl=d_ctrl.data_ptr(),
                            d_plant=d_plant.data_ptr(), d_trace_forces=d_tf.data_ptr(), d_trace_contacts=d_tc.data_ptr())
    s.wait()
    d_st2, d_oc2 = dev(st), dev(pkg.loop_outcomes(B, lib))      # ... and with the gait record alone, from the start again
    torch.cuda.synchronize()
    s.loop_run_gaits_device(B, d_st2.data_ptr(), T, d_oc2.data_ptr(), d_gait.data_ptr(), lp=lp, op=op, d_plant=d_plant.data_ptr())
    s.wait()
    s.close()
    assert d_st.cpu().numpy().tobytes() == want[0].tobytes() and d_oc.cpu().numpy().tobytes() == want[1].tobytes()
    assert d_ta.cpu().numpy().tobytes() == want[2].tobytes() and d_line.cpu().numpy().tobytes() == want[3].tobytes()
    assert d_seen.cpu().numpy().tobytes() == want[4].tobytes()
    assert _same(d_tf.cpu().numpy(), want[5]) and _same(d_tc.cpu().numpy(), want[6])
    assert d_gait.cpu().numpy().tobytes() == gait.tobytes()      # read in place
    assert d_st2.cpu().numpy().tobytes() == bare[0].tobytes() and d_oc2.cpu().numpy().tobytes() == bare[1].tobytes()
    assert not _same(bare[0], want[0]) and _same(bare[4], pkg.sense_seen(B))


# ---- 5. the initial state --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_set_gait_starts_the_legs_in_their_patterns_state(pkg, lib, model):
    """phase0 on both sides of split, both patterns: after qmpc_loop_state_set_gait a walking robot's first tick advances every
    leg from its pattern's state at phase0 -- the record read back is one FSM update from the reset rule, and a leg that starts
    in swing is not in the tick's contacts."""
    cases = [(fs, split, ph) for fs in (0.0, 1.0) for split in (0.25, 0.625) for ph in (0.0, 0.125, 0.5, 0.75)]
    B = len(cases)
    p = _params(pkg, lib, model)
    lp = pkg.default_loop_params(lib)
    gait = pkg.gait_params(B, "trot_overlap", gait_freq=2.0)      # (the other three legs keep the robot on the ground)
    for i, (fs, split, ph) in enumerate(cases):
        gait["first_stance"][i, 2], gait["split"][i, 2], gait["phase0"][i, 2] = fs, split, ph
        gait["first_stance"][i, [0, 1, 3]], gait["split"][i, [0, 1, 3]], gait["phase0"][i, [0, 1, 3]] = 1.0, 0.75, [0.0, 0.25, 0.5]
    st = pkg.loop_states([[0.1, 0.0, 0.30, 0.0, 0.0, 0.0, 1.0]] * B, lp, height=0.3, yaw=np.linspace(-1, 1, B), lib=lib)
    st = pkg.loop_states_set_gait(st, gait, lib)
    s = _solver(pkg, lib, p, B, model)
    x, *_ = s.loop_run_gaits(st, 1, gait, lp=lp)
    s.close()
    swinging = 0
    for i, (fs, split, ph) in enumerate(cases):
        want = Leg(fs, split, ph)
        assert st["contacts"][i, 2] == want.state and tuple(float(st["leg"][i, 2][k]) for k in SCHEDULE) == want.fields()
        want.update(2.0 * (5.0 / 1000.0), True)
        assert tuple(float(x["leg"][i, 2][k]) for k in SCHEDULE) == want.fields(), (fs, split, ph)
        assert x["contacts"][i, 2] == want.state
        swinging += want.state == 0.0
    assert swinging >= 4 and (x["status"] == pkg.OK).all() and (x["tick"] == 1).all()


# ---- 6. refusals and buffers -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,form", FORMS)
def test_an_invalid_record_freezes_its_robot_alone(pkg, lib, B, form):
    T = 6
    p = pkg.default_params(10, pkg.MODE_CONVERGED, lib)
    lp, st = _fleet(pkg, lib, B, seed=9)
    ground = _binding(pkg, p, B)
    act, line = _mixed(pkg, p, lp, B)
    sense = pkg.random_go1_senses(B, seed=4)
    gait = _mixed_gaits(pkg, lp, B)
    bad_gait = gait.copy()
    cases = ([("gait_freq", None, v) for v in (0.0, -2.0, 12.5 + 1e-9, np.nan, np.inf)] + [("split", 1, v) for v in (0.3, 1 / 16, 15 / 16, np.nan)]
             + [("phase0", 2, v) for v in (1.0, -0.25, 0.1, np.inf)] + [("first_stance", 3, v) for v in (2.0, 0.5, np.nan)]
             + [("reserved", c, v) for c in (0, 1, 2) for v in (1.0, np.nan)])
    for i, (k, c, v) in enumerate(cases):
        if c is None:
            bad_gait[k][i] = v
        else:
            bad_gait[k][i, c] = v
    n = len(cases)
    bad_gait[n] = pkg.gait_params(1, "trot", gait_freq=2.0)      # pronk: all four legs swing together
    bad_gait["first_stance"][n] = 1.0
    bad_gait[n + 1] = pkg.gait_params(1, "crawl", gait_freq=2.0)      # a crawl whose last leg lifts early: a flight phase
    bad_gait["first_stance"][n + 1], bad_gait["phase0"][n + 1] = 1.0, [0.0, 0.75, 0.5, 0.375]
    bad = np.zeros(B, dtype=bool)
    bad[:n + 2] = True
    op = pkg.default_outcome_params(lib)
    oc0, ta0, sn0 = pkg.loop_outcomes(B, lib), pkg.ground_tallies(B), pkg.sense_seen(B)
    s = _solver(pkg, lib, p, B)
    assert s.loop_instances_plan(B, False, False)[0] == form
    ref = s.loop_run_gaits(st, T, gait, sense, None, act, line, ground, None, lp, op=op, trace=True)
    got = s.loop_run_gaits(st, T, bad_gait, sense, None, act, line, ground, None, lp, op=op, trace=True)
    s.close()
    x, oc, ta, li, sn, tf, tc = got
    frozen = st[bad].copy()
    frozen["status"], frozen["iterations"] = pkg.BAD_PARAMS, 0
    assert _same(x[bad], frozen) and (tf[:, bad] == 0).all() and (tc[:, bad] == 0).all()
    assert _same(oc[bad], oc0[bad]) and _same(ta[bad], ta0[bad]) and _same(li[bad], line[bad]) and _same(sn[bad], sn0[bad])
    assert all(_same(a[~bad], b[~bad]) for a, b in zip(got[:5], ref[:5])) and _same(tf[:, ~bad], ref[5][:, ~bad]) and _same(tc[:, ~bad], ref[6][:, ~bad])
    assert (ref[0]["tick"] == T).all()


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

    def code(s, ga=gait, se=sense, a=act, g=ground, pu=None, **kw):
        try:
            s.loop_run_gaits(kw.pop("st", st), 3, ga, se, None, a, None, g, pu, kw.pop("lp", lp), **kw)
            return pkg.OK
        except pkg.QmpcError as e:
            return e.code

    warm = pkg.default_loop_params(lib); warm.warm_start = 1.0
    sr = pkg.Solver(pkg.default_params(10, pkg.MODE_REFERENCE, lib), 4, device=0, lib=lib)
    assert code(sr, plant=plant) == pkg.UNSUPPORTED and code(sr) == pkg.UNSUPPORTED and code(sr, se=None, a=None, g=None) == pkg.UNSUPPORTED
    sr.close()
    s8 = pkg.Solver(pkg.default_biped8_params(16, pkg.MODE_CONVERGED, lib), 4, device=0, lib=lib)
    assert code(s8, plant=plant) == pkg.BAD_ARGUMENT and code(s8) == pkg.BAD_ARGUMENT
    s8.close()
    pc = pkg.default_convex_params(10, pkg.MODE_CONVERGED, lib)      # a ConvexMpc handle that did not opt in is refused
    sc = pkg.Solver(pc, 4, device=0, lib=lib)
    for kw in ({}, {"plant": pkg.plant_params(pc, 4)}, {"se": None, "a": None, "g": None}, {"pu": pkg.push_params(4)}):
        assert code(sc, **kw) == pkg.UNSUPPORTED, kw
    sc.set_convex_records(True)
    assert code(sc) == pkg.OK and code(sc, se=None, a=None, g=None) == pkg.OK
    sc.close()
    s = pkg.Solver(p, 4, device=0, lib=lib)
    assert code(s, ctrl=ctrl, lp=warm) == pkg.UNSUPPORTED      # (the handle did not opt in: qmpc_set_loop_warm_records)
    assert code(s, plant=plant, lp=warm) == pkg.OK and code(s) == pkg.OK and code(s, ctrl=ctrl) == pkg.OK
    assert code(s, se=None) == pkg.OK and code(s, se=None, a=None, g=None) == pkg.OK      # every other record may be absent
    assert code(s, pu=pkg.push_params(4, 0)) == pkg.BAD_ARGUMENT and code(s, pu=pkg.push_params(4, 9)) == pkg.BAD_ARGUMENT
    assert code(s, pu=pkg.push_params(4, 8)) == pkg.OK
    big = pkg.loop_states([[0.0, 0.0, 0.3, 0.0, 0.0, 0.0, 0.0]] * 5, lp, lib=lib)
    assert code(s, st=big, g=None, a=None, se=None, ga=pkg.gait_params(5, "pace")) == pkg.BATCH_TOO_LARGE
    s.set_loop_warm_records(True)
    assert code(s, ctrl=ctrl, lp=warm) == pkg.OK
    s.close()
    # buffers: the host-buffer gait call stages its records in a buffer of its own (128 B x max_batch), allocated by ticks = 0
    # too; no other call allocates it, a call with gait = None is the sensing call
    s = pkg.Solver(p, 1000, device=0, lib=lib)
    s.prepare(4)
    s.loop_run(st, 3, lp)
    s.loop_run_sensing(st, 3, sense, None, act, None, ground, pkg.push_params(4, 2), lp, ctrl=ctrl, plant=plant)
    before = s.query(pkg.QUERY_DEVICE_BYTES)
    s.loop_run_gaits(st, 3, None, sense, None, act, None, ground, pkg.push_params(4, 2), lp, ctrl=ctrl, plant=plant)
    assert s.query(pkg.QUERY_DEVICE_BYTES) == before
    got = s.loop_run_gaits(st, 0, gait, sense, None, act, None, ground, pkg.push_params(4, 2), lp, ctrl=ctrl, plant=plant, trace=True)
    assert _same(got[0], st) and _same(got[1], pkg.loop_outcomes(4, lib)) and _same(got[4], pkg.sense_seen(4))      # nothing was launched
    assert s.query(pkg.QUERY_DEVICE_BYTES) - before == 128 * 1000
    s.loop_run_gaits(st, 3, gait, None, None, None, None, None, None, lp, plant=plant)
    s.loop_run_sensing(st, 3, sense, None, act, None, ground, pkg.push_params(4, 2), lp, ctrl=ctrl, plant=plant)
    s.loop_run_instances(st, 3, lp, ctrl=ctrl, plant=plant)
    assert s.query(pkg.QUERY_DEVICE_BYTES) - before == 128 * 1000
    s.close()
    # a handle that only ever made gait calls without a sensing record has no staging for one
    s = pkg.Solver(p, 1000, device=0, lib=lib)
    s.prepare(4)
    s.loop_run_pushes(st, 3, pkg.push_params(4, 2), lp, ctrl=ctrl, plant=plant)
    before = s.query(pkg.QUERY_DEVICE_BYTES)
    s.loop_run_gaits(st, 0, gait, None, None, None, None, None, pkg.push_params(4, 2), lp, ctrl=ctrl, plant=plant)
    assert s.query(pkg.QUERY_DEVICE_BYTES) - before == 128 * 1000
    s.close()
