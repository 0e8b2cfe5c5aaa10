"""GPU suite (-m gpu): state-estimate bias and noise per robot in the closed loop (qmpc_loop_run_sensing*, include/qmpc.h;
DESIGN.md section 3w).

The call is qmpc_loop_run_actuation* whose controller reads a measured state: the true one plus the robot's bias and reproducible
bounded noise.  Identity records give that call's bytes and leave seen alone; a robot with a bias-only record solves exactly what
a robot standing in the measured state solves, while its plant moves exactly as a robot in the true state fed the same force;
with noise on, seen holds the rule's measurement of the state read back before the last tick; behind a delay line and on binding
ground the delivered force, the tally and the line are those of the actuation call; splits over calls, device buffers, launch
forms and the lane tick give the same bytes; ConvexMpc (opted in) behaves alike; the host twin agrees; invalid records freeze
their robot alone.  Every case is N = 10 and at most 40 ticks; sizes with two launch forms run once per form: 96 robots
(persistent kernel) and 3000 (per-tick graph on the wave kernels).  The measurement the device is compared against is
qh_sense_one of the host shim: loop_sense_one of csrc/qmpc_loop_math.h, the one source of the rule."""
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

pytestmark = pytest.mark.gpu

HERE = Path(__file__).resolve().parent
PLANT13 = ("pos_world", "quat", "lin_vel_world", "ang_vel_body")
# what the front end writes besides the record: the controller's memory and the tick's plan
FRONT = ("pos_d_world", "pos_d_init", "quat_d", "lin_vel_d_rel", "vel_filter", "pos_filter", "leg", "contacts", "gait_counter",
         "foot_target_world", "attitude_traj_count")
BIAS = np.array([0.012, -0.02, 0.006, 0.03, -0.05, 0.08, 0.06, -0.03, 0.02, 0.04, 0.02, -0.05])


@pytest.fixture(scope="module")
def shim():
    import __graft_entry__ as g

    host = C.CDLL(str(g.build_host()))
    vp = C.c_void_p
    host.qh_sense_one.argtypes = [vp, C.c_double, vp, vp]
    host.qh_sense_one.restype = C.c_int
    host.qh_loop_create_robot.argtypes = [C.c_char_p, C.c_int, vp, vp, vp, vp]
    host.qh_loop_create_robot.restype = vp
    for f in ("qh_loop_tick", "qh_loop_destroy", "qh_loop_device_status"):
        getattr(host, f).argtypes = [vp]
    for f in ("qh_loop_outcome", "qh_loop_export", "qh_loop_set_ground", "qh_loop_ground_tally", "qh_loop_actuation_line", "qh_loop_set_sense",
              "qh_loop_sense_seen"):
        getattr(host, f).argtypes = [vp, vp]
    host.qh_loop_set_actuation.argtypes = [vp, vp, vp]
    host.qh_loop_set_pushes.argtypes = [vp, vp, C.c_int]
    host.qh_loop_set_command.argtypes = [vp, vp, C.c_double]
    return host


def _x13(st):
    return np.ascontiguousarray(np.concatenate([st[k] for k in PLANT13], axis=1))


def _put13(st, m):
    out = st.copy()
    out["pos_world"], out["quat"], out["lin_vel_world"], out["ang_vel_body"] = m[:, 0:3], m[:, 3:7], m[:, 7:10], m[:, 10:13]
    return out


def _measure(shim, sense, st):
    """qh_sense_one of every robot's record on its state at its state.tick: [B, 13]"""
    x = _x13(st)
    m = np.zeros_like(x)
    for i in range(len(st)):
        assert shim.qh_sense_one(sense[i:i + 1].ctypes.data, float(st["tick"][i]), x[i].ctypes.data, m[i].ctypes.data) == 1
    return m


def _biased(pkg, B):
    """bias-only records (sigma = 0) on all four channel groups, scaled per robot; every fourth the identity"""
    se = pkg.sense_params(B, seed=np.arange(B))
    se["bias"] = BIAS[None, :] * (0.25 + (np.arange(B) % 7)[:, None] / 4.0) * np.where(np.arange(B) % 2, -1.0, 1.0)[:, None]
    se["bias"][np.arange(B) % 4 == 3] = 0.0
    return se


def _noisy(pkg, B, seed=3):
    """records by i mod 4: the identity, a bias on all groups, noise on all twelve channels, a random bias and noise"""
    se = pkg.random_go1_senses(B, seed=seed)
    k = np.arange(B) % 4
    se["bias"][k == 0], se["sigma"][k == 0] = 0.0, 0.0
    se["sigma"][k == 1] = 0.0
    se["bias"][k == 1] = BIAS
    se["bias"][k == 2] = 0.0
    se["sigma"][k == 2] = np.abs(BIAS) / 2
    return se


def _marked_seen(pkg, B):
    """seen records that are visibly not fresh: an untouched one comes back with these bytes"""
    sn = pkg.sense_seen(B)
    sn["meas"], sn["ticks"], sn["reserved"] = 7.0, 3.0, -1.0
    return sn


def _walked(pkg, lib, s, B, model, ticks=9, seed=1):
    """the walking fleet after 6 ticks standing and `ticks` ticks on its commands, through the plain loop (the switch resets the
    gait, after which two legs swing at once): moving robots with their controller memory in place"""
    lp, st = _fleet(pkg, lib, B, seed=seed, model=model)
    mode = st["movement_mode"].copy()
    st["movement_mode"] = 0.0
    st = s.loop_run(st, 6, lp)
    st["movement_mode"] = mode
    return lp, s.loop_run(st, ticks, lp)


# ---- 1. identity records give the actuation call -------------------------------------------------------------------------
@pytest.mark.parametrize("B,form", FORMS)
@pytest.mark.parametrize("kind", ["both", "neither"])
@pytest.mark.parametrize("model", MODELS)
def test_identity_records_give_the_actuation_call(pkg, lib, B, form, kind, model):
    """With identity records, and with sense = None, states, outcome records, tallies, lines and both traces are the actuation
    call's bytes and seen comes back untouched -- with every other record present (mixed actuation records, binding ground,
    shoves) and with none of them (act = None, ground = None: the outcome call's robots)."""
    T = 20
    p = _params(pkg, lib, model)
    lp, st = _fleet(pkg, lib, B, model=model)
    ctrl, plant = _records(pkg, p, B, kind, model=model)
    op = pkg.default_outcome_params(lib)
    push = _shoves(pkg, lp, B, 40, (3.0, 9.0), (4.0, 5.0))
    ground = _binding(pkg, p, B)
    act, line = _mixed(pkg, p, lp, B)
    ident, seen0 = pkg.sense_params(B, seed=np.arange(B) * 1000.0), _marked_seen(pkg, B)
    s = _solver(pkg, lib, p, B, model)
    assert s.loop_instances_plan(B, ctrl is not None, False)[0] == form
    want = s.loop_run_actuation(st, T, act, line, ground, push, lp, ctrl=ctrl, plant=plant, op=op, trace=True)
    got = s.loop_run_sensing(st, T, ident, seen0, act, line, ground, push, lp, ctrl=ctrl, plant=plant, op=op, trace=True)
    none = s.loop_run_sensing(st, T, None, seen0, act, line, ground, push, lp, ctrl=ctrl, plant=plant, op=op, trace=True)
    bare_want = s.loop_run_actuation(st, T, None, None, None, None, lp, ctrl=ctrl, plant=plant, op=op, trace=True)
    bare = s.loop_run_sensing(st, T, ident, seen0, None, line, None, None, lp, ctrl=ctrl, plant=plant, op=op, trace=True)
    s.close()
    assert (want[0]["tick"] == T).all() and (want[2]["clipped_ticks"] > 0).any() and not _same(want[0], bare_want[0])
    for run in (got, none):
        assert _all_same(run[:4] + run[5:], want) and _same(run[4], seen0)
    assert _all_same(bare[:3] + bare[5:], bare_want[:3] + bare_want[4:]) and _same(bare[3], line) and _same(bare[4], seen0)      # act = NULL: line untouched


def test_identity_on_the_lane_tick_with_uniform_controller_records(pkg, lib):
    """20480 robots under QMPC_INSTANCES_AUTO with uniform controller records, as the actuation suite's test of that name: the
    sensing call with identity records against the actuation call, on the lane kernel -- and a bias on every fourth robot moves
    that robot alone."""
    B, T = 20480, 10
    p, lp, st = _standing(pkg, lib, B, np.linspace(-3, 3, B))
    cls = np.arange(B) % 4
    ground = pkg.ground_params(B)
    ground["fz_max"][cls == 1] = p.mass * G / 8.0
    ground["mu"][cls == 3] = 0.5 * p.mu
    push = pkg.push_params(B)
    push["start_tick"][cls >= 2], push["ticks"][cls >= 2] = 2.0, 6.0
    push["force_world"][cls >= 2, 0, 1] = 60.0
    ctrl = pkg.instance_params(p, B)
    act = pkg.actuation_params(B, delay_ticks=cls.astype(float))
    op = pkg.default_outcome_params(lib, stop_when_down=True)
    some = pkg.sense_params(B)
    some["bias"][cls == 2] = BIAS
    s = _solver(pkg, lib, p, B)
    s.set_instances_policy("auto")
    assert s.loop_instances_plan(B, True, False)[0] == "per_tick" and s.loop_instances_plan(B, True, False)[1].startswith("lane")
    want = s.loop_run_actuation(st, T, act, None, ground, push, lp, ctrl=ctrl, op=op, trace=True)
    got = s.loop_run_sensing(st, T, pkg.sense_params(B), None, act, None, ground, push, lp, ctrl=ctrl, op=op, trace=True)
    assert pkg.KERNEL_FAMILY[s.query(pkg.QUERY_LAST_KERNEL)].startswith("lane")
    part = s.loop_run_sensing(st, T, some, None, act, None, ground, push, lp, ctrl=ctrl, op=op)
    s.close()
    assert _all_same(got[:4] + got[5:], want) and _same(got[4], pkg.sense_seen(B))
    assert _same(part[0][cls != 2], want[0][cls != 2]) and (part[4]["ticks"][cls == 2] == part[0]["tick"][cls == 2]).all()
    assert np.mean([part[0][i].tobytes() != want[0][i].tobytes() for i in np.flatnonzero(cls == 2)]) > 0.9


# ---- 2. the measurement replaces the state --------------------------------------------------------------------------------
@pytest.mark.parametrize("B,form", FORMS)
@pytest.mark.parametrize("model", MODELS)
def test_measurement_replaces_the_state(pkg, lib, shim, B, form, model):
    """One tick, bias-only records on all four channel groups.  Robot A starts from s0 with the record; robot B starts from s0
    with its 13 plant doubles replaced by qh_sense_one(s0), with the identity record: after the tick everything the controller
    wrote is byte-identical -- the solve's force (QuatMpc: forces_body; ConvexMpc, whose solve returns world-frame forces and
    whose forces_body = R' u is formed with the robot's own R afterwards: grf_world), the plan and the controller's memory.
    Robot C starts from the true s0 without a sensing record, behind a delay line of one tick whose slots hold A's forces_body:
    its plant receives A's force, and A's plant fields are C's bytes -- and not B's.  seen.meas is qh_sense_one(s0)."""
    p = _params(pkg, lib, model)
    s = _solver(pkg, lib, p, B, model)
    assert s.loop_instances_plan(B, False, False)[0] == form
    lp, s0 = _walked(pkg, lib, s, B, model)
    sense = _biased(pkg, B)
    on = np.arange(B) % 4 != 3
    m = _measure(shim, sense, s0)
    a = s.loop_run_sensing(s0, 1, sense, _marked_seen(pkg, B), lp=lp)
    b = s.loop_run_sensing(_put13(s0, m), 1, pkg.sense_params(B), lp=lp)
    delay1 = pkg.actuation_params(B, delay_ticks=1)
    c = s.loop_run_actuation(s0, 1, delay1, pkg.actuation_lines(B, a[0]["forces_body"]), None, None, lp)
    s.close()
    A, Bs, Cs = a[0], b[0], c[0]
    assert (A["tick"] == s0["tick"] + 1).all() and np.isin(A["status"], (pkg.OK, pkg.MAX_ITER)).mean() > 0.9 and (s0["contacts"] == 0).any()
    for k in FRONT + ("status", "iterations", "grf_world" if model == "convex" else "forces_body"):
        assert _same(A[k], Bs[k]), k
    assert (A["forces_body"][on] != Cs["forces_body"][on]).any(axis=1).mean() > 0.9      # the bias changed what was solved
    for k in PLANT13:      # (a swing foot goes to the FSM's target, which comes from the state the controller read: B's, not C's)
        assert _same(A[k], Cs[k]), k
    assert _same(A["foot_pos_world"], Bs["foot_pos_world"])
    assert all((A[k][on] != Bs[k][on]).any(axis=1).all() for k in ("pos_world", "quat"))
    # seen: the measurement, one tick more; an identity record leaves it alone
    marked = _marked_seen(pkg, B)
    assert _same(a[4]["meas"][on], m[on]) and (a[4]["ticks"][on] == 4.0).all() and _same(a[4][~on], marked[~on])
    assert _same(m[~on], _x13(s0)[~on]) and (m[on] != _x13(s0)[on]).all()


# ---- 3. with noise on, seen holds the measurement of the state before the last tick --------------------------------------
@pytest.mark.parametrize("B,form", FORMS)
@pytest.mark.parametrize("model", MODELS)
def test_seen_is_the_rule_on_the_state_read_back(pkg, lib, shim, B, form, model):
    T = 12
    p = _params(pkg, lib, model)
    lp, st = _fleet(pkg, lib, B, seed=3, model=model)
    sense = _noisy(pkg, B)
    on = np.arange(B) % 4 != 0
    s = _solver(pkg, lib, p, B, model)
    assert s.loop_instances_plan(B, False, False)[0] == form
    before = s.loop_run_sensing(st, T - 1, sense, None, lp=lp)
    after = s.loop_run_sensing(before[0], 1, sense, before[4], lp=lp, outcomes=before[1])
    clean = s.loop_run_sensing(st, T, None, None, lp=lp)
    s.close()
    m = _measure(shim, sense, before[0])
    assert (before[0]["tick"] == T - 1).all() and (after[0]["tick"] == T).all()
    assert _same(after[4]["meas"][on], m[on]) and (after[4]["ticks"][on] == T).all() and _same(after[4][~on], pkg.sense_seen(B)[~on])
    # the measurement is not the state, and the noisy robots went another way than the clean ones
    k = np.arange(B) % 4
    assert (m[on] != _x13(before[0])[on]).any(axis=1).all() and _same(m[~on], _x13(before[0])[~on])
    assert _same(after[0][~on], clean[0][~on])
    assert np.mean([after[0][i].tobytes() != clean[0][i].tobytes() for i in np.flatnonzero(on)]) > 0.95


# ---- 4. splits over calls ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,form", FORMS)
def test_calls_split_give_one_call(pkg, lib, B, form):
    """30 ticks in one call against calls of 1, 10, 6 and 13 ticks (cuts at 1 / 11 / 17) that hand on states, outcome records,
    tallies, lines and seen: the noise is keyed on state.tick, not on the call."""
    T = 30
    p = pkg.default_params(10, pkg.MODE_CONVERGED, lib)
    lp, st = _fleet(pkg, lib, B, seed=4)
    ctrl, plant = _records(pkg, p, B, "both", seed=8)
    push = _shoves(pkg, lp, B, 41, (4.0, 8.0), (5.0, 4.0))
    ground = _binding(pkg, p, B)
    act, line = _mixed(pkg, p, lp, B)
    sense = _noisy(pkg, B, seed=5)
    op = pkg.default_outcome_params(lib, stop_when_down=True)
    s = _solver(pkg, lib, p, B)
    assert s.loop_instances_plan(B, True, False)[0] == form
    run = lambda x, t, li, sn=None, oc=None, ta=None: s.loop_run_sensing(x, t, sense, sn, act, li, ground, push, lp, ctrl=ctrl, plant=plant,      # noqa: E731
                                                                         op=op, outcomes=oc, tallies=ta, trace=True)
    whole = run(st, T, line)
    parts, x = [], (st, None, None, line, None)
    for n in (1, 10, 6, T - 17):
        x = run(x[0], n, x[3], x[4], x[1], x[2])
        parts.append(x)
    ident = s.loop_run_sensing(st, T, pkg.sense_params(B), None, act, line, ground, push, lp, ctrl=ctrl, plant=plant, op=op)
    s.close()
    assert _all_same(whole[:5], x[:5])
    assert _same(whole[5], np.concatenate([q[5] for q in parts])) and _same(whole[6], np.concatenate([q[6] for q in parts]))
    k = np.arange(B) % 4
    assert (whole[4]["ticks"][k != 0] == whole[0]["tick"][k != 0]).all() and (whole[4]["ticks"][k == 0] == 0).all()
    assert _same(whole[0][k == 0], ident[0][k == 0])
    assert np.mean([whole[0][i].tobytes() != ident[0][i].tobytes() for i in np.flatnonzero(k != 0)]) > 0.9


# ---- 5. the launch forms at one size -------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_launch_forms_give_the_same_bytes(model):
    worker = HERE / "_loop_sensing_worker.py"
    out = {}
    for fused in ("0", "1"):
        env = dict(os.environ, QMPC_LOOP_FUSED=fused)
        r = subprocess.run([sys.executable, str(worker), "200", "40", "10", "stop", model], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.splitlines()
        out[fused] = tuple([l for l in lines if l.startswith(k)][0] for k in ("FORM", "OUTCOMES", "SHA"))
    print(out)
    f0, f1 = eval(out["0"][0][5:]), eval(out["1"][0][5:])
    assert f0[0] == "per_tick" and f1[0] == "persistent"
    assert out["0"][1] == out["1"][1] and out["0"][2] == out["1"][2]


# ---- 6. device buffers ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_device_buffers_give_the_host_call(pkg, lib, model):
    import torch

    B, T = 48, 25
    p = _params(pkg, lib, model)
    lp, st = _fleet(pkg, lib, B, seed=6, model=model)
    ctrl, plant = _records(pkg, p, B, "both", seed=2, model=model)
    push = _shoves(pkg, lp, B, 43, (2.0, 6.0, 15.0), (5.0, 3.0, 6.0))
    ground = _binding(pkg, p, B)
    act, line = _mixed(pkg, p, lp, B)
    sense, seen0 = _noisy(pkg, B, seed=9), _marked_seen(pkg, B)
    op = pkg.default_outcome_params(lib, stop_when_down=True)
    s = _solver(pkg, lib, p, B, model)
    want = s.loop_run_sensing(st, T, sense, seen0, act, line, ground, push, lp, ctrl=ctrl, plant=plant, op=op, trace=True)
    bare = s.loop_run_sensing(st, T, sense, seen0, None, None, None, None, lp, plant=plant, op=op, want_seen=False)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1).copy()).cuda()      # noqa: E731
    d_st, d_oc, d_ta, d_ctrl, d_plant = dev(st), dev(pkg.loop_outcomes(B, lib)), dev(pkg.ground_tallies(B)), dev(ctrl), dev(plant)
    d_push, d_ground, d_act, d_line, d_sense, d_seen = dev(push), dev(ground), dev(act), dev(line), dev(sense), dev(seen0)
    d_tf = torch.full((T, B, 12), 7.0, dtype=torch.float64, device="cuda")
    d_tc = torch.full((T, B, 4), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s.loop_run_sensing_device(B, d_st.data_ptr(), T, d_oc.data_ptr(), d_sense.data_ptr(), d_seen.data_ptr(), d_act.data_ptr(), d_line.data_ptr(),
                              d_ground.data_ptr(), d_ta.data_ptr(), d_push.data_ptr(), 3, lp, op, d_ctrl=d_ctrl.data_ptr(),
                              d_plant=d_plant.data_ptr(), d_trace_forces=d_tf.data_ptr(), d_trace_contacts=d_tc.data_ptr())
    s.wait()
    # ... and with the sensing record alone (act, line, ground, push and seen NULL), from the start again
    d_st2, d_oc2 = dev(st), dev(pkg.loop_outcomes(B, lib))
    torch.cuda.synchronize()
    s.loop_run_sensing_device(B, d_st2.data_ptr(), T, d_oc2.data_ptr(), d_sense.data_ptr(), lp=lp, op=op, d_plant=d_plant.data_ptr())
    s.wait()
    s.close()
    assert d_st.cpu().numpy().tobytes() == want[0].tobytes() and d_oc.cpu().numpy().tobytes() == want[1].tobytes()
    assert d_ta.cpu().numpy().tobytes() == want[2].tobytes() and d_line.cpu().numpy().tobytes() == want[3].tobytes()
    assert d_seen.cpu().numpy().tobytes() == want[4].tobytes() and not _same(want[4], seen0)
    assert _same(d_tf.cpu().numpy(), want[5]) and _same(d_tc.cpu().numpy(), want[6])
    assert d_sense.cpu().numpy().tobytes() == sense.tobytes() and d_act.cpu().numpy().tobytes() == act.tobytes()      # read in place
    assert d_st2.cpu().numpy().tobytes() == bare[0].tobytes() and d_oc2.cpu().numpy().tobytes() == bare[1].tobytes()
    assert _same(bare[4], seen0) and _same(bare[3], pkg.actuation_lines(B)) and not _same(bare[0], want[0])      # seen = NULL: never written


# ---- 7. the host class ---------------------------------------------------------------------------------------------------
def test_host_class_with_a_sensing_record(pkg, lib, shim):
    """Six robots, 40 ticks (6 standing, 34 on their commands), a shove on robot 1; sensing records: the identity, a gyro bias, a
    position bias with position noise, noise on all channels, an attitude bias, a random record; robot 3 behind a delay of 2
    ticks and a lag of 10 ms, robot 2 under a 45 N normal limit -- against the host twin (host/ClosedLoopHost.h: the same tick
    on the CPU through loop_sense_one, loop_actuation_one, loop_ground_clamp and plant_step_ext).  Outcome counters and
    measurement counts equal; fields to the tolerances of the actuation suite's test_host_class_behind_delay_and_lag."""
    N, T0, T, B = 10, 6, 34, 6
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    lp = pkg.default_loop_params(lib)
    cmds = np.array(COMMANDS)
    cmds[:, 6] = 1.0
    stand = cmds.copy(); stand[:, 6] = 0.0
    st = pkg.loop_states(stand, lp, height=0.3, yaw=np.linspace(-2, 2, B), lib=lib)
    push = pkg.push_params(B, 2)
    push[1, 0] = (20.0, 6.0, [0.0, 30.0, 0.0], [0.0, 0.0, 0.0])
    ground = pkg.ground_params(B)
    ground["fz_max"][2] = 45.0
    act = pkg.actuation_params(B, delay_ticks=[0, 0, 0, 2, 0, 1], tau=[0.0, 0.0, 0.0, 0.01, 0.0, 0.0], dt=lp.dt)
    line = pkg.actuation_lines(B, pkg.stand_forces_body(p.mass))
    sense = pkg.random_go1_senses(B, seed=2)
    sense["bias"][:5], sense["sigma"][:5] = 0.0, 0.0
    sense["bias"][1, 9:12] = [0.03, -0.02, 0.04]
    sense["bias"][2, 0:3], sense["sigma"][2, 0:3] = [0.01, -0.015, 0.008], 0.004
    sense["sigma"][3] = np.abs(BIAS) / 4
    sense["bias"][4, 3:6] = [0.03, -0.04, 0.06]
    s = pkg.Solver(p, B, device=0, lib=lib)
    x, oc, ta, li, sn = s.loop_run_sensing(st, T0, sense, None, act, line, ground, push, lp)
    x["movement_mode"] = cmds[:, 6]
    fin, oc, ta, li, sn = s.loop_run_sensing(x, T, sense, sn, act, li, ground, push, lp, outcomes=oc, tallies=ta)
    s.close()
    ho, ht, hl, hn = pkg.loop_outcomes(B, lib), pkg.ground_tallies(B), pkg.actuation_lines(B), pkg.sense_seen(B)
    hs = np.zeros(B, dtype=pkg.LOOP_STATE_DTYPE)
    for i in range(B):
        h = shim.qh_loop_create_robot(str(pkg.LIB_PATH).encode(), N, C.addressof(lp), st[i:i + 1].ctypes.data, None, None)
        assert h and shim.qh_loop_device_status(h) == 0
        shim.qh_loop_set_pushes(h, push[i].ctypes.data, 2)
        shim.qh_loop_set_ground(h, ground[i:i + 1].ctypes.data)
        shim.qh_loop_set_actuation(h, act[i:i + 1].ctypes.data, line[i:i + 1].ctypes.data)
        shim.qh_loop_set_sense(h, sense[i:i + 1].ctypes.data)
        for _ in range(T0):
            assert shim.qh_loop_tick(h) == 1
        shim.qh_loop_set_command(h, np.ascontiguousarray(cmds[i, :6]).ctypes.data, float(cmds[i, 6]))
        for t in range(T):
            assert shim.qh_loop_tick(h) == 1, (i, t)
        shim.qh_loop_outcome(h, ho[i:i + 1].ctypes.data)
        shim.qh_loop_ground_tally(h, ht[i:i + 1].ctypes.data)
        shim.qh_loop_actuation_line(h, hl[i:i + 1].ctypes.data)
        shim.qh_loop_sense_seen(h, hn[i:i + 1].ctypes.data)
        shim.qh_loop_export(h, hs[i:i + 1].ctypes.data)
        shim.qh_loop_destroy(h)
    assert np.array_equal(sn["ticks"], hn["ticks"]) and sn["ticks"].tolist() == [0.0] + [float(T0 + T)] * 5
    assert np.array_equal(li["count"], hl["count"]) and (li["count"] == T0 + T).all()
    for k in COUNTERS:
        assert np.array_equal(oc[k], ho[k]), k
    worst = {k: float(np.abs(oc[k] - ho[k]).max()) for k in ("min_height", "min_upright", "max_height_err", "max_vel_err", "max_ang_vel",
                                                            "max_force_z", "sum_vel_err_sq")}
    worst_state = {k: float(np.abs(fin[k] - hs[k]).max()) for k in ("pos_world", "quat", "lin_vel_world", "ang_vel_body", "grf_world")}
    worst_meas = float(np.abs(sn["meas"] - hn["meas"]).max())
    print("device against host, worst differences:", worst, "final states (not asserted):", worst_state, "meas (not asserted):", worst_meas)
    for k in ("min_height", "min_upright", "max_height_err", "max_vel_err", "max_ang_vel"):
        assert worst[k] <= 1e-8, (k, worst)
    assert worst["max_force_z"] <= 1e-6
    assert (np.abs(oc["sum_vel_err_sq"] - ho["sum_vel_err_sq"]) <= oc["ticks"] * 2 * oc["max_vel_err"] * 1e-8).all()
    assert (fin["tick"] == T0 + T).all() and (oc["ticks"][oc["down_tick"] < 0] == T0 + T).all()
    # the records did something: the clean robot 0 aside, the host's measurement is not its state
    assert (hn["meas"][1:] != _x13(hs)[1:]).any(axis=1).all()


# ---- 8. composition: behind a delay line, on binding ground --------------------------------------------------------------
@pytest.mark.parametrize("B,form", FORMS)
@pytest.mark.parametrize("model", MODELS)
def test_sensing_composes_with_the_delay_line_and_the_ground(pkg, lib, shim, B, form, model):
    """Three ticks, one call each, bias-only sensing records, every robot behind a delay of 1 .. 4 ticks (some with a lag) on
    binding ground.  With a delay the force delivered in a tick does not depend on that tick's command, so in each tick robot C
    -- the true state, lines, tallies and outcome records of A, no sensing record, through the actuation call -- must deliver
    what A delivers: grf_world, the tally, the plant fields, the line's applied and count and every ring slot but the one the
    tick's command went to are A's bytes.  That slot holds A's command: the bytes robot B solves (test 2's construction: the
    measured state, the identity record; QuatMpc -- ConvexMpc's forces_body = R' u carries the robot's own R).  (A swing foot
    lands on the FSM's target, which comes from the state the controller read: foot_pos_world is A's own and is handed on.)"""
    p = _params(pkg, lib, model)
    s = _solver(pkg, lib, p, B, model)
    assert s.loop_instances_plan(B, False, False)[0] == form
    lp, x = _walked(pkg, lib, s, B, model, seed=5)
    sense = _biased(pkg, B)
    on = np.arange(B) % 4 != 3
    ground = _binding(pkg, p, B)
    ground["fz_max"][np.arange(B) % 3 == 2] = 30.0      # every robot on ground that binds or nearly does
    act = pkg.actuation_params(B, delay_ticks=1.0 + np.arange(B) % 4, tau=np.where(np.arange(B) % 2, 0.01, 0.0), dt=lp.dt)
    li = pkg.actuation_lines(B, pkg.stand_forces_body(p.mass) * 1.3)
    oc, ta, sn = None, None, None
    clipped = differs = 0
    for t in range(3):
        a = s.loop_run_sensing(x, 1, sense, sn, act, li, ground, None, lp, outcomes=oc, tallies=ta)
        c = s.loop_run_actuation(x, 1, act, li, ground, None, lp, outcomes=oc, tallies=ta)
        b = s.loop_run_actuation(_put13(x, _measure(shim, sense, x)), 1, act, li, ground, None, lp, outcomes=oc, tallies=ta)
        A, Cs = a[0], c[0]
        for k in PLANT13 + ("grf_world", "contacts", "tick"):
            assert _same(A[k], Cs[k]), (t, k)
        assert _same(a[2], c[2]) and _same(a[3]["applied"], c[3]["applied"]) and _same(a[3]["count"], c[3]["count"])
        slot = int(li["count"][0]) % 8
        keep = [q for q in range(8) if q != slot]
        assert _same(a[3]["cmd"][:, keep], c[3]["cmd"][:, keep]) and _same(a[3]["cmd"][:, slot], A["forces_body"])
        if model == "quat":
            assert _same(A["forces_body"], b[0]["forces_body"]) and _same(a[3]["cmd"][:, slot], b[3]["cmd"][:, slot])
        differs += int((A["forces_body"][on] != Cs["forces_body"][on]).any(axis=1).sum())
        clipped = int((a[2]["clipped_ticks"] > 0).sum())
        x, oc, ta, li, sn = a
    s.close()
    assert clipped > B // 10 and differs > 2 * int(on.sum())      # the ground bound, and the bias changed most commands
    assert (sn["ticks"][on] == 3).all() and (sn["ticks"][~on] == 0).all()


# ---- 9. refusals and buffers ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,form", FORMS)
def test_an_invalid_record_freezes_its_robot_alone(pkg, lib, B, form):
    T = 6
    p = pkg.default_params(10, pkg.MODE_CONVERGED, lib)
    lp, st = _fleet(pkg, lib, B, seed=9)
    ground = _binding(pkg, p, B)
    act, line = _mixed(pkg, p, lp, B)
    sense, seen0 = _noisy(pkg, B, seed=4), _marked_seen(pkg, B)
    bad_sense = sense.copy()
    cases = ([("bias", c, v) for c in (0, 4, 11) for v in (np.nan, np.inf)] + [("sigma", c, v) for c in (1, 5, 9) for v in (-1e-9, np.nan, -np.inf)]
             + [("seed", None, v) for v in (-1.0, 0.5, 2.0 ** 53, np.nan, np.inf)] + [("reserved", 3, np.nan)])
    for i, (k, c, v) in enumerate(cases):
        if c is None:
            bad_sense[k][i] = v
        else:
            bad_sense[k][i, c] = v
    bad = np.zeros(B, dtype=bool)
    bad[:len(cases)] = True
    op = pkg.default_outcome_params(lib)
    oc0, ta0 = pkg.loop_outcomes(B, lib), pkg.ground_tallies(B)
    s = _solver(pkg, lib, p, B)
    assert s.loop_instances_plan(B, False, False)[0] == form
    ref = s.loop_run_sensing(st, T, sense, seen0, act, line, ground, None, lp, op=op, trace=True)
    got = s.loop_run_sensing(st, T, bad_sense, seen0, act, line, ground, None, lp, op=op, trace=True)
    s.close()
    x, oc, ta, li, sn, tf, tc = got
    frozen = st[bad].copy()
    frozen["status"], frozen["iterations"] = pkg.BAD_PARAMS, 0
    assert _same(x[bad], frozen) and (tf[:, bad] == 0).all() and (tc[:, bad] == 0).all()
    assert _same(oc[bad], oc0[bad]) and _same(ta[bad], ta0[bad]) and _same(li[bad], line[bad]) and _same(sn[bad], seen0[bad])
    assert all(_same(a[~bad], b[~bad]) for a, b in zip(got[:5], ref[:5])) and _same(tf[:, ~bad], ref[5][:, ~bad]) and _same(tc[:, ~bad], ref[6][:, ~bad])
    assert (ref[0]["tick"] == T).all() and (ref[4]["ticks"][np.arange(B) % 4 != 0] == 3 + T).all()


def test_refusals_and_buffers(pkg, lib):
    lp = pkg.default_loop_params(lib)
    st = pkg.loop_states([[0.0, 0.0, 0.3, 0.0, 0.0, 0.0, 0.0]] * 4, lp, lib=lib)
    p = pkg.default_params(10, pkg.MODE_CONVERGED, lib)
    ctrl, plant = pkg.instance_params(p, 4), pkg.plant_params(p, 4)
    ground = pkg.ground_params(4)
    ground["mu"] = 0.4
    act = pkg.actuation_params(4, 2, 0.01)
    sense = pkg.sense_params(4, seed=1, gyro_bias=0.01, pos_noise=0.003)

    def code(s, se=sense, a=act, g=ground, pu=None, **kw):
        try:
            s.loop_run_sensing(kw.pop("st", st), 3, se, None, a, None, g, pu, kw.pop("lp", lp), **kw)
            return pkg.OK
        except pkg.QmpcError as e:
            return e.code

    warm = pkg.default_loop_params(lib); warm.warm_start = 1.0
    sr = pkg.Solver(pkg.default_params(10, pkg.MODE_REFERENCE, lib), 4, device=0, lib=lib)
    assert code(sr, plant=plant) == pkg.UNSUPPORTED and code(sr) == pkg.UNSUPPORTED and code(sr, se=None) == pkg.UNSUPPORTED
    assert code(sr, a=None, g=None) == pkg.UNSUPPORTED
    sr.close()
    s8 = pkg.Solver(pkg.default_biped8_params(16, pkg.MODE_CONVERGED, lib), 4, device=0, lib=lib)
    assert code(s8, plant=plant) == pkg.BAD_ARGUMENT and code(s8) == pkg.BAD_ARGUMENT
    s8.close()
    # a ConvexMpc handle that did not opt in is refused
    pc = pkg.default_convex_params(10, pkg.MODE_CONVERGED, lib)
    sc = pkg.Solver(pc, 4, device=0, lib=lib)
    for kw in ({}, {"plant": pkg.plant_params(pc, 4)}, {"g": None}, {"a": None, "g": None}, {"pu": pkg.push_params(4)}):
        assert code(sc, **kw) == pkg.UNSUPPORTED, kw
    sc.set_convex_records(True)
    assert code(sc) == pkg.OK and code(sc, g=None) == pkg.OK and code(sc, a=None, g=None) == pkg.OK
    sc.close()
    s = pkg.Solver(p, 4, device=0, lib=lib)
    assert code(s, ctrl=ctrl, lp=warm) == pkg.UNSUPPORTED      # (the handle did not opt in: qmpc_set_loop_warm_records)
    assert code(s, plant=plant, lp=warm) == pkg.OK and code(s) == pkg.OK and code(s, ctrl=ctrl) == pkg.OK and code(s, g=None) == pkg.OK
    assert code(s, a=None) == pkg.OK and code(s, a=None, g=None) == pkg.OK      # act == NULL with sense
    assert code(s, pu=pkg.push_params(4, 0)) == pkg.BAD_ARGUMENT and code(s, pu=pkg.push_params(4, 9)) == pkg.BAD_ARGUMENT
    assert code(s, pu=pkg.push_params(4, 8)) == pkg.OK
    big = pkg.loop_states([[0.0, 0.0, 0.3, 0.0, 0.0, 0.0, 0.0]] * 5, lp, lib=lib)
    assert code(s, st=big, g=pkg.ground_params(5), a=pkg.actuation_params(5), se=pkg.sense_params(5)) == pkg.BATCH_TOO_LARGE
    s.set_loop_warm_records(True)
    assert code(s, ctrl=ctrl, lp=warm) == pkg.OK      # ... and with the opt-in the warm-started ticks with controller records run
    # act without a line, and a NULL op, with everything else in place
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    x, oc, ta, li, sn = st.copy(), pkg.loop_outcomes(4, lib), pkg.ground_tallies(4), pkg.actuation_lines(4), pkg.sense_seen(4)
    op = pkg.default_outcome_params(lib)
    assert lib.qmpc_loop_run_sensing(s._h, C.byref(lp), 4, vp(x), 3, None, None, None, None, C.byref(op), vp(oc), None, 0, vp(ground), vp(ta),
                                     vp(act), None, vp(sense), vp(sn)) == pkg.BAD_ARGUMENT
    assert lib.qmpc_loop_run_sensing(s._h, C.byref(lp), 4, vp(x), 3, None, None, None, None, None, vp(oc), None, 0, vp(ground), vp(ta),
                                     vp(act), vp(li), vp(sense), vp(sn)) == pkg.BAD_ARGUMENT
    assert _same(x, st) and _same(ta, pkg.ground_tallies(4)) and _same(li, pkg.actuation_lines(4)) and _same(oc, pkg.loop_outcomes(4, lib))
    assert _same(sn, pkg.sense_seen(4))
    s.close()
    # buffers: the host-buffer sensing call stages records and seen in a buffer of its own ((256 + 128) B x max_batch), allocated by
    # ticks = 0 too; no other call allocates it, a call with sense = None is the actuation call
    s = pkg.Solver(p, 1000, device=0, lib=lib)
    s.prepare(4)
    s.loop_run(st, 3, lp)
    s.loop_run_actuation(st, 3, act, None, ground, pkg.push_params(4, 2), lp, ctrl=ctrl, plant=plant)
    before = s.query(pkg.QUERY_DEVICE_BYTES)
    s.loop_run_sensing(st, 3, None, None, act, None, ground, pkg.push_params(4, 2), lp, ctrl=ctrl, plant=plant)
    assert s.query(pkg.QUERY_DEVICE_BYTES) == before
    got = s.loop_run_sensing(st, 0, sense, None, act, None, ground, pkg.push_params(4, 2), lp, ctrl=ctrl, plant=plant, trace=True)      # ticks = 0: the buffers only
    assert _same(got[0], st) and _same(got[1], pkg.loop_outcomes(4, lib)) and _same(got[2], pkg.ground_tallies(4))
    assert _same(got[3], pkg.actuation_lines(4)) and _same(got[4], pkg.sense_seen(4))      # nothing was launched
    assert s.query(pkg.QUERY_DEVICE_BYTES) - before == (256 + 128) * 1000
    s.loop_run_sensing(st, 3, sense, None, None, None, None, None, lp, plant=plant)
    s.loop_run_actuation(st, 3, act, None, ground, pkg.push_params(4, 2), lp, ctrl=ctrl, plant=plant)
    s.loop_run_ground(st, 3, ground, pkg.push_params(4, 2), lp, ctrl=ctrl, plant=plant)
    s.loop_run_instances(st, 3, lp, ctrl=ctrl, plant=plant)
    assert s.query(pkg.QUERY_DEVICE_BYTES) - before == (256 + 128) * 1000
    s.close()
    # a handle that only ever made sensing calls without an actuation record has no staging for one
    s = pkg.Solver(p, 1000, device=0, lib=lib)
    s.prepare(4)
    s.loop_run_pushes(st, 3, pkg.push_params(4, 2), lp, ctrl=ctrl, plant=plant)
    before = s.query(pkg.QUERY_DEVICE_BYTES)
    s.loop_run_sensing(st, 0, sense, None, None, None, None, pkg.push_params(4, 2), lp, ctrl=ctrl, plant=plant)
    assert s.query(pkg.QUERY_DEVICE_BYTES) - before == (256 + 128) * 1000
    s.close()
