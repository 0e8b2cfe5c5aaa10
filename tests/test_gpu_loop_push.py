"""GPU suite (-m gpu): timed push windows per robot in the device closed loop (qmpc_loop_run_pushes*, include/qmpc.h; DESIGN.md
section 3n).

The call is qmpc_loop_run_outcomes* whose plant step integrates under the effective wrench of the tick.  Windows that never act give
that call's bytes; a one-tick window changes the state by the impulse identities of tests/native/loop_push_host.cpp, in the tick it
names and in no other; a window over the whole run is the plant's constant disturbance; launch forms, splits over calls, device
buffers and the lane tick give the same bytes; a population whose fate is derived falls when and only when it must; the host twin
agrees; refusals and invalid windows are those of the outcome call and of an invalid plant record.  Every case is N = 10; sizes with
two launch forms run once per form: 96 robots (persistent kernel) and 3000 (per-tick graph on the wave kernels)."""
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
COUNTERS = ("ticks", "down_tick", "not_ok_ticks", "rejected_ticks", "first_rejected_tick")
FORMS = [(96, "persistent"), (3000, "per_tick")]


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _all_same(got, want):
    return len(got) == len(want) and all(_same(a, b) for a, b in zip(got, want))


def _fleet(pkg, lib, B, seed=1):
    """B robots at their initial poses, walking from the first tick with the commands of tests/test_gpu_loop_outcome.py"""
    lp = pkg.default_loop_params(lib)
    rng = np.random.default_rng(seed)
    cmds = np.array([COMMANDS[i % len(COMMANDS)] for i in range(B)])
    cmds[:, 0] += rng.uniform(-0.1, 0.1, B) * cmds[:, 6]
    stand = cmds.copy(); stand[:, 6] = 0.0
    st = pkg.loop_states(stand, lp, height=0.3, yaw=rng.uniform(-3, 3, B), lib=lib)
    st["movement_mode"] = cmds[:, 6]
    return lp, st


def _records(pkg, p, B, kind, seed=5):
    ctrl = plant = None
    if kind == "both":
        ctrl = pkg.random_go1_variants(B, seed=seed, base=p)
        ctrl["mu"] = np.maximum(ctrl["mu"], 0.5)
        plant = pkg.random_go1_plants(B, seed=seed + 1, base=p, payload=(-1.0, 3.0), force=(0.0, 10.0))
    return ctrl, plant


def _shoves(pkg, lp, B, seed, per_robot, starts, lengths):
    """per_robot windows per robot: window k starts at starts[k] and lasts lengths[k] ticks; impulses of 0.5 .. 3 N s in random
    horizontal directions (random_go1_pushes) and a yaw torque on every third robot's last window"""
    push = pkg.random_go1_pushes(B, seed=seed, per_robot=per_robot, impulse=(0.5, 3.0), dt=lp.dt)
    for k in range(per_robot):
        push["force_world"][:, k] *= (push["ticks"][:, k] / lengths[k])[:, None]      # the same impulse over the new length
        push["start_tick"][:, k] = starts[k]
        push["ticks"][:, k] = lengths[k]
    push["torque_body"][::3, per_robot - 1, 2] = 1.5
    return push


# ---- 1. records that never act -------------------------------------------------------------------------------------------
def _never(pkg, kind, T):
    """one window that never acts in a run of ticks 0 .. T - 1, by its kind"""
    w = np.zeros((), dtype=pkg.PUSH_PARAMS_DTYPE)
    w["force_world"], w["torque_body"] = [300.0, -200.0, -500.0], [5.0, -5.0, 5.0]
    if kind == 0:      # zero (or negative) length, in the middle of the run
        w["start_tick"], w["ticks"] = 3.0, 0.0
    elif kind == 1:    # an active window, over the whole run, with a wrench of zeros of both signs
        w["start_tick"], w["ticks"] = 0.0, 1000.0
        w["force_world"], w["torque_body"] = [0.0, -0.0, 0.0], [-0.0, 0.0, -0.0]
    elif kind == 2:    # before tick 0: its last tick would be tick -1
        w["start_tick"], w["ticks"] = -8.0, 8.0
    elif kind == 3:    # beyond the run: its first tick is the one after the last
        w["start_tick"], w["ticks"] = float(T), 5.0
    else:              # a negative length
        w["start_tick"], w["ticks"] = 3.0, -4.0
    return w


@pytest.mark.parametrize("B,form", FORMS)
@pytest.mark.parametrize("kind", ["both", "neither"])
def test_windows_that_never_act_give_the_outcome_call(pkg, lib, B, form, kind):
    T = 20
    p = pkg.default_params(10, pkg.MODE_CONVERGED, lib)
    lp, st = _fleet(pkg, lib, B)
    ctrl, plant = _records(pkg, p, B, kind)
    op = pkg.default_outcome_params(lib)
    push = pkg.push_params(B, 2)      # robot i: the kinds i mod 5 and (i div 5) mod 5 -- every kind, alone and beside every other
    kinds = np.array([_never(pkg, k, T) for k in range(5)], dtype=pkg.PUSH_PARAMS_DTYPE)
    push[:, 0], push[:, 1] = kinds[np.arange(B) % 5], kinds[(np.arange(B) // 5) % 5]
    assert (push["ticks"] > 0).any() and (push["force_world"] != 0).any() and np.signbit(push["force_world"]).any()
    s = pkg.Solver(p, B, device=0, lib=lib)
    assert s.loop_instances_plan(B, ctrl is not None, False)[0] == form
    want = s.loop_run_outcomes(st, T, lp, ctrl=ctrl, plant=plant, op=op, trace=True)
    got = s.loop_run_pushes(st, T, push, lp, ctrl=ctrl, plant=plant, op=op, trace=True)
    none = s.loop_run_pushes(st, T, None, lp, ctrl=ctrl, plant=plant, op=op, trace=True)
    s.close()
    assert (want[0]["tick"] == T).all()
    assert _all_same(got, want)
    assert _all_same(none, want)


# ---- 2. timing and impulse on the device ---------------------------------------------------------------------------------
def _close3(d, e, tol):
    """|d - e| <= tol * (largest component of e), per robot: the bound of tests/native/loop_push_host.cpp"""
    return (np.abs(d - e) <= tol * np.abs(e).max(axis=1, keepdims=True)).all()


def test_a_one_tick_window_acts_in_its_tick_alone(pkg, lib):
    """64 standing robots of varied mass and inertia; a one-tick window at s = 0, 3, 7.  Through s ticks nothing differs from the
    unpushed run, byte for byte; after tick s + 1 the state differs by the impulse identities: the controller has seen nothing yet
    (same forces), the plant has no gyroscopic term and the midpoint attitude does not see the wrench.  1e-12 relative to the
    largest component: standing at |p| < 0.5 and |v|, |w| << 1 the two roundings of a difference are 6e-17 against
    dp >= 1/2 dt^2 250 N / 17 kg = 1.8e-4 (3e-13), and far less for dv and dw."""
    B, F, TAU = 64, np.array([300.0, -200.0, 250.0]), np.array([4.0, -3.0, 5.0])
    p = pkg.default_params(10, pkg.MODE_CONVERGED, lib)
    lp = pkg.default_loop_params(lib)
    st = pkg.loop_states([[0.0, 0.0, 0.30, 0.0, 0.0, 0.0, 0.0]] * B, lp, height=0.3, yaw=np.linspace(-3, 3, B), lib=lib)
    plant = pkg.random_go1_plants(B, seed=31, base=p, payload=(-1.0, 4.0))
    assert len(np.unique(plant["mass"])) == B and plant["mass"].max() < 17.0
    Iinv = np.linalg.inv(plant["inertia"].reshape(B, 3, 3))
    s = pkg.Solver(p, B, device=0, lib=lib)
    U = [st]
    for _ in range(8):
        U.append(s.loop_run_outcomes(U[-1], 1, lp, plant=plant)[0])
    assert (U[8]["tick"] == 8).all() and (U[8]["status"] == 0).all()
    for start in (0, 3, 7):
        for what in ("force", "torque"):
            push = pkg.push_params(B)
            push["start_tick"], push["ticks"] = float(start), 1.0
            push["force_world" if what == "force" else "torque_body"] = F if what == "force" else TAU
            before = s.loop_run_pushes(st, start, push, lp, plant=plant)[0]
            assert _same(before, U[start]), (start, what)
            after = s.loop_run_pushes(before, 1, push, lp, plant=plant)[0]      # state.tick is absolute: the window is this tick
            ref = U[start + 1]
            for k in after.dtype.names:      # everything the plant does not integrate is untouched
                if k not in ("pos_world", "quat", "lin_vel_world", "ang_vel_body"):
                    assert _same(after[k], ref[k]), (start, what, k)
            if what == "force":
                assert _same(after["quat"], ref["quat"]) and _same(after["ang_vel_body"], ref["ang_vel_body"])
                dv, dp = after["lin_vel_world"] - ref["lin_vel_world"], after["pos_world"] - ref["pos_world"]
                ev, ep = lp.dt * F[None] / plant["mass"][:, None], 0.5 * lp.dt ** 2 * F[None] / plant["mass"][:, None]
                print(f"start {start} force: worst relative error dv {np.abs(dv - ev).max() / np.abs(ev).max():.2e}, "
                      f"dp {np.abs(dp - ep).max() / np.abs(ep).max():.2e}")
                assert _close3(dv, ev, 1e-12) and _close3(dp, ep, 1e-12), (start, what)
            else:
                assert _same(after["lin_vel_world"], ref["lin_vel_world"])
                dw, ew = after["ang_vel_body"] - ref["ang_vel_body"], lp.dt * np.einsum("bij,j->bi", Iinv, TAU)
                print(f"start {start} torque: worst relative error dw {np.abs(dw - ew).max() / np.abs(ew).max():.2e}")
                assert _close3(dw, ew, 1e-12), (start, what)
            later = s.loop_run_pushes(after, 1, push, lp, plant=plant)[0]       # ... and the next tick is an unpushed one again:
            plain = s.loop_run_outcomes(after, 1, lp, plant=plant)[0]           # the outcome call from the same state
            assert _same(later, plain), (start, what)
    s.close()


# ---- 3. a window over the whole run is the plant's constant disturbance --------------------------------------------------
@pytest.mark.parametrize("B,form", FORMS)
def test_a_window_over_the_whole_run_is_the_constant_disturbance(pkg, lib, B, form):
    T = 30
    p = pkg.default_params(10, pkg.MODE_CONVERGED, lib)
    lp, st = _fleet(pkg, lib, B, seed=2)
    ctrl, plant = _records(pkg, p, B, "both", seed=12)      # horizontal forces: the z component is exactly zero
    plant["ext_torque_body"][::2, 2] = 0.4                  # a yaw torque on every second robot, no other torque component
    plant["ext_force_world"][::7] = 0.0                     # ... and robots without any force
    plant["ext_force_world"][3::7, 0] = -0.0
    quiet = plant.copy()
    quiet["ext_force_world"], quiet["ext_torque_body"] = 0.0, 0.0
    push = pkg.push_params(B)
    push["start_tick"], push["ticks"] = -3.0, T + 10.0
    push["force_world"], push["torque_body"] = plant["ext_force_world"][:, None], plant["ext_torque_body"][:, None]
    op = pkg.default_outcome_params(lib)
    s = pkg.Solver(p, B, device=0, lib=lib)
    assert s.loop_instances_plan(B, True, False)[0] == form
    want = s.loop_run_outcomes(st, T, lp, ctrl=ctrl, plant=plant, op=op, trace=True)
    got = s.loop_run_pushes(st, T, push, lp, ctrl=ctrl, plant=quiet, op=op, trace=True)
    calm = s.loop_run_outcomes(st, T, lp, ctrl=ctrl, plant=quiet, op=op, trace=True)
    s.close()
    assert (plant["ext_force_world"][:, 2] == 0).all() and (plant["ext_force_world"][:, 0] != 0).any()
    assert _all_same(got, want)
    assert not _same(calm[0], want[0])      # (the disturbance is felt)


# ---- 4. launch forms -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stop", ["nostop", "stop"])
def test_launch_forms_give_the_same_bytes(stop):
    worker = Path(__file__).resolve().parent / "_loop_push_worker.py"
    out = {}
    for fused in ("0", "1"):
        env = dict(os.environ, QMPC_LOOP_FUSED=fused)
        r = subprocess.run([sys.executable, str(worker), "200", "60", "10", stop], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.splitlines()
        out[fused] = tuple([l for l in lines if l.startswith(k)][0] for k in ("FORM", "OUTCOMES", "SHA"))
    print(out)
    f0, f1 = eval(out["0"][0][5:]), eval(out["1"][0][5:])
    assert f0[0] == "per_tick" and f1[0] == "persistent" and f0[1] == f1[1]      # the same solve variant in both forms
    assert out["0"][1] == out["1"][1] and out["0"][2] == out["1"][2]
    assert int(out["1"][1].split()[3]) >= 200 // 8      # the pressed robots went down


# ---- 5. accumulation over calls ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,form", FORMS)
def test_windows_span_calls_and_split_over_calls(pkg, lib, B, form):
    p = pkg.default_params(10, pkg.MODE_CONVERGED, lib)
    lp, st = _fleet(pkg, lib, B, seed=4)
    ctrl, plant = _records(pkg, p, B, "both", seed=8)
    op = pkg.default_outcome_params(lib, stop_when_down=True)
    s = pkg.Solver(p, B, device=0, lib=lib)
    assert s.loop_instances_plan(B, True, False)[0] == form
    run = lambda x, t, pu, oc=None: s.loop_run_pushes(x, t, pu, lp, ctrl=ctrl, plant=plant, op=op, outcomes=oc, trace=True)      # noqa: E731
    # windows straddling tick 20 (ticks 15 .. 24, and ticks 18 .. 21 on top): one call of 60 ticks is 20 + 40 with the same records
    over = _shoves(pkg, lp, B, 41, 2, (15.0, 18.0), (10.0, 4.0))
    whole = run(st, 60, over)
    a = run(st, 20, over)
    b = run(a[0], 40, over, a[1])
    assert _same(whole[0], b[0]) and _same(whole[1], b[1])
    assert _same(whole[2], np.concatenate([a[2], b[2]])) and _same(whole[3], np.concatenate([a[3], b[3]]))
    # two disjoint windows (ticks 5 .. 11 and 30 .. 37) are two calls of one window each, each carrying the window that falls in it
    apart = _shoves(pkg, lp, B, 42, 2, (5.0, 30.0), (7.0, 8.0))
    both = run(st, 60, apart)
    c = run(st, 20, apart[:, :1])
    d = run(c[0], 40, apart[:, 1:], c[1])
    calm = s.loop_run_outcomes(st, 60, lp, ctrl=ctrl, plant=plant, op=op)
    s.close()
    assert _same(both[0], d[0]) and _same(both[1], d[1])
    assert _same(both[2], np.concatenate([c[2], d[2]])) and _same(both[3], np.concatenate([c[3], d[3]]))
    assert not _same(both[0], calm[0]) and not _same(whole[0], both[0])      # (the shoves are felt, and differ)


# ---- 6. a population whose fate is known ---------------------------------------------------------------------------------
def _classes(pkg, lib, B):
    """Standing robots as in _falling of tests/test_gpu_loop_outcome.py (12.84 kg, 4 x fz_max = 400 N of lift at most), classes by
    i mod 4: 0 no push; 1 -1000 N in z from tick 0 for 30 ticks; 2 the same from tick 10; 3 100 N lateral for one tick at tick 5"""
    p = pkg.default_params(10, pkg.MODE_CONVERGED, lib)
    assert abs(p.mass - 12.84) < 1e-12 and p.fz_max == 100.0
    lp = pkg.default_loop_params(lib)
    st = pkg.loop_states([[0.0, 0.0, 0.30, 0.0, 0.0, 0.0, 0.0]] * B, lp, height=0.3, yaw=np.linspace(-3, 3, B), lib=lib)
    cls = np.arange(B) % 4
    push = pkg.push_params(B)
    push["force_world"][cls == 1, 0, 2] = push["force_world"][cls == 2, 0, 2] = -1000.0
    push["ticks"][cls == 1], push["ticks"][cls == 2] = 30.0, 30.0
    push["start_tick"][cls == 2] = 10.0
    push["force_world"][cls == 3, 0, 1] = 100.0
    push["start_tick"][cls == 3], push["ticks"][cls == 3] = 5.0, 1.0
    return p, lp, st, push, cls


@pytest.mark.parametrize("B,form", FORMS)
def test_a_population_whose_fate_is_known(pkg, lib, B, form):
    T = 45
    p, lp, st, push, cls = _classes(pkg, lib, B)
    plant = pkg.plant_params(p, B)
    s = pkg.Solver(p, B, device=0, lib=lib)
    assert s.loop_instances_plan(B, False, False)[0] == form
    go = pkg.default_outcome_params(lib)
    x6, oc = s.loop_run_pushes(st, 6, push, lp, plant=plant, op=go)
    u6 = s.loop_run_outcomes(st, 6, lp, plant=plant, op=go)[0]      # the same robots unpushed: what class 0 does in their place
    x10, oc = s.loop_run_pushes(x6, 4, push, lp, plant=plant, op=go, outcomes=oc)
    fin, oc = s.loop_run_pushes(x10, T - 10, push, lp, plant=plant, op=go, outcomes=oc)
    halt = s.loop_run_pushes(st, T, push, lp, plant=plant, op=pkg.default_outcome_params(lib, stop_when_down=True), trace=True)
    s.close()
    dt = oc["down_tick"]
    print(f"B={B} {form}: down ticks class 1 {sorted(set(dt[cls == 1].astype(int).tolist()))}, class 2 "
          f"{sorted(set(dt[cls == 2].astype(int).tolist()))}; class 0 at tick 10: |z - 0.3| <= "
          f"{np.abs(x10['pos_world'][cls == 0, 2] - 0.3).max():.2e} m, |vz| <= {np.abs(x10['lin_vel_world'][cls == 0, 2]).max():.2e} m/s")
    # class 2 starts its fall at tick 10 from where class 0 stands then: within 5 mm of 0.30 m and slower than 0.05 m/s vertically, under
    # which the drop time of 11.7 .. 14.6 ticks moves by under 3 %
    assert (np.abs(x10["pos_world"][cls == 0, 2] - 0.30) < 0.005).all() and (np.abs(x10["lin_vel_world"][cls == 0, 2]) < 0.05).all()
    assert (dt[cls == 0] == -1).all() and (dt[cls == 3] == -1).all()
    assert ((10 <= dt[cls == 1]) & (dt[cls == 1] <= 18)).all()
    assert ((20 <= dt[cls == 2]) & (dt[cls == 2] <= 28)).all()
    assert pkg.summarize_outcomes(oc)["down"] * 2 == B
    assert (fin["tick"] == T).all() and (oc["ticks"][dt < 0] == T).all() and (oc["ticks"][dt >= 0] == dt[dt >= 0]).all()
    # class 3: byte-identical to the unpushed robot through tick 5, then shoved by dv = dt F / m = 0.039 m/s sideways
    c3 = cls == 3
    x5 = x6      # (states after 6 ticks: the window acted in the tick 5 -> 6)
    assert not _same(x5["lin_vel_world"][c3], u6["lin_vel_world"][c3])
    dv = x5["lin_vel_world"][c3] - u6["lin_vel_world"][c3]
    assert np.abs(dv[:, 1] - lp.dt * 100.0 / 12.84).max() <= 1e-12 and _same(dv[:, 0], np.zeros(c3.sum())) and _same(dv[:, 2], np.zeros(c3.sum()))
    assert _same(x6[cls == 0], u6[cls == 0]) and _same(x6[cls == 2], u6[cls == 2])
    # stop_when_down: the same records; a halted robot stays at its down tick, its trace rows are zero from there on
    hx, ho, hf, hc = halt
    assert _same(ho, oc)
    down = dt >= 0
    assert (hx["tick"][down] == dt[down]).all() and (hx["tick"][~down] == T).all() and _same(hx[~down], fin[~down])
    for i in np.flatnonzero(down)[:96]:
        k = int(dt[i])
        assert (hf[k:, i] == 0).all() and (hc[k:, i] == 0).all() and (hf[:k, i] != 0).any(), i


# ---- 7. the lane tick ----------------------------------------------------------------------------------------------------
def test_lane_tick_with_uniform_controller_records(pkg, lib):
    """20480 robots under QMPC_INSTANCES_AUTO: uniform controller records + pushes against no controller records + pushes, the
    contract of DESIGN.md section 3l for uniform records.  Two calls of 12 ticks on the falling classes with stop_when_down: class 1
    goes down by tick 18, so the second call's sort has its idle class filled."""
    B, T = 20480, 12
    p, lp, st, push, cls = _classes(pkg, lib, B)
    ctrl = pkg.instance_params(p, B)
    op = pkg.default_outcome_params(lib, stop_when_down=True)
    s = pkg.Solver(p, B, device=0, lib=lib)
    s.set_instances_policy("auto")
    assert s.loop_instances_plan(B, True, False)[0] == "per_tick" and s.loop_instances_plan(B, True, False)[1].startswith("lane")
    w1 = s.loop_run_pushes(st, T, push, lp, op=op)
    g1 = s.loop_run_pushes(st, T, push, lp, ctrl=ctrl, op=op)
    assert pkg.KERNEL_FAMILY[s.query(pkg.QUERY_LAST_KERNEL)].startswith("lane")
    w2 = s.loop_run_pushes(w1[0], T, push, lp, op=op, outcomes=w1[1])
    g2 = s.loop_run_pushes(g1[0], T, push, lp, ctrl=ctrl, op=op, outcomes=g1[1])
    s.close()
    assert _all_same(g1, w1) and _all_same(g2, w2)
    dt = g2[1]["down_tick"]
    assert ((10 <= dt[cls == 1]) & (dt[cls == 1] <= 18)).all() and (dt[cls == 0] == -1).all() and (dt[cls == 3] == -1).all()
    assert (g2[0]["tick"][cls == 1] == dt[cls == 1]).all() and (g2[0]["tick"][cls == 0] == 2 * T).all()


# ---- 8. device buffers ---------------------------------------------------------------------------------------------------
def test_device_buffers_give_the_host_call(pkg, lib):
    import torch

    B, T = 48, 25
    p = pkg.default_params(10, pkg.MODE_CONVERGED, lib)
    lp, st = _fleet(pkg, lib, B, seed=6)
    ctrl, plant = _records(pkg, p, B, "both", seed=2)
    push = _shoves(pkg, lp, B, 43, 3, (2.0, 6.0, 15.0), (5.0, 3.0, 6.0))
    push["force_world"][5, 0] = [0.0, 0.0, -1000.0]; push["ticks"][5, 0] = 30.0      # one robot falls
    op = pkg.default_outcome_params(lib, stop_when_down=True)
    s = pkg.Solver(p, B, device=0, lib=lib)
    want = s.loop_run_pushes(st, T, push, lp, ctrl=ctrl, plant=plant, op=op, trace=True)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1).copy()).cuda()      # noqa: E731
    d_st, d_oc, d_ctrl, d_plant, d_push = dev(st), dev(pkg.loop_outcomes(B, lib)), dev(ctrl), dev(plant), dev(push)
    d_tf = torch.full((T, B, 12), 7.0, dtype=torch.float64, device="cuda")
    d_tc = torch.full((T, B, 4), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s.loop_run_pushes_device(B, d_st.data_ptr(), T, d_oc.data_ptr(), d_push.data_ptr(), 3, lp, op, d_ctrl=d_ctrl.data_ptr(),
                             d_plant=d_plant.data_ptr(), d_trace_forces=d_tf.data_ptr(), d_trace_contacts=d_tc.data_ptr())
    s.wait()
    s.close()
    assert d_st.cpu().numpy().tobytes() == want[0].tobytes() and d_oc.cpu().numpy().tobytes() == want[1].tobytes()
    assert _same(d_tf.cpu().numpy(), want[2]) and _same(d_tc.cpu().numpy(), want[3])
    assert d_push.cpu().numpy().tobytes() == push.tobytes()      # read in place, not written
    assert want[1]["down_tick"][5] > 0


# ---- 9. the host class ---------------------------------------------------------------------------------------------------
def _host(pkg):
    import __graft_entry__ as g

    host = C.CDLL(str(g.build_host()))
    vp = C.c_void_p
    host.qh_loop_create_robot.argtypes = [C.c_char_p, C.c_int, vp, vp, vp, vp]
    host.qh_loop_create_robot.restype = vp
    for f in ("qh_loop_tick", "qh_loop_destroy", "qh_loop_device_status"):
        getattr(host, f).argtypes = [vp]
    host.qh_loop_outcome.argtypes = [vp, vp]
    host.qh_loop_export.argtypes = [vp, vp]
    host.qh_loop_set_pushes.argtypes = [vp, vp, C.c_int]
    host.qh_loop_set_command.argtypes = [vp, vp, C.c_double]
    return host


def test_host_class_under_pushes(pkg, lib):
    """Six robots, 60 ticks (6 standing, 54 on their commands), a lateral shove and a yaw-torque shove among them, against the host
    twin (host/ClosedLoopHost.h: the same tick on the CPU through loop_push_wrench and plant_step_ext; without a plant record on
    the handle's mass and inverse inertia).  Counters equal; fields to the tolerances of test_host_class_records."""
    N, T0, T, B = 10, 6, 54, 6
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    lp = pkg.default_loop_params(lib)
    cmds = np.array(COMMANDS)
    cmds[:, 6] = 1.0
    stand = cmds.copy(); stand[:, 6] = 0.0
    st = pkg.loop_states(stand, lp, height=0.3, yaw=np.linspace(-2, 2, B), lib=lib)
    push = pkg.push_params(B, 2)
    push[1, 0] = (20.0, 6.0, [0.0, 60.0, 0.0], [0.0, 0.0, 0.0])       # lateral: 1.8 N s
    push[2, 1] = (30.0, 5.0, [0.0, 0.0, 0.0], [0.0, 0.0, 3.0])        # yaw torque
    push[3, 0] = (12.0, 4.0, [-40.0, 30.0, 0.0], [0.0, 0.0, 0.0])     # both, overlapping
    push[3, 1] = (14.0, 6.0, [0.0, 20.0, 0.0], [0.5, 0.0, -2.0])
    push[4, 0] = (3.0, 2.0, [50.0, 0.0, 0.0], [0.0, 0.0, 0.0])        # while standing
    results = {}
    for with_plant in (True, False):
        plant = pkg.plant_params(p, B) if with_plant else None
        if with_plant:
            plant["mass"][1] += 2.0
            plant["ext_force_world"][3] = [0.0, 8.0, 0.0]
        s = pkg.Solver(p, B, device=0, lib=lib)
        x, oc = s.loop_run_pushes(st, T0, push, lp, plant=plant)
        x["movement_mode"] = cmds[:, 6]
        fin, oc = s.loop_run_pushes(x, T, push, lp, plant=plant, outcomes=oc)
        y, calm = s.loop_run_outcomes(st, T0, lp, plant=plant)
        y["movement_mode"] = cmds[:, 6]
        calm = s.loop_run_outcomes(y, T, lp, plant=plant, outcomes=calm)[1]
        s.close()
        host = _host(pkg)
        ho = pkg.loop_outcomes(B, lib)
        hs = np.zeros(B, dtype=pkg.LOOP_STATE_DTYPE)
        for i in range(B):
            h = host.qh_loop_create_robot(str(pkg.LIB_PATH).encode(), N, C.addressof(lp), st[i:i + 1].ctypes.data, None,
                                          plant[i:i + 1].ctypes.data if with_plant else None)
            assert h and host.qh_loop_device_status(h) == 0
            host.qh_loop_set_pushes(h, push[i].ctypes.data, 2)
            for _ in range(T0):
                assert host.qh_loop_tick(h) == 1
            host.qh_loop_set_command(h, np.ascontiguousarray(cmds[i, :6]).ctypes.data, float(cmds[i, 6]))
            for t in range(T):
                assert host.qh_loop_tick(h) == 1, (i, t)
            host.qh_loop_outcome(h, ho[i:i + 1].ctypes.data)
            host.qh_loop_export(h, hs[i:i + 1].ctypes.data)
            host.qh_loop_destroy(h)
        for k in COUNTERS:
            assert np.array_equal(oc[k], ho[k]), (with_plant, k)
        worst = {k: float(np.abs(oc[k] - ho[k]).max()) for k in ("min_height", "min_upright", "max_height_err", "max_vel_err", "max_ang_vel",
                                                                "max_force_z", "sum_vel_err_sq")}
        worst_state = {k: float(np.abs(fin[k] - hs[k]).max()) for k in ("pos_world", "quat", "lin_vel_world", "ang_vel_body")}
        print("plant records" if with_plant else "no plant records", "device against host, worst differences:", worst,
              "final states (not asserted):", worst_state)
        for k in ("min_height", "min_upright", "max_height_err", "max_vel_err", "max_ang_vel"):
            assert worst[k] <= 1e-8, (with_plant, k, worst)
        assert worst["max_force_z"] <= 1e-6
        assert (np.abs(oc["sum_vel_err_sq"] - ho["sum_vel_err_sq"]) <= oc["ticks"] * 2 * oc["max_vel_err"] * 1e-8).all()
        assert (fin["tick"] == T0 + T).all() and (oc["ticks"][oc["down_tick"] < 0] == T0 + T).all()
        # the shoved robots felt it, the others are the unpushed run's, byte for byte
        assert all(oc[i].tobytes() != calm[i].tobytes() for i in range(1, 5))
        assert _same(oc[[0, 5]], calm[[0, 5]])
        results[with_plant] = oc
    assert not _same(results[True][1], results[False][1])


# ---- 10. refusals and invalid windows ------------------------------------------------------------------------------------
def test_refusals_invalid_windows_and_buffers(pkg, lib, monkeypatch):
    lp = pkg.default_loop_params(lib)
    st = pkg.loop_states([[0.0, 0.0, 0.3, 0.0, 0.0, 0.0, 0.0]] * 4, lp, lib=lib)
    p = pkg.default_params(10, pkg.MODE_CONVERGED, lib)
    ctrl, plant = pkg.instance_params(p, 4), pkg.plant_params(p, 4)
    push = pkg.push_params(4, 2)

    def code(s, pu=push, **kw):
        try:
            s.loop_run_pushes(kw.pop("st", st), 3, pu, kw.pop("lp", lp), **kw)
            return pkg.OK
        except pkg.QmpcError as e:
            return e.code

    def code_out(s, **kw):
        try:
            s.loop_run_outcomes(st, 3, kw.pop("lp", lp), **kw)
            return pkg.OK
        except pkg.QmpcError as e:
            return e.code

    warm = pkg.default_loop_params(lib); warm.warm_start = 1.0
    # the outcome call's refusals, unchanged
    sc = pkg.Solver(pkg.default_convex_params(20, pkg.MODE_CONVERGED, lib), 4, device=0, lib=lib)
    assert code(sc, plant=plant) == code_out(sc, plant=plant) == pkg.UNSUPPORTED and code(sc) == code(sc, pu=None) == pkg.UNSUPPORTED
    sc.close()
    sr = pkg.Solver(pkg.default_params(10, pkg.MODE_REFERENCE, lib), 4, device=0, lib=lib)
    assert code(sr, plant=plant) == code_out(sr, plant=plant) == pkg.UNSUPPORTED and code(sr) == pkg.UNSUPPORTED
    sr.close()
    s8 = pkg.Solver(pkg.default_biped8_params(16, pkg.MODE_CONVERGED, lib), 4, device=0, lib=lib)
    assert code(s8, plant=plant) == code_out(s8, plant=plant) == pkg.BAD_ARGUMENT and code(s8) == pkg.BAD_ARGUMENT
    s8.close()
    s = pkg.Solver(p, 4, device=0, lib=lib)
    assert code(s, ctrl=ctrl, lp=warm) == code_out(s, ctrl=ctrl, lp=warm) == pkg.UNSUPPORTED
    assert code(s, plant=plant, lp=warm) == pkg.OK and code(s, lp=warm) == pkg.OK and code(s) == pkg.OK and code(s, ctrl=ctrl) == pkg.OK
    # pushes_per_robot outside 1 .. QMPC_MAX_PUSHES
    assert code(s, pu=pkg.push_params(4, 0)) == pkg.BAD_ARGUMENT and code(s, pu=pkg.push_params(4, 9)) == pkg.BAD_ARGUMENT
    assert code(s, pu=pkg.push_params(4, 8)) == pkg.OK and code(s, pu=pkg.push_params(4, 1)) == pkg.OK
    big = pkg.loop_states([[0.0, 0.0, 0.3, 0.0, 0.0, 0.0, 0.0]] * 5, lp, lib=lib)
    assert code(s, st=big, pu=pkg.push_params(5, 2), plant=pkg.plant_params(p, 5)) == pkg.BATCH_TOO_LARGE
    s.close()
    # a NaN in one window freezes that robot, in both launch forms: state untouched but status and iterations, zero trace rows, the
    # outcome record's bytes untouched; everybody else has the bytes of the run where that window is valid and never acts
    B = 12
    lp2, st2 = _fleet(pkg, lib, B, seed=6)
    c2 = pkg.random_go1_variants(B, seed=7, base=p)
    c2["mu"] = np.maximum(c2["mu"], 0.5)
    p2 = pkg.random_go1_plants(B, seed=8, base=p, force=(0.0, 10.0))
    valid = _shoves(pkg, lp2, B, 44, 2, (3.0, 9.0), (4.0, 5.0))
    valid["ticks"][3, 1] = 0.0            # robot 3's second window never acts ...
    valid["ticks"][8, 0] = 0.0            # ... nor does robot 8's first
    bad = valid.copy()
    bad["force_world"][3, 1, 1] = np.nan  # ... and they are invalid all the same
    bad["start_tick"][8, 0] = np.inf
    marked = pkg.loop_outcomes(B, lib)
    raw = marked.view(np.uint8).reshape(B, 128)
    raw[3] = 0xA5
    raw[8] = np.frombuffer(np.full(16, np.nan).tobytes(), dtype=np.uint8)
    clean = pkg.loop_outcomes(B, lib)
    outs = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("QMPC_LOOP_FUSED", fused)
        s = pkg.Solver(p, B, device=0, lib=lib)
        assert s.loop_instances_plan(B, True, False)[0] == ("persistent" if fused == "1" else "per_tick")
        x, oc, tf, tc = s.loop_run_pushes(st2, 20, bad, lp2, ctrl=c2, plant=p2, outcomes=marked, trace=True)
        ref = s.loop_run_pushes(st2, 20, valid, lp2, ctrl=c2, plant=p2, outcomes=clean, trace=True)
        s.close()
        for i in (3, 8):
            assert oc[i].tobytes() == marked[i].tobytes() and x["status"][i] == pkg.BAD_PARAMS and x["iterations"][i] == 0
            frozen = st2[i:i + 1].copy()
            frozen["status"], frozen["iterations"] = x["status"][i], x["iterations"][i]
            assert x[i].tobytes() == frozen[0].tobytes()
            assert (tf[:, i] == 0).all() and (tc[:, i] == 0).all()
        others = [i for i in range(B) if i not in (3, 8)]
        assert (ref[0]["tick"] == 20).all() and (ref[1]["ticks"][others] == 20).all()
        assert _same(x[others], ref[0][others]) and _same(oc[others], ref[1][others])
        assert _same(tf[:, others], ref[2][:, others]) and _same(tc[:, others], ref[3][:, others])
        outs[fused] = (x, oc, tf, tc)
    monkeypatch.delenv("QMPC_LOOP_FUSED")
    assert _all_same(outs["0"], outs["1"])
    # buffers: the host-buffer push call stages the windows in a buffer of its own (64 B x pushes_per_robot x max_batch), allocated
    # by ticks = 0 too and grown with pushes_per_robot; no other call allocates it, the device-buffer call reads in place
    s = pkg.Solver(p, 1000, device=0, lib=lib)
    s.prepare(4)
    s.loop_run(st, 3, lp)
    s.loop_run_outcomes(st, 3, lp, ctrl=ctrl, plant=plant)
    before = s.query(pkg.QUERY_DEVICE_BYTES)
    s.loop_run_pushes(st, 3, None, lp, ctrl=ctrl, plant=plant)
    assert s.query(pkg.QUERY_DEVICE_BYTES) == before
    assert _same(s.loop_run_pushes(st, 0, pkg.push_params(4, 2), lp, ctrl=ctrl, plant=plant)[0], st)      # ticks = 0: the buffers only
    assert s.query(pkg.QUERY_DEVICE_BYTES) - before == 2 * 64 * 1000
    s.loop_run_pushes(st, 3, pkg.push_params(4, 2), lp, ctrl=ctrl, plant=plant)
    s.loop_run_pushes(st, 3, pkg.push_params(4, 1), lp, plant=plant)
    assert s.query(pkg.QUERY_DEVICE_BYTES) - before == 2 * 64 * 1000
    s.loop_run_pushes(st, 3, pkg.push_params(4, 5), lp)
    assert s.query(pkg.QUERY_DEVICE_BYTES) - before == 5 * 64 * 1000
    s.loop_run_outcomes(st, 3, lp, ctrl=ctrl, plant=plant)
    s.loop_run_instances(st, 3, lp, ctrl=ctrl, plant=plant)
    assert s.query(pkg.QUERY_DEVICE_BYTES) - before == 5 * 64 * 1000
    s.close()
