"""GPU suite (-m gpu): per-robot outcome records of the closed loop (qmpc_loop_run_outcomes*, include/qmpc.h).

The call is qmpc_loop_run_instances* -- the same states and traces, bit for bit -- and accumulates a 128-byte record per robot on
the device inside the tick: when the robot went down, its worst height, tilt and tracking errors, its solves' statuses.  The
records are checked against a restatement in numpy from the states of one-tick calls of the EXISTING entry point, across the
launch forms, across calls, on a population that certainly falls, with stop_when_down, and against the host twin."""
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
SELECTED = ("min_height", "max_force_z", "max_ang_vel", "iterations_sum", "iterations_max")      # selections / sums of stored values
DERIVED = ("min_upright", "max_height_err", "max_vel_err", "sum_vel_err_sq")


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _fleet(pkg, lib, B, seed=1):
    """B robots standing at their initial poses (movement 0) and the commands they walk with afterwards"""
    lp = pkg.default_loop_params(lib)
    rng = np.random.default_rng(seed)
    cmds = np.array([COMMANDS[i % len(COMMANDS)] for i in range(B)])
    cmds[:, 0] += rng.uniform(-0.1, 0.1, B) * cmds[:, 6]
    stand = cmds.copy(); stand[:, 6] = 0.0
    st = pkg.loop_states(stand, lp, height=0.3, yaw=rng.uniform(-3, 3, B), lib=lib)
    return lp, st, cmds


def _records(pkg, p, B, kind, seed=5):
    """the controller and plant records of a fleet: kind in both / ctrl / plant / neither; with plant records every 16th robot is
    pressed down with 1000 N (it falls within 20 ticks, see test_a_population_that_certainly_falls)"""
    ctrl = plant = None
    if kind in ("both", "ctrl"):
        ctrl = pkg.random_go1_variants(B, seed=seed, base=p)
        ctrl["mu"] = np.maximum(ctrl["mu"], 0.5)
    if kind in ("both", "plant"):
        plant = pkg.random_go1_plants(B, seed=seed + 1, base=p, payload=(-1.0, 3.0), force=(0.0, 10.0))
        plant["ext_force_world"][3::16, 2] = -1000.0
    return ctrl, plant


def _chunks(s, st, T, lp, ctrl, plant):
    """T one-tick calls of the existing qmpc_loop_run_instances: the states after every tick"""
    seq = []
    for _ in range(T):
        st = s.loop_run_instances(st, 1, lp, ctrl=ctrl, plant=plant)
        seq.append(st)
    return seq


def _first_max(cols):
    """the running maximum as the record takes it: from -inf, a later value replaces the held one only when it is greater"""
    cur = np.full(len(cols), -np.inf)
    for c in cols.T:
        take = c > cur
        cur[take] = c[take]
    return cur


def _restate(pkg, lib, seq, op, start=None):
    """the outcome records of the state sequence seq, restated in numpy from include/qmpc.h's definitions"""
    o = pkg.loop_outcomes(len(seq[0]), lib) if start is None else start.copy()
    for s in seq:
        live = o["down_tick"] < 0
        h = s["pos_world"][:, 2]
        w, x, y, z = (s["quat"][:, k] for k in range(4))
        R = np.empty((len(s), 3, 3))      # Eigen's toRotationMatrix
        R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - w * z); R[:, 0, 2] = 2 * (x * z + w * y)
        R[:, 1, 0] = 2 * (x * y + w * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - w * x)
        R[:, 2, 0] = 2 * (x * z - w * y); R[:, 2, 1] = 2 * (y * z + w * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
        up = R[:, 2, 2]
        vb = np.einsum("bji,bj->bi", R, s["lin_vel_world"])      # R' v
        e = vb[:, :2] - s["lin_vel_d_rel"][:, :2]
        e2 = (e * e).sum(axis=1)
        with np.errstate(invalid="ignore"):
            ev = np.sqrt(e2)
            he = np.abs(h - s["joy"][:, 2])
            wmax = _first_max(np.abs(s["ang_vel_body"]))
            fz = _first_max(s["forces_body"][:, 2::3])
            o["ticks"] += live
            for k, v, less in (("min_height", h, True), ("min_upright", up, True), ("max_height_err", he, False),
                               ("max_vel_err", ev, False), ("max_ang_vel", wmax, False), ("max_force_z", fz, False),
                               ("iterations_max", s["iterations"], False)):
                take = live & ((v < o[k]) if less else (v > o[k]))      # a NaN selects nothing
                o[k][take] = v[take]
            o["sum_vel_err_sq"][live] += e2[live]
            o["iterations_sum"][live] += s["iterations"][live]
            not_ok = live & (s["status"] != pkg.OK)
            rejected = not_ok & (s["status"] != pkg.MAX_ITER)
            o["not_ok_ticks"] += not_ok
            o["rejected_ticks"] += rejected
            first = rejected & (o["first_rejected_tick"] < 0)
            o["first_rejected_tick"][first] = s["tick"][first]
            down = live & ~(np.isfinite(h) & np.isfinite(up) & (h >= op.down_height) & (up >= op.down_upright))
        o["down_tick"][down] = s["tick"][down]
    return o


def _assert_restated(got, want, what):
    for k in COUNTERS:
        assert np.array_equal(got[k], want[k]), (what, k, np.flatnonzero(got[k] != want[k])[:8])
    for k in SELECTED:
        assert _same(got[k], want[k]), (what, k)
    worst = {}
    for k in DERIVED:
        d = np.abs(got[k] - want[k]) / np.maximum(1.0, np.abs(want[k]))
        d[(got[k] == want[k]) | (np.isnan(got[k]) & np.isnan(want[k]))] = 0.0      # infinities of an empty record, NaN sums
        worst[k] = float(d.max())
    print(what, "derived fields, worst relative difference:", worst)
    assert max(worst.values()) <= 1e-12, (what, worst)
    assert (got["reserved"] == 0).all()


_cache = {}


def _case(pkg, lib, B, kind):
    """one fleet: 6 ticks standing, then T ticks walking -- in T one-tick calls of the existing entry point, in one T-tick call of
    it, and in one T-tick outcome call; cached per (B, kind)"""
    if (B, kind) in _cache:
        return _cache[(B, kind)]
    N, T = 10, 30
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    lp, st, cmds = _fleet(pkg, lib, B)
    ctrl, plant = _records(pkg, p, B, kind)
    op = pkg.default_outcome_params(lib)
    op.down_height = 0.29      # the caller's threshold: robots commanded to 0.27 / 0.28 m cross it while the others walk on
    s = pkg.Solver(p, B, device=0, lib=lib)
    st0 = s.loop_run_instances(st, 6, lp, ctrl=ctrl, plant=plant)
    st0["movement_mode"] = cmds[:, 6]
    seq = _chunks(s, st0, T, lp, ctrl, plant)
    ref = s.loop_run_instances(st0, T, lp, ctrl=ctrl, plant=plant, trace=True)
    got = s.loop_run_outcomes(st0, T, lp, ctrl=ctrl, plant=plant, op=op, trace=True)
    form = s.loop_instances_plan(B, ctrl is not None, False)
    s.close()
    # (the restatement now, not the 30 x B states: the cache lives as long as the module)
    _cache[(B, kind)] = (seq[-1], _restate(pkg, lib, seq, op), ref, got, form, plant)
    return _cache[(B, kind)]


CASES = [(B, kind) for B in (96, 1024, 3000) for kind in ("both", "ctrl", "plant", "neither")]


@pytest.mark.parametrize("B,kind", CASES)
def test_records_equal_their_restatement_from_one_tick_calls(pkg, lib, B, kind):
    last, want, ref, got, form, plant = _case(pkg, lib, B, kind)
    assert form[0] == ("per_tick" if B > 2048 else "persistent")
    assert _same(last, ref[0])      # chunked cold calls are one call (the premise of the restatement)
    oc = got[1]
    down = oc["down_tick"] >= 0
    print(f"B={B} {kind} {form}: {int(down.sum())} robots down, down ticks {sorted(set(oc['down_tick'][down].astype(int).tolist()))[:12]}")
    _assert_restated(oc, want, f"B={B} {kind}")
    assert (oc["ticks"][~down] == 30).all() and (oc["ticks"][down] == oc["down_tick"][down] - 6).all()
    if plant is not None:      # the pressed robots went down, and not only they were evaluated
        assert down[3::16].all() and not down.all()


@pytest.mark.parametrize("B,kind", CASES)
def test_outcomes_change_nothing_else(pkg, lib, B, kind):
    last, want, ref, got, form, plant = _case(pkg, lib, B, kind)
    assert _same(got[0], ref[0]) and _same(got[2], ref[1]) and _same(got[3], ref[2])
    assert (ref[0]["tick"] == 36).all() and (ref[2] == 0).any()      # everybody ticked, swing phases happened


@pytest.mark.parametrize("robots,ticks,horizon,ctrl,warm,stop", [(200, 60, 10, "ctrl", "cold", "nostop"), (200, 60, 10, "noctrl", "warm", "stop"),
                                                                (96, 40, 20, "ctrl", "cold", "stop")])
def test_launch_forms_give_the_same_records(robots, ticks, horizon, ctrl, warm, stop):
    worker = Path(__file__).resolve().parent / "_loop_outcome_worker.py"
    out = {}
    for fused in ("0", "1"):
        env = dict(os.environ, QMPC_LOOP_FUSED=fused)
        r = subprocess.run([sys.executable, str(worker), str(robots), str(ticks), str(horizon), ctrl, warm, stop], env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.splitlines()
        out[fused] = tuple([l for l in lines if l.startswith(k)][0] for k in ("FORM", "OUTCOMES", "SHA"))
    print(out)
    f0, f1 = eval(out["0"][0][5:]), eval(out["1"][0][5:])
    assert f0[0] == "per_tick" and f1[0] == "persistent" and f0[1] == f1[1]      # the same solve variant in both forms
    assert out["0"][1] == out["1"][1] and out["0"][2] == out["1"][2]
    assert int(out["1"][1].split()[3]) >= robots // 8      # the pressed robots and the NaN robot went down


def test_lane_kernel_records_against_the_wave_form(pkg, lib):
    """32768 robots with plant records (the per-tick form on the lane kernel and its hand-off) against their first 1024 run as a
    shard of their own (the persistent wave kernel), with stop_when_down: a halted robot's NaN record is rejected by the lane
    kernel too.  Both run in one-tick calls on one outcome buffer (test_accumulation_across_calls: the same records) so that the
    statuses of every tick are known: where they agree the counters agree; where every solve of both runs converged (an iterate
    at the iteration cap is the kernel family's own) the continuous fields agree to the 1e-7 the cross-family tests use for
    forces and states.  Iteration counts are the kernel family's own."""
    N, B, S, T = 10, 32768, 1024, 20
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    lp, st, cmds = _fleet(pkg, lib, B, seed=10)
    plant = pkg.random_go1_plants(B, seed=11, base=p, payload=(-1.0, 3.0), force=(0.0, 10.0))
    plant["ext_force_world"][3::16, 2] = -1000.0
    op = pkg.default_outcome_params(lib, stop_when_down=True)
    st["movement_mode"] = cmds[:, 6]
    runs = {}
    for name, n in (("lane", B), ("wave", S)):
        s = pkg.Solver(p, n, device=0, lib=lib)
        form = s.loop_instances_plan(n, False, False)
        x, oc, statuses = st[:n], None, []
        for _ in range(T):
            x, oc = s.loop_run_outcomes(x, 1, lp, plant=plant[:n], op=op, outcomes=oc)
            statuses.append(x["status"][:S].copy())
        family = pkg.KERNEL_FAMILY[s.query(pkg.QUERY_LAST_KERNEL)]
        s.close()
        runs[name] = (x[:S], oc[:S], np.array(statuses), form, family)
    xl, ol, sl, fl, kl = runs["lane"]
    xw, ow, sw, fw, kw = runs["wave"]
    assert fl[0] == "per_tick" and fl[1] in ("lane", "lane_handoff") and kl == fl[1] and fw[0] == "persistent"
    agree = (sl == sw).all(axis=0)
    down = ol["down_tick"] >= 0
    print(f"lane {fl} vs wave {fw}: statuses agree for {int(agree.sum())} of {S} robots, {int(down.sum())} down")
    conv = ((sl == pkg.OK) & (sw == pkg.OK)).all(axis=0)
    assert agree.mean() > 0.9 and conv.mean() > 0.8 and down[3::16].all() and not down.all()
    for k in COUNTERS:
        assert np.array_equal(ol[k][agree], ow[k][agree]), k
    assert (xl["tick"][down] == ol["down_tick"][down]).all() and (xl["tick"][~down] == T).all()
    worst = {}
    for k in ("min_height", "min_upright", "max_height_err", "max_vel_err", "sum_vel_err_sq", "max_ang_vel", "max_force_z"):
        d = np.abs(ol[k] - ow[k]) / np.maximum(1.0, np.abs(ow[k]))
        worst[k] = float(d[conv].max())
    print("worst relative differences:", worst)
    assert max(worst.values()) <= 1e-7, worst
    for k in ("pos_world", "quat", "lin_vel_world", "ang_vel_body"):
        assert np.abs(xl[k][conv] - xw[k][conv]).max() <= 1e-7, k


def _falling(pkg, lib, B):
    """Half the robots carry ext_force_world[2] = -1000 N, the other half are their controller's robot; all stand at 0.3 m.
    m = 12.84 kg (weight 126 N), 4 x fz_max = 400 N, so the lift lies in [0, 400 N]: the net downward acceleration of a loaded
    robot is 56.5 .. 87.7 m/s^2 and 0.15 m of drop take 11.7 .. 14.6 ticks of 5 ms."""
    p = pkg.default_params(10, pkg.MODE_CONVERGED, lib)
    assert abs(p.mass - 12.84) < 1e-12 and p.fz_max == 100.0
    lp = pkg.default_loop_params(lib)
    st = pkg.loop_states([[0.0, 0.0, 0.30, 0.0, 0.0, 0.0, 0.0]] * B, lp, height=0.3, yaw=np.linspace(-3, 3, B), lib=lib)
    plant = pkg.plant_params(p, B)
    loaded = np.arange(B) % 2 == 1
    plant["ext_force_world"][loaded, 2] = -1000.0
    return p, lp, st, plant, loaded


@pytest.mark.parametrize("B", [64, 2500])
def test_a_population_that_certainly_falls(pkg, lib, B):
    p, lp, st, plant, loaded = _falling(pkg, lib, B)
    s = pkg.Solver(p, B, device=0, lib=lib)
    fin, oc = s.loop_run_outcomes(st, 40, lp, plant=plant, op=pkg.default_outcome_params(lib))
    form = s.loop_instances_plan(B, False, False)
    s.close()
    dt = oc["down_tick"]
    print(f"B={B} {form}: down ticks of the loaded half {sorted(set(dt[loaded].astype(int).tolist()))}, lowest height of the other half "
          f"{oc['min_height'][~loaded].min():.4f}, summary {pkg.summarize_outcomes(oc)}")
    assert loaded.sum() * 2 == B == (~loaded).sum() * 2
    assert ((10 <= dt[loaded]) & (dt[loaded] <= 18)).all()
    assert (dt[~loaded] == -1).all()
    assert (dt >= 0).sum() * 2 == B and (dt == -1).sum() * 2 == B
    assert (oc["ticks"][loaded] == dt[loaded]).all() and (oc["ticks"][~loaded] == 40).all() and (fin["tick"] == 40).all()
    assert pkg.summarize_outcomes(oc)["down"] * 2 == B


@pytest.mark.parametrize("B", [64, 2500])
def test_stop_when_down(pkg, lib, B):
    T = 40
    p, lp, st, plant, loaded = _falling(pkg, lib, B)
    s = pkg.Solver(p, B, device=0, lib=lib)
    go = s.loop_run_outcomes(st, T, lp, plant=plant, op=pkg.default_outcome_params(lib), trace=True)
    stop = s.loop_run_outcomes(st, T, lp, plant=plant, op=pkg.default_outcome_params(lib, stop_when_down=True), trace=True)
    seq = _chunks(s, st, 18, lp, None, plant)
    s.close()
    up = ~loaded
    dt = stop[1]["down_tick"].astype(int)
    assert (dt[up] == -1).all() and (dt[loaded] >= 10).all() and (dt[loaded] <= 18).all()
    # robots never down: states, traces and records are those of the run that does not stop
    assert _same(stop[0][up], go[0][up]) and _same(stop[1][up], go[1][up])
    assert _same(stop[2][:, up], go[2][:, up]) and _same(stop[3][:, up], go[3][:, up])
    # halted robots: the record of the run that does not stop, the state that run had at the down tick, zero trace rows afterwards
    assert _same(stop[1][loaded], go[1][loaded])
    assert (stop[0]["tick"][loaded] == dt[loaded]).all() and (go[0]["tick"] == T).all()
    for i in np.flatnonzero(loaded):
        assert stop[0][i].tobytes() == seq[dt[i] - 1][i].tobytes(), i
        assert _same(stop[2][:dt[i], i], go[2][:dt[i], i]) and _same(stop[3][:dt[i], i], go[3][:dt[i], i]), i
        assert (stop[2][dt[i]:, i] == 0).all() and (stop[3][dt[i]:, i] == 0).all(), i
        assert (go[2][dt[i]:, i] != 0).any(), i      # (the other run went on applying forces)
    # a second call on the halted fleet leaves the halted robots alone from its first tick
    s = pkg.Solver(p, B, device=0, lib=lib)
    again = s.loop_run_outcomes(stop[0], 5, lp, plant=plant, op=pkg.default_outcome_params(lib, stop_when_down=True), outcomes=stop[1], trace=True)
    s.close()
    assert _same(again[0][loaded], stop[0][loaded]) and _same(again[1][loaded], stop[1][loaded])
    assert (again[2][:, loaded] == 0).all() and (again[3][:, loaded] == 0).all()
    assert (again[0]["tick"][up] == T + 5).all() and (again[1]["ticks"][up] == T + 5).all()


@pytest.mark.parametrize("B,stop", [(96, False), (96, True), (3000, False), (3000, True)])
def test_accumulation_across_calls(pkg, lib, B, stop):
    p = pkg.default_params(10, pkg.MODE_CONVERGED, lib)
    lp, st, cmds = _fleet(pkg, lib, B, seed=4)
    ctrl, plant = _records(pkg, p, B, "both", seed=8)      # every 16th robot pressed with 1000 N: down by tick 18
    plant["ext_force_world"][11::16, 2] = -450.0           # ... and as many with 450 N, who sink more slowly
    op = pkg.default_outcome_params(lib, stop_when_down=stop)
    st["movement_mode"] = cmds[:, 6]
    s = pkg.Solver(p, B, device=0, lib=lib)
    whole = s.loop_run_outcomes(st, 60, lp, ctrl=ctrl, plant=plant, op=op, trace=True)
    a = s.loop_run_outcomes(st, 20, lp, ctrl=ctrl, plant=plant, op=op, trace=True)
    b = s.loop_run_outcomes(a[0], 40, lp, ctrl=ctrl, plant=plant, op=op, outcomes=a[1], trace=True)
    s.close()
    down = whole[1]["down_tick"]
    print(f"B={B} stop={stop}: down ticks {np.unique(down, return_counts=True)}")
    assert ((down > 0) & (down <= 20)).any() and (down > 20).any() and (down == -1).any()      # before, after the cut, never
    assert _same(whole[0], b[0]) and _same(whole[1], b[1])
    assert _same(whole[2], np.concatenate([a[2], b[2]])) and _same(whole[3], np.concatenate([a[3], b[3]]))
    assert a[1].tobytes() != b[1].tobytes()      # (the buffer given is not written: the call returns a copy)


def test_device_buffers_give_the_host_call(pkg, lib):
    import torch

    B, T = 48, 25
    p = pkg.default_params(10, pkg.MODE_CONVERGED, lib)
    lp, st, cmds = _fleet(pkg, lib, B, seed=6)
    ctrl, plant = _records(pkg, p, B, "both", seed=2)
    st["movement_mode"] = cmds[:, 6]
    op = pkg.default_outcome_params(lib, stop_when_down=True)
    s = pkg.Solver(p, B, device=0, lib=lib)
    want = s.loop_run_outcomes(st, T, lp, ctrl=ctrl, plant=plant, op=op, trace=True)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1).copy()).cuda()      # noqa: E731
    d_st, d_oc, d_ctrl, d_plant = dev(st), dev(pkg.loop_outcomes(B, lib)), dev(ctrl), dev(plant)
    d_tf = torch.full((T, B, 12), 7.0, dtype=torch.float64, device="cuda")
    d_tc = torch.full((T, B, 4), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s.loop_run_outcomes_device(B, d_st.data_ptr(), T, d_oc.data_ptr(), lp, op, d_ctrl=d_ctrl.data_ptr(), d_plant=d_plant.data_ptr(),
                               d_trace_forces=d_tf.data_ptr(), d_trace_contacts=d_tc.data_ptr())
    s.wait()
    s.close()
    assert d_st.cpu().numpy().tobytes() == want[0].tobytes() and d_oc.cpu().numpy().tobytes() == want[1].tobytes()
    assert _same(d_tf.cpu().numpy(), want[2]) and _same(d_tc.cpu().numpy(), want[3])
    assert (want[1]["down_tick"] > 0).any()


def _host(pkg):
    import __graft_entry__ as g

    host = C.CDLL(str(g.build_host()))
    vp = C.c_void_p
    host.qh_loop_create_robot.argtypes = [C.c_char_p, C.c_int, vp, vp, vp, vp]
    host.qh_loop_create_robot.restype = vp
    for f in ("qh_loop_tick", "qh_loop_destroy", "qh_loop_device_status"):
        getattr(host, f).argtypes = [vp]
    host.qh_loop_outcome.argtypes = [vp, vp]
    host.qh_loop_set_outcome_params.argtypes = [vp, vp]
    host.qh_loop_set_command.argtypes = [vp, vp, C.c_double]
    return host


def test_host_class_records(pkg, lib):
    """The records of robots under model mismatch against those of the host twin (host/ClosedLoopHost.h: the same tick on the CPU,
    one B = 1 solve per tick, feeding the same loop_outcome_one).  Counters equal; state-derived fields to the 1e-8 and forces to
    the 1e-6 N of the existing host comparison; the sum of squares to what 1e-8 per velocity error amounts to over its ticks,
    |d sum e^2| <= ticks * 2 max(e) * 1e-8."""
    N, T0, T, B = 10, 6, 130, 8
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    lp, st, cmds = _fleet(pkg, lib, B, seed=3)
    cmds[:, 6] = 1.0
    ctrl = pkg.instance_params(p, B)
    plant = pkg.plant_params(p, B)
    plant["mass"][0] += 3.0
    plant["mass"][1] -= 2.0
    plant["ext_force_world"][3] = [0.0, 12.0, 0.0]
    plant["ext_torque_body"][4] = [0.0, 0.0, 0.8]
    v = pkg.random_go1_variants(B, seed=9, base=p)[5]
    v["mu"] = 0.6
    ctrl[5] = v
    plant["mass"][5] = v["mass"] + 1.5
    op = pkg.default_outcome_params(lib)
    op.down_height = 0.285      # robots 2 (0.28 m) and 5 (0.27 m) are commanded below it: "down" ticks without a crash
    s = pkg.Solver(p, B, device=0, lib=lib)
    st0, oc = s.loop_run_outcomes(st, T0, lp, ctrl=ctrl, plant=plant, op=op)
    st0["movement_mode"] = cmds[:, 6]
    fin, oc = s.loop_run_outcomes(st0, T, lp, ctrl=ctrl, plant=plant, op=op, outcomes=oc)
    s.close()
    host = _host(pkg)
    ho = pkg.loop_outcomes(B, lib)
    for i in range(B):
        h = host.qh_loop_create_robot(str(pkg.LIB_PATH).encode(), N, C.addressof(lp), st[i:i + 1].ctypes.data, ctrl[i:i + 1].ctypes.data,
                                      plant[i:i + 1].ctypes.data)
        assert h and host.qh_loop_device_status(h) == 0
        host.qh_loop_set_outcome_params(h, C.addressof(op))
        for _ in range(T0):
            assert host.qh_loop_tick(h) == 1
        host.qh_loop_set_command(h, np.ascontiguousarray(cmds[i, :6]).ctypes.data, float(cmds[i, 6]))
        for t in range(T):
            assert host.qh_loop_tick(h) == 1, (i, t)
        host.qh_loop_outcome(h, ho[i:i + 1].ctypes.data)
        host.qh_loop_destroy(h)
    down = oc["down_tick"] >= 0
    print("down ticks, device:", oc["down_tick"].tolist(), "host:", ho["down_tick"].tolist())
    assert down.any() and not down.all() and (oc["ticks"][~down] == T0 + T).all()
    for k in COUNTERS:
        assert np.array_equal(oc[k], ho[k]), k
    worst = {k: float(np.abs(oc[k] - ho[k]).max()) for k in ("min_height", "min_upright", "max_height_err", "max_vel_err", "max_ang_vel",
                                                            "max_force_z", "sum_vel_err_sq")}
    print("device against host records, worst differences:", worst)
    for k in ("min_height", "min_upright", "max_height_err", "max_vel_err", "max_ang_vel"):
        assert worst[k] <= 1e-8, (k, worst)
    assert worst["max_force_z"] <= 1e-6
    assert (np.abs(oc["sum_vel_err_sq"] - ho["sum_vel_err_sq"]) <= oc["ticks"] * 2 * oc["max_vel_err"] * 1e-8).all()


def test_refusals_invalid_records_and_buffers(pkg, lib, monkeypatch):
    lp = pkg.default_loop_params(lib)
    st = pkg.loop_states([[0.0, 0.0, 0.3, 0.0, 0.0, 0.0, 0.0]] * 4, lp, lib=lib)
    p = pkg.default_params(10, pkg.MODE_CONVERGED, lib)
    ctrl, plant = pkg.instance_params(p, 4), pkg.plant_params(p, 4)

    def code(s, **kw):
        try:
            s.loop_run_outcomes(st, 3, kw.pop("lp", lp), **kw)
            return pkg.OK
        except pkg.QmpcError as e:
            return e.code

    def code_inst(s, **kw):
        try:
            s.loop_run_instances(st, 3, kw.pop("lp", lp), **kw)
            return pkg.OK
        except pkg.QmpcError as e:
            return e.code

    warm = pkg.default_loop_params(lib); warm.warm_start = 1.0
    # the codes qmpc_loop_run_instances gives
    sc = pkg.Solver(pkg.default_convex_params(20, pkg.MODE_CONVERGED, lib), 4, device=0, lib=lib)
    assert code(sc, plant=plant) == code_inst(sc, plant=plant) == pkg.UNSUPPORTED
    assert code(sc, ctrl=ctrl) == code_inst(sc, ctrl=ctrl) == pkg.UNSUPPORTED
    assert code(sc) == pkg.UNSUPPORTED      # without records too: the outcome kernels are QuatMpc's
    sc.close()
    sr = pkg.Solver(pkg.default_params(10, pkg.MODE_REFERENCE, lib), 4, device=0, lib=lib)
    assert code(sr, plant=plant) == code_inst(sr, plant=plant) == pkg.UNSUPPORTED and code(sr) == pkg.UNSUPPORTED
    sr.close()
    s8 = pkg.Solver(pkg.default_biped8_params(16, pkg.MODE_CONVERGED, lib), 4, device=0, lib=lib)
    assert code(s8, plant=plant) == code_inst(s8, plant=plant) == pkg.BAD_ARGUMENT and code(s8) == pkg.BAD_ARGUMENT
    s8.close()
    s = pkg.Solver(p, 4, device=0, lib=lib)
    assert code(s, ctrl=ctrl, lp=warm) == code_inst(s, ctrl=ctrl, lp=warm) == pkg.UNSUPPORTED
    assert code(s, plant=plant, lp=warm) == pkg.OK and code(s, lp=warm) == pkg.OK and code(s) == pkg.OK
    big = pkg.loop_states([[0.0, 0.0, 0.3, 0.0, 0.0, 0.0, 0.0]] * 5, lp, lib=lib)
    with pytest.raises(pkg.QmpcError) as e:
        s.loop_run_outcomes(big, 3, lp, plant=pkg.plant_params(p, 5))
    assert e.value.code == pkg.BATCH_TOO_LARGE
    s.close()
    # an invalid record leaves its outcome record's bytes untouched, in both launch forms
    B = 12
    lp2, st2, cmds = _fleet(pkg, lib, B, seed=6)
    c2 = pkg.random_go1_variants(B, seed=7, base=p)
    c2["mu"] = np.maximum(c2["mu"], 0.5)
    p2 = pkg.random_go1_plants(B, seed=8, base=p, force=(0.0, 10.0))
    c2["mu"][3] = -1.0                 # invalid controller record
    p2["inertia"][8] = 0.0             # invalid (singular) plant record
    marked = pkg.loop_outcomes(B, lib)
    raw = marked.view(np.uint8).reshape(B, 128)
    raw[3] = 0xA5
    raw[8] = np.frombuffer(np.full(16, np.nan).tobytes(), dtype=np.uint8)
    outs = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("QMPC_LOOP_FUSED", fused)
        s = pkg.Solver(p, B, device=0, lib=lib)
        assert s.loop_instances_plan(B, True, False)[0] == ("persistent" if fused == "1" else "per_tick")
        x, oc, tf, tc = s.loop_run_outcomes(st2, 20, lp2, ctrl=c2, plant=p2, outcomes=marked, trace=True)
        s.close()
        for i in (3, 8):
            assert oc[i].tobytes() == marked[i].tobytes() and x["status"][i] == pkg.BAD_PARAMS and x["tick"][i] == 0
            assert (tf[:, i] == 0).all() and (tc[:, i] == 0).all()
        others = [i for i in range(B) if i not in (3, 8)]
        assert (oc["ticks"][others] == 20).all() and (x["tick"][others] == 20).all()
        outs[fused] = (x, oc, tf, tc)
    monkeypatch.delenv("QMPC_LOOP_FUSED")
    for a, b in zip(outs["0"], outs["1"]):
        assert _same(a, b)
    # buffers: what qmpc_loop_run_instances allocates (764 + 264 B per robot of max_batch), and for the host-buffer outcome call
    # its staging of the records (128 B) on first use; the device-buffer call allocates no staging
    s = pkg.Solver(p, 1000, device=0, lib=lib)
    s.prepare(4)
    s.loop_run(st, 3, lp)
    before = s.query(pkg.QUERY_DEVICE_BYTES)
    s.loop_run_instances(st, 3, lp, ctrl=ctrl, plant=plant)
    assert s.query(pkg.QUERY_DEVICE_BYTES) - before == 1028 * 1000
    assert _same(s.loop_run_outcomes(st, 0, lp, ctrl=ctrl, plant=plant)[0], st)      # ticks = 0: nothing runs, no staging yet
    assert s.query(pkg.QUERY_DEVICE_BYTES) - before == 1028 * 1000
    s.loop_run_outcomes(st, 3, lp, ctrl=ctrl, plant=plant)
    assert s.query(pkg.QUERY_DEVICE_BYTES) - before == (1028 + 128) * 1000
    s.loop_run_outcomes(st, 3, lp, plant=plant)
    s.loop_run_instances(st, 3, lp, ctrl=ctrl, plant=plant)
    assert s.query(pkg.QUERY_DEVICE_BYTES) - before == (1028 + 128) * 1000
    s.close()
