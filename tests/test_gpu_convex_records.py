"""GPU suite (-m gpu): the closed loops with per-robot records on a ConvexMpc handle (qmpc_set_convex_records, include/qmpc.h;
qmpc_loop_crec.hip).

A ConvexMpc handle in the converged mode that opted in runs qmpc_loop_run_instances*, qmpc_loop_run_outcomes* and
qmpc_loop_run_pushes* with the semantics they have on a QuatMpc handle.  Records equal to the handle's values give the bytes of
qmpc_loop_run on the same handle in both launch forms; the two forms agree with each other on any records; interleaved
controller sets are the plain loops of handles carrying each set; a permuted fleet gives the permuted result; outcome records,
stop_when_down, push windows and the freeze of an invalid record behave as DESIGN.md sections 3l - 3n define them.

Sizes, from the enumeration of tests/native/records_plan_host.cpp --check convex: up to 2048 robots the call takes the persistent kernel
on the plain loop's variant (3 up to 768 robots at N = 10 and 512 at N = 20); under QMPC_LOOP_FUSED=0 the per-tick solve with
controller records is qmpc_solve_cw_inst_kernel on the variant of qmpc_convex_solve_instances* (3 / 5 / 6 from 1 / 769 / 2049
instances at N = 10, 1 / 513 / 1025 at N = 20).  Launch forms other than the default are run in worker processes
(tests/_convex_records_worker.py): the knob is read once per process."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = Path(__file__).resolve().parent
WORKER = HERE / "_convex_records_worker.py"


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _all_same(got, want):
    return all(_same(a, b) for a, b in zip(got, want))


def _fleet(pkg, lib, B, seed=29):
    """the commands of the ConvexMpc loop tests (tests/test_gpu_lane.py): no roll / pitch rate command"""
    rng = np.random.default_rng(seed)
    lp = pkg.default_loop_params(lib)
    cmds = np.zeros((B, 7))
    cmds[:, 0] = 0.6 * rng.uniform(-0.5, 0.5, B); cmds[:, 1] = rng.uniform(-0.2, 0.2, B); cmds[:, 2] = rng.uniform(0.26, 0.32, B)
    cmds[:, 5] = rng.uniform(-0.5, 0.5, B); cmds[:, 6] = (rng.random(B) < 0.9).astype(float)
    cmds[cmds[:, 6] == 0, :2] = 0.0
    cmds[cmds[:, 6] == 0, 5] = 0.0
    stand = cmds.copy(); stand[:, 6] = 0.0
    return lp, pkg.loop_states(stand, lp, height=0.3, yaw=rng.uniform(-3, 3, B), lib=lib), cmds


def _solver(pkg, lib, p, B, opt_in=True):
    s = pkg.Solver(p, B, device=0, lib=lib)
    if opt_in:
        s.set_convex_records(True)
    return s


def _worker(args, fused, variant=None):
    env = dict(os.environ)
    env.pop("QMPC_LOOP_FUSED", None)
    env.pop("QMPC_VARIANT", None)
    if fused is not None:
        env["QMPC_LOOP_FUSED"] = fused
    if variant is not None:
        env["QMPC_VARIANT"] = variant
    r = subprocess.run([sys.executable, str(WORKER)] + [str(a) for a in args], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_not_opted_in_is_refused_and_the_setting_reads_back(pkg, lib):
    B = 4
    p = pkg.default_convex_params(10, pkg.MODE_CONVERGED, lib)
    lp, st, _ = _fleet(pkg, lib, B)
    ctrl, plant, push = pkg.instance_params(p, B), pkg.plant_params(p, B), pkg.push_params(B)
    s = _solver(pkg, lib, p, B, opt_in=False)
    assert s.convex_records() is False and s.query(pkg.QUERY_CONVEX_RECORDS) == 0
    assert s.loop_instances_plan(B, True, False) is None and s.loop_instances_plan(B, False, False) is None
    calls = (lambda: s.loop_run_instances(st, 2, lp, ctrl=ctrl, plant=plant), lambda: s.loop_run_instances(st, 2, lp, plant=plant),
             lambda: s.loop_run_outcomes(st, 2, lp, plant=plant), lambda: s.loop_run_outcomes(st, 2, lp),
             lambda: s.loop_run_pushes(st, 2, push, lp, ctrl=ctrl))
    for call in calls:
        with pytest.raises(pkg.QmpcError) as e:
            call()
        assert e.value.code == pkg.UNSUPPORTED
    s.set_convex_records(True)
    assert s.convex_records() is True and s.loop_instances_plan(B, True, False) == ("persistent", "wform_lds")
    for call in calls:
        call()
    s.set_convex_records(False)
    assert s.convex_records() is False
    with pytest.raises(pkg.QmpcError) as e:
        calls[0]()
    assert e.value.code == pkg.UNSUPPORTED
    for bad in (2, -1):
        assert lib.qmpc_set_convex_records(s._h, bad) == pkg.BAD_ARGUMENT
    s.close()
    # the setting does nothing on a handle of another model
    pq = pkg.default_params(10, pkg.MODE_CONVERGED, lib)
    sq = pkg.Solver(pq, B, device=0, lib=lib)
    before = sq.loop_instances_plan(B, True, False)
    sq.set_convex_records(True)
    assert sq.loop_instances_plan(B, True, False) == before
    sq.close()


@pytest.mark.parametrize("N,B,T,family", [(10, 40, 30, "wform_lds"), (20, 40, 30, "wform_lds"), (10, 800, 8, "wform_ws"),
                                          (20, 1100, 6, "wform_ws")])
def test_uniform_records_equal_the_plain_loop_persistent(pkg, lib, N, B, T, family):
    """40 robots x 30 ticks, the persistent kernel on variant 3; 800 robots at N = 10 on variant 5 and 1100 at N = 20 on variant
    6 (the two instantiations at the 256-register limit), a few ticks each"""
    p = pkg.default_convex_params(N, pkg.MODE_CONVERGED, lib)
    lp, st0, cmds = _fleet(pkg, lib, B)
    s = _solver(pkg, lib, p, B)
    assert s.loop_instances_plan(B, True, False) == ("persistent", family)
    ctrl, plant = pkg.instance_params(p, B), pkg.plant_params(p, B)
    a = s.loop_run(st0, 6, lp)
    b = s.loop_run_instances(st0, 6, lp, ctrl=ctrl, plant=plant)
    assert _same(a, b)
    a["movement_mode"] = b["movement_mode"] = cmds[:, 6]
    want = s.loop_run(a, T, lp, trace=True)
    got = s.loop_run_instances(b, T, lp, ctrl=ctrl, plant=plant, trace=True)
    only_plant = s.loop_run_instances(b, T, lp, plant=plant, trace=True)
    only_ctrl = s.loop_run_instances(b, T, lp, ctrl=ctrl, trace=True)
    s.close()
    assert (want[0]["tick"] == 6 + T).all() and (want[0]["status"] == 0).mean() > 0.95 and (want[2] == 0).any()
    assert _all_same(got, want) and _all_same(only_plant, want) and _all_same(only_ctrl, want)


@pytest.mark.parametrize("B,T,horizons,family", [(200, 20, "10,20", "wform_lds"), (800, 6, "10", "wform_ws"), (1100, 5, "20", "wform_ws")])
def test_uniform_records_equal_the_plain_loop_per_tick(B, T, horizons, family):
    """Under QMPC_LOOP_FUSED=0 (the worker asserts the bytes): 200 robots x 20 ticks at N = 10 and N = 20, the per-instance
    kernel on variant 3; 800 robots at N = 10 on variant 5; 1100 robots at N = 20 on variant 6"""
    out = _worker(["uniform", B, T, horizons], "0")
    for N in horizons.split(","):
        assert f"UNIFORM {N} ('per_tick', '{family}')" in out, out


@pytest.mark.parametrize("B,variant,form", [(40, None, "('per_tick', 'wform_lds')"), (2100, None, "('per_tick', 'dense_ws')"),
                                            (200, "4", "('per_tick', 'lane')")])
def test_plant_records_alone_freeze_and_halt_per_tick(B, variant, form):
    """Without controller records the tick's solve is the plain ConvexMpc tick, and a frozen or halted robot rests on that kernel
    rejecting the NaN in the first word of a qmpc_convex_input: the wrench form (40 robots), the round-1 kernel (2100 robots at
    N = 10: beyond one resident round of the workspace form) and the lane kernel (QMPC_VARIANT=4).  The worker asserts what
    freezing and halting mean.  The other robots: on the wave kernels, where a workgroup owns its instance, the bytes of the run
    on valid records; on the lane kernel the same status words and positions within 1e-7 m, the bound of
    tests/test_gpu_lane.py between ConvexMpc loops of different kernel families (the stance sort sees another batch)."""
    out = _worker(["idle", B, 16, 10], "0", variant)
    line = [l for l in out.splitlines() if l.startswith("IDLE")][0]
    print(line)
    assert form in line, line
    if variant is None:
        assert "others the same bytes: True" in line, line
    else:
        assert float(line.split("max position difference ")[1].split()[0]) <= 1e-7, line


def test_launch_forms_give_the_same_bytes():
    """random controllers, random plants with disturbance wrenches, pushes, outcome records with stop_when_down, frozen robots:
    40 robots x 40 ticks in the persistent and in the per-tick form"""
    outs = {f: _worker(["random", 40, 40, 10], f) for f in ("0", "1")}
    sha = {f: [l for l in o.splitlines() if l.startswith("SHA")][0] for f, o in outs.items()}
    print(outs["1"])
    assert "FORM ('per_tick', 'wform_lds')" in outs["0"] and "FORM ('persistent', 'wform_lds')" in outs["1"]
    assert sha["0"] == sha["1"], (sha["0"], sha["1"])


def test_two_interleaved_controller_sets_and_a_permuted_fleet(pkg, lib):
    B, T, N = 40, 25, 10
    p = pkg.default_convex_params(N, pkg.MODE_CONVERGED, lib)
    lp, st0, cmds = _fleet(pkg, lib, B, seed=5)
    sets = pkg.random_go1_convex_variants(2, seed=9, base=p)
    sets["mu"] = np.maximum(sets["mu"], 0.5)
    ctrl = sets[np.arange(B) % 2]
    s = _solver(pkg, lib, p, B)
    pre = s.loop_run_instances(st0, 6, lp, ctrl=ctrl)
    st = pre.copy()
    st["movement_mode"] = cmds[:, 6]
    got = s.loop_run_instances(st, T, lp, ctrl=ctrl, trace=True)
    perm = np.random.default_rng(2).permutation(B)
    gp = s.loop_run_instances(st[perm], T, lp, ctrl=ctrl[perm], trace=True)
    s.close()
    assert (got[0]["tick"] == 6 + T).all() and (got[0]["status"] == 0).mean() > 0.95
    assert _same(gp[0], got[0][perm]) and _same(gp[1], got[1][:, perm]) and _same(gp[2], got[2][:, perm])
    for g in range(2):      # a plain loop on a handle carrying the set: controller and plant are the set's robot
        idx = np.arange(g, B, 2)
        sg = pkg.Solver(pkg.params_with(p, sets[g]), len(idx), device=0, lib=lib)
        x = sg.loop_run(st0[idx], 6, lp)
        assert _same(x, pre[idx]), g
        x["movement_mode"] = cmds[idx, 6]
        want = sg.loop_run(x, T, lp, trace=True)
        sg.close()
        assert _same(want[0], got[0][idx]) and _same(want[1], got[1][:, idx]) and _same(want[2], got[2][:, idx]), g
    assert not _same(got[1][:, 0::2], got[1][:, 1::2])


def _standing(pkg, lib, B):
    """standing robots (12.84 kg, 4 x fz_max = 800 N of lift at most), classes by i mod 4: 0 no push; 1 -2500 N in z from tick 0
    for 40 ticks (net 1826 N down: 0.15 m in 9.2 ticks of 5 ms from rest); 2 the same from tick 10; 3 100 N lateral for one tick
    at tick 5"""
    p = pkg.default_convex_params(10, pkg.MODE_CONVERGED, lib)
    assert abs(p.mass - 12.84) < 1e-12 and p.fz_max == 200.0
    lp = pkg.default_loop_params(lib)
    st = pkg.loop_states([[0.0, 0.0, 0.30, 0.0, 0.0, 0.0, 0.0]] * B, lp, height=0.3, yaw=np.linspace(-3, 3, B), lib=lib)
    cls = np.arange(B) % 4
    push = pkg.push_params(B)
    push["force_world"][cls == 1, 0, 2] = push["force_world"][cls == 2, 0, 2] = -2500.0
    push["ticks"][cls == 1], push["ticks"][cls == 2] = 40.0, 40.0
    push["start_tick"][cls == 2] = 10.0
    push["force_world"][cls == 3, 0, 1] = 100.0
    push["start_tick"][cls == 3], push["ticks"][cls == 3] = 5.0, 1.0
    return p, lp, st, push, cls


def test_outcomes_and_pushes(pkg, lib):
    B, T = 40, 40
    p, lp, st, push, cls = _standing(pkg, lib, B)
    ctrl, plant = pkg.instance_params(p, B), pkg.plant_params(p, B)
    go, stop = pkg.default_outcome_params(lib), pkg.default_outcome_params(lib, stop_when_down=True)
    s = _solver(pkg, lib, p, B)
    inst = s.loop_run_instances(st, T, lp, ctrl=ctrl, plant=plant, trace=True)
    outc = s.loop_run_outcomes(st, T, lp, ctrl=ctrl, plant=plant, op=go, trace=True)
    # the outcome call's states and traces are the instances call's
    assert _same(outc[0], inst[0]) and _same(outc[2], inst[1]) and _same(outc[3], inst[2])
    assert (outc[1]["down_tick"] == -1).all() and (outc[1]["ticks"] == T).all()
    # windows that never act give the outcome call's bytes
    never = pkg.push_params(B, 2)
    never["start_tick"][:, 0], never["ticks"][:, 0], never["force_world"][:, 0] = T + 10.0, 5.0, [300.0, -200.0, -500.0]
    never["start_tick"][:, 1], never["ticks"][:, 1], never["force_world"][:, 1] = 3.0, 0.0, [300.0, -200.0, -500.0]
    assert _all_same(s.loop_run_pushes(st, T, never, lp, ctrl=ctrl, plant=plant, op=go, trace=True), outc)
    # a push large enough to fell a robot sets down_tick; without stop_when_down the robot goes on
    fin, oc = s.loop_run_pushes(st, T, push, lp, ctrl=ctrl, plant=plant, op=go)
    halt = s.loop_run_pushes(st, T, push, lp, ctrl=ctrl, plant=plant, op=stop, trace=True)
    s.close()
    dt = oc["down_tick"]
    print(f"down ticks class 1 {sorted(set(dt[cls == 1].astype(int).tolist()))}, class 2 {sorted(set(dt[cls == 2].astype(int).tolist()))}")
    assert (dt[cls == 0] == -1).all() and (dt[cls == 3] == -1).all()
    assert ((6 <= dt[cls == 1]) & (dt[cls == 1] <= 14)).all() and ((16 <= dt[cls == 2]) & (dt[cls == 2] <= 24)).all()
    assert (fin["tick"] == T).all() and (oc["ticks"][dt < 0] == T).all() and (oc["ticks"][dt >= 0] == dt[dt >= 0]).all()
    # class 0 is the unpushed robot, bit for bit; class 3 is shoved
    assert _same(fin[cls == 0], outc[0][cls == 0]) and not _same(fin[cls == 3], outc[0][cls == 3])
    # stop_when_down: the same records; a halted robot stays at its down tick, its trace rows are zero from there on, and its
    # neighbours keep their bytes
    hx, ho, hf, hc = halt
    down = dt >= 0
    assert _same(ho, oc) and (hx["tick"][down] == dt[down]).all() and _same(hx[~down], fin[~down])
    for i in np.flatnonzero(down):
        k = int(dt[i])
        assert (hf[k:, i] == 0).all() and (hc[k:, i] == 0).all() and (hf[:k, i] != 0).any(), i


def test_invalid_records_freeze_their_robot_alone(pkg, lib):
    B, T = 40, 12
    p = pkg.default_convex_params(10, pkg.MODE_CONVERGED, lib)
    lp, st, cmds = _fleet(pkg, lib, B, seed=3)
    st["movement_mode"] = cmds[:, 6]
    ctrl = pkg.random_go1_convex_variants(B, seed=21, base=p)
    ctrl["mu"] = np.maximum(ctrl["mu"], 0.5)
    plant = pkg.random_go1_plants(B, seed=22, base=p)
    bad_c, bad_p = ctrl.copy(), plant.copy()
    bad_c["mass"][3] = np.nan; bad_c["mu"][9] = 0.0; bad_p["mass"][17] = -1.0; bad_p["inertia"][25] = 0.0
    frozen = [3, 9, 17, 25]
    s = _solver(pkg, lib, p, B)
    good = s.loop_run_outcomes(st, T, lp, ctrl=ctrl, plant=plant, trace=True)
    got = s.loop_run_outcomes(st, T, lp, ctrl=bad_c, plant=bad_p, trace=True)
    s.close()
    x, oc, tf, tc = got
    assert (x["status"][frozen] == pkg.BAD_PARAMS).all() and (x["iterations"][frozen] == 0).all() and (x["tick"][frozen] == 0).all()
    keep = [n for n in pkg.LOOP_STATE_DTYPE.names if n not in ("status", "iterations")]
    for n in keep:
        assert _same(x[n][frozen], st[n][frozen]), n
    assert (tf[:, frozen] == 0).all() and (tc[:, frozen] == 0).all() and _same(oc[frozen], pkg.loop_outcomes(B, lib)[frozen])
    rest = np.setdiff1d(np.arange(B), frozen)
    assert _same(x[rest], good[0][rest]) and _same(oc[rest], good[1][rest]) and _same(tf[:, rest], good[2][:, rest])
    assert _same(tc[:, rest], good[3][:, rest]) and (good[0]["tick"] == T).all()


def test_refusals_with_the_setting_on(pkg, lib):
    B = 4
    p = pkg.default_convex_params(10, pkg.MODE_CONVERGED, lib)
    lp, st, _ = _fleet(pkg, lib, B)
    ctrl, plant = pkg.instance_params(p, B), pkg.plant_params(p, B)
    warm = pkg.default_loop_params(lib)
    warm.warm_start = 1.0
    s = _solver(pkg, lib, p, B)
    for wr in (False, True):      # ctrl with the warm start: refused whatever qmpc_set_loop_warm_records says
        s.set_loop_warm_records(wr)
        assert s.loop_instances_plan(B, True, True) is None
        for call in (lambda: s.loop_run_instances(st, 2, warm, ctrl=ctrl), lambda: s.loop_run_outcomes(st, 2, warm, ctrl=ctrl, plant=plant),
                     lambda: s.loop_run_pushes(st, 2, pkg.push_params(B), warm, ctrl=ctrl)):
            with pytest.raises(pkg.QmpcError) as e:
                call()
            assert e.value.code == pkg.UNSUPPORTED
    # plant records alone follow the plain warm-started loop
    assert s.loop_instances_plan(B, False, True) == ("persistent", "wform_lds")
    assert _same(s.loop_run_instances(st, 8, warm, plant=plant), s.loop_run(st, 8, warm))
    with pytest.raises(pkg.QmpcError) as e:
        s.loop_run_instances(np.concatenate([st, st]), 2, lp, plant=np.concatenate([plant, plant]))
    assert e.value.code == pkg.BATCH_TOO_LARGE
    s.close()
    p10 = pkg.default_convex_params(10, pkg.MODE_CONVERGED, lib)      # a knot spacing other than the tick's 5 ms (as qmpc_loop_run*)
    p10.h = 0.01
    sh = _solver(pkg, lib, p10, B)
    for call in (lambda: sh.loop_run_instances(st, 2, lp, plant=plant), lambda: sh.loop_run_outcomes(st, 2, lp, ctrl=ctrl),
                 lambda: sh.loop_run(st, 2, lp)):
        with pytest.raises(pkg.QmpcError) as e:
            call()
        assert e.value.code == pkg.UNSUPPORTED
    sh.close()
    sr = _solver(pkg, lib, pkg.default_convex_params(10, pkg.MODE_REFERENCE, lib), B)      # the reference mode
    assert sr.loop_instances_plan(B, False, False) is None
    for call in (lambda: sr.loop_run_instances(st, 2, lp, plant=plant), lambda: sr.loop_run_outcomes(st, 2, lp)):
        with pytest.raises(pkg.QmpcError) as e:
            call()
        assert e.value.code == pkg.UNSUPPORTED
    sr.close()


def test_ticks_zero_then_a_capture_by_the_caller(pkg, lib):
    """After a call with ticks = 0 the device entry point runs inside a stream capture of the CALLER's in the persistent form:
    nothing is allocated, and the graph replayed once gives the bytes of the eager call."""
    import torch

    N, B, TT = 10, 40, 8
    p = pkg.default_convex_params(N, pkg.MODE_CONVERGED, lib)
    lp, st, cmds = _fleet(pkg, lib, B, seed=48)
    st["movement_mode"] = cmds[:, 6]
    ctrl = pkg.random_go1_convex_variants(B, seed=35, base=p)
    ctrl["mu"] = np.maximum(ctrl["mu"], 0.5)
    plant = pkg.random_go1_plants(B, seed=36, base=p)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1).copy()).cuda()      # noqa: E731
    s = _solver(pkg, lib, p, B)
    assert s.loop_instances_plan(B, True, False)[0] == "persistent"
    assert _same(s.loop_run_instances(st, 0, lp, ctrl=ctrl, plant=plant), st)
    held = s.query(pkg.QUERY_DEVICE_BYTES)
    d_ctrl, d_plant = dev(ctrl), dev(plant)
    stream = torch.cuda.Stream()

    def buffers():
        return (dev(st), torch.full((TT + 2, B, 12), 7.0, dtype=torch.float64, device="cuda"),
                torch.full((TT + 2, B, 4), 7.0, dtype=torch.float64, device="cuda"))

    def call(d_st, d_tf, d_tc):
        s.loop_run_instances_device(B, d_st.data_ptr(), TT, lp, d_ctrl=d_ctrl.data_ptr(), d_plant=d_plant.data_ptr(),
                                    d_trace_forces=d_tf.data_ptr(), d_trace_contacts=d_tc.data_ptr(), stream=stream.cuda_stream)

    e_st, e_tf, e_tc = buffers()
    torch.cuda.synchronize()
    call(e_st, e_tf, e_tc)      # eager: the reference
    stream.synchronize()
    assert (e_tf[TT:] == 7.0).all() and (e_tc[TT:] == 7.0).all() and not (e_tf[:TT] == 7.0).any()
    x = e_st.cpu().numpy().view(pkg.LOOP_STATE_DTYPE).reshape(B)
    assert (x["status"] == 0).mean() > 0.9 and (x["tick"] == TT).all()
    c_st, c_tf, c_tc = buffers()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        graph.capture_begin(capture_error_mode="thread_local")
        call(c_st, c_tf, c_tc)
        graph.capture_end()
    torch.cuda.synchronize()
    assert _same(c_st.cpu().numpy(), dev(st).cpu().numpy()) and (c_tf == 7.0).all() and (c_tc == 7.0).all()      # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    got = c_st.cpu().numpy(), c_tf.cpu().numpy(), c_tc.cpu().numpy()
    del graph
    assert s.query(pkg.QUERY_DEVICE_BYTES) == held
    s.close()
    assert _same(got[0], e_st.cpu().numpy()) and _same(got[1], e_tf.cpu().numpy()) and _same(got[2], e_tc.cpu().numpy())


def test_host_class_under_disturbance_wrenches(pkg, lib):
    """The world-frame back end with a non-zero wrench against an independent restatement: ConvexMpcHipT in the host closed loop
    (host/ClosedLoopHost.h: the controller's tick on the CPU, optimized_input = R' u, loop_push_wrench and plant_step_ext on the
    handle's mass and inverse inertia, the swing feet), tick for tick.  Five robots, 6 ticks standing and 40 on their commands; a
    window over the whole run is a constant disturbance force and torque, the others are shoves of a few ticks, one while
    standing; robot 0 has none.  Contacts equal in every tick; forces within 1e-6 N and states within 1e-8, the bounds of
    test_convex_mpc_closed_loop_matches_host_classes (tests/test_gpu_parity.py) for the same comparison without a wrench.  The
    device call carries uniform controller + plant records (persistent form; test_launch_forms_give_the_same_bytes ties the
    per-tick form to it), so the solve and the post step are those of the records' unit."""
    import __graft_entry__ as g

    host = C.CDLL(str(g.build_host()))
    vp = C.c_void_p
    host.qh_loop_create_convex_mode.argtypes = [C.c_char_p, C.c_int, C.c_int, vp, vp]
    host.qh_loop_create_convex_mode.restype = vp
    for f in ("qh_loop_tick", "qh_loop_destroy", "qh_loop_device_status"):
        getattr(host, f).argtypes = [vp]
    host.qh_loop_export.argtypes = [vp, vp]
    host.qh_loop_set_pushes.argtypes = [vp, vp, C.c_int]
    host.qh_loop_set_command.argtypes = [vp, vp, C.c_double]
    N, T0, T, B = 10, 6, 40, 5
    p = pkg.default_convex_params(N, pkg.MODE_CONVERGED, lib)
    lp = pkg.default_loop_params(lib)
    cmds = np.array([[0.3, 0.0, 0.30, 0, 0, 0.0, 1], [0.2, 0.1, 0.28, 0, 0, 0.3, 1], [-0.2, 0.0, 0.31, 0, 0, -0.2, 1],
                     [0.0, 0.15, 0.30, 0, 0, 0.0, 1], [0.25, -0.1, 0.29, 0, 0, 0.4, 1]], dtype=np.float64)
    stand = cmds.copy(); stand[:, 6] = 0.0
    st = pkg.loop_states(stand, lp, height=0.3, yaw=[0.0, 0.4, -1.0, 2.0, 0.7], lib=lib)
    push = pkg.push_params(B, 2)
    push[1, 0] = (0.0, 1000.0, [6.0, -9.0, 4.0], [0.2, -0.1, 0.4])      # a constant disturbance: force and torque, every tick
    push[2, 0] = (20.0, 6.0, [0.0, 60.0, 0.0], [0.0, 0.0, 0.0])         # a lateral shove
    push[3, 0] = (12.0, 4.0, [-40.0, 30.0, 0.0], [0.0, 0.0, 0.0])       # two windows, overlapping, with a body torque
    push[3, 1] = (14.0, 6.0, [0.0, 20.0, 0.0], [0.5, 0.0, -2.0])
    push[4, 0] = (3.0, 2.0, [50.0, 0.0, 0.0], [0.0, 0.0, 1.0])          # while standing
    ctrl, plant = pkg.instance_params(p, B), pkg.plant_params(p, B)
    s = _solver(pkg, lib, p, B)
    x, oc = s.loop_run_pushes(st, T0, push, lp, ctrl=ctrl, plant=plant)
    x["movement_mode"] = cmds[:, 6]
    fin, oc, tf, tc = s.loop_run_pushes(x, T, push, lp, ctrl=ctrl, plant=plant, outcomes=oc, trace=True)
    y = s.loop_run_outcomes(st, T0, lp, ctrl=ctrl, plant=plant)[0]
    y["movement_mode"] = cmds[:, 6]
    calm_tf = s.loop_run_outcomes(y, T, lp, ctrl=ctrl, plant=plant, trace=True)[2]
    s.close()
    assert (fin["tick"] == T0 + T).all() and (fin["status"] == 0).all() and (oc["down_tick"] == -1).all()
    worst_f = worst_x = 0.0
    for i in range(B):
        h = host.qh_loop_create_convex_mode(str(pkg.LIB_PATH).encode(), N, pkg.MODE_CONVERGED, C.addressof(lp), st[i:i + 1].ctypes.data)
        assert h and host.qh_loop_device_status(h) == 0
        host.qh_loop_set_pushes(h, push[i].ctypes.data, 2)
        e = np.zeros(1, dtype=pkg.LOOP_STATE_DTYPE)
        for t in range(T0):
            assert host.qh_loop_tick(h) == 1
        host.qh_loop_set_command(h, np.ascontiguousarray(cmds[i, :6]).ctypes.data, float(cmds[i, 6]))
        for t in range(T):
            assert host.qh_loop_tick(h) == 1, (i, t)
            host.qh_loop_export(h, e.ctypes.data)
            assert np.array_equal(e[0]["contacts"], tc[t, i]), (i, t)
            worst_f = max(worst_f, float(np.abs(e[0]["forces_body"] - tf[t, i]).max()))
        for k in ("pos_world", "quat", "lin_vel_world", "ang_vel_body", "foot_pos_world", "lin_vel_d_rel", "foot_target_world"):
            worst_x = max(worst_x, float(np.abs(fin[i][k] - e[0][k]).max()))
        host.qh_loop_destroy(h)
    felt = [float(np.abs(tf[:, i] - calm_tf[:, i]).max()) for i in range(B)]
    print(f"ConvexMpc loop with records under wrenches against the host class, {B} robots x {T0 + T} ticks: worst force difference "
          f"{worst_f:.2e} N, worst state difference {worst_x:.2e}; largest change of a force against the unpushed run [N]: {['%.1e' % v for v in felt]}")
    assert worst_f <= 1e-6 and worst_x <= 1e-8
    # the wrenches were felt (a back end that dropped them would agree with the unpushed run, not with the host class)
    assert felt[0] == 0.0 and min(felt[1:]) > 1e-3
