"""GPU suite (-m gpu): warm-started closed loops with per-robot controller records (qmpc_set_loop_warm_records, include/qmpc.h;
DESIGN.md section 3p).

A handle that opted in accepts lp->warm_start with ctrl in qmpc_loop_run_instances* / _outcomes* / _pushes*: the persistent
kernel (which always carried warm_t), the per-tick wave form (qmpc_solve_w_inst_warm_kernel) and, under QMPC_INSTANCES_AUTO, the
lane form (qmpc_lane_inst_warm_kernel to the warm ticks' cap, the per-instance list kernel on the stragglers).  Every comparison
is against code the library had before: the plain warm-started loop on handles that carry the same values (bytes), the other
launch form (bytes), the wave family against the lane family (status words, 1e-7 N: the cross-family bound of include/qmpc.h).
Sizes: a few hundred robots for the wave forms; 20480 (lane pairs) and 40960 (64-lane wavefronts) for the lane form, as in
tests/test_gpu_loop_instance_lane.py."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from records_fleet import quat_fleet as _fleet, same as _same, walk as _walk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


def _params(pkg, lib, N):
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    p.ipm_mu0 = 1e-6
    return p


def _last(pkg, s):
    return pkg.KERNEL_FAMILY[s.query(pkg.QUERY_LAST_KERNEL)]


def _solver(pkg, lib, p, B, auto=False):
    s = pkg.Solver(p, B, device=0, lib=lib)
    s.set_loop_warm_records(True)
    if auto:
        s.set_instances_policy("auto")
    return s


def _pressed(st, cmds):
    """every 8th robot walks with a fast diagonal command from a state with a sideways and downward velocity and a roll rate
    (tests/test_gpu_loop_instance_lane.py): these take more iterations than the in-gait states"""
    sub = np.arange(len(st)) % 8 == 5
    cmds[sub] = [0.5, -0.2, 0.26, 0.3, -0.3, 0.6, 1.0]
    st["lin_vel_world"][sub] = [0.0, 0.6, -0.4]
    st["ang_vel_body"][sub] = [1.5, 0.0, 0.0]
    return sub


# ---- 1. uniform records give the plain warm loop's bytes ----------------------------------------------------------------------
@pytest.mark.parametrize("N,B,fused,form", [(10, 256, None, "persistent"), (20, 40, None, "persistent"),
                                            (10, 200, "0", "per_tick"), (20, 200, "0", "per_tick")])
def test_uniform_records_equal_the_plain_warm_loop(pkg, lib, monkeypatch, N, B, fused, form):
    if fused is not None:
        monkeypatch.setenv("QMPC_LOOP_FUSED", fused)
    p = _params(pkg, lib, N)
    lp, st, cmds = _fleet(pkg, lib, B, seed=41, trot=True)
    s = _solver(pkg, lib, p, B)
    assert s.loop_instances_plan(B, True, True)[0] == form
    ref = _walk(lambda x, t, tr: s.loop_run(x, t, lp, trace=tr), st, cmds, 6, 40)
    ctrl, plant = pkg.instance_params(p, B), pkg.plant_params(p, B)
    got = _walk(lambda x, t, tr: s.loop_run_instances(x, t, lp, ctrl=ctrl, plant=plant, trace=tr), st, cmds, 6, 40)
    if form == "per_tick":
        assert _last(pkg, s) == s.loop_instances_plan(B, True, True)[1] and _last(pkg, s).startswith("wform")
    only = _walk(lambda x, t, tr: s.loop_run_instances(x, t, lp, ctrl=ctrl, trace=tr), st, cmds, 6, 40)
    # the warm start took part: the same robots started cold in every tick end on other bits
    lp0 = pkg.default_loop_params(lib)
    cold = _walk(lambda x, t, tr: s.loop_run_instances(x, t, lp0, ctrl=ctrl, plant=plant, trace=tr), st, cmds, 6, 40)
    s.close()
    assert (ref[0]["status"] == 0).all() and (ref[0]["tick"] == 46).all() and (ref[2] == 0).any()
    print(f"N={N} B={B} {form}: last tick's iterations warm {ref[0]['iterations'].mean():.2f}, cold {cold[0]['iterations'].mean():.2f}")
    assert (cold[0]["status"] == 0).all() and not _same(ref[1], cold[1])
    for out in (got, only):
        for a, b in zip(ref, out):
            assert _same(a, b)


@pytest.mark.parametrize("B", [20480, 40960])
def test_uniform_records_equal_the_plain_warm_loop_on_the_lane_kernel(pkg, lib, monkeypatch, B):
    # the warm ticks' cap (8): in-gait warm starts take 5 iterations, the pressed robots 10 and more -- those are handed over
    N, T0, T = 10, 3, 9
    p = _params(pkg, lib, N)
    lp, st, cmds = _fleet(pkg, lib, B, seed=42, trot=True)
    _pressed(st, cmds)
    s = _solver(pkg, lib, p, B, auto=True)
    cap = s.query(pkg.QUERY_LANE_CAP, 3)
    assert cap == 8 and s.loop_instances_plan(B, True, True) == ("per_tick", "lane_handoff")
    ref = _walk(lambda x, t, tr: s.loop_run(x, t, lp, trace=tr), st, cmds, T0, T)      # (the plain warm loop's lane form from 18432 robots on)
    ctrl, plant = pkg.instance_params(p, B), pkg.plant_params(p, B)
    got = _walk(lambda x, t, tr: s.loop_run_instances(x, t, lp, ctrl=ctrl, plant=plant, trace=tr), st, cmds, T0, T)
    assert _last(pkg, s) == "lane_handoff"
    s.close()
    # the iteration records of the last tick, a warm-started one: robots beyond the cap were continued by the list kernel
    its = got[0]["iterations"]
    print(f"B={B}: cap {cap}, {int((its > cap).sum())} robots beyond it in the last tick, most iterations {int(its.max())}, "
          f"status words {np.unique(got[0]['status']).tolist()}")
    assert (its > cap).any() and (its <= cap).any()
    assert (ref[0]["tick"] == T0 + T).all() and (ref[2] == 0).any()
    for a, b in zip(ref, got):
        assert _same(a, b)


# ---- 2. per-robot values reach the warm-started solve ------------------------------------------------------------------------------
def _mixed_fleet(pkg, lib, s, p, lp, st, cmds, H, T0, T, family):
    """two interleaved parameter sets over 2 H robots: two H-robot plain warm loops on handles carrying each set, a permuted
    fleet, a shard"""
    B = 2 * H
    v = pkg.random_go1_variants(2, seed=25, base=p)
    v["mu"] = np.maximum(v["mu"], 0.5)
    ctrl = v[np.arange(B) % 2]
    run = lambda c: (lambda x, t, tr: s.loop_run_instances(x, t, lp, ctrl=c, trace=tr))      # noqa: E731
    fleet = _walk(run(ctrl), st, cmds, T0, T)
    if family:
        assert _last(pkg, s) == family
    assert (fleet[0]["tick"] == T0 + T).all() and (fleet[2] == 0).any()
    shard = _walk(run(ctrl[:H]), st[:H], cmds[:H], T0, T)
    perm = np.random.default_rng(3).permutation(B)
    shuf = _walk(run(ctrl[perm]), st[perm], cmds[perm], T0, T)
    assert _same(shard[0], fleet[0][:H]) and _same(shard[1], fleet[1][:, :H]) and _same(shard[2], fleet[2][:, :H])
    assert _same(shuf[0], fleet[0][perm]) and _same(shuf[1], fleet[1][:, perm]) and _same(shuf[2], fleet[2][:, perm])
    parts = []
    for k in range(2):
        one = pkg.Solver(pkg.params_with(p, v[k]), H, device=0, lib=lib)
        r = _walk(lambda x, t, tr: one.loop_run(x, t, lp, trace=tr), st[k::2], cmds[k::2], T0, T)
        one.close()
        assert _same(r[0], fleet[0][k::2]) and _same(r[1], fleet[1][:, k::2]) and _same(r[2], fleet[2][:, k::2]), k
        parts.append(r)
    assert not _same(parts[0][1], parts[1][1])      # the two sets walk differently


@pytest.mark.parametrize("fused", ["0", "1"])
def test_a_mixed_fleet_equals_its_parts(pkg, lib, monkeypatch, fused):
    monkeypatch.setenv("QMPC_LOOP_FUSED", fused)
    N, H = 10, 128
    p = _params(pkg, lib, N)
    lp, st, cmds = _fleet(pkg, lib, 2 * H, seed=43)
    s = _solver(pkg, lib, p, 2 * H)
    assert s.loop_instances_plan(2 * H, True, True)[0] == ("persistent" if fused == "1" else "per_tick")
    _mixed_fleet(pkg, lib, s, p, lp, st, cmds, H, 6, 40, None)
    s.close()


def test_a_mixed_fleet_equals_its_parts_on_the_lane_kernel(pkg, lib):
    N, H = 10, 20480
    p = _params(pkg, lib, N)
    lp, st, cmds = _fleet(pkg, lib, 2 * H, seed=44)
    s = _solver(pkg, lib, p, 2 * H, auto=True)
    _mixed_fleet(pkg, lib, s, p, lp, st, cmds, H, 3, 9, "lane_handoff")
    s.close()


# ---- 3. the two launch forms agree byte for byte; 6. outcome records too, pushes that never act ----------------------------------
@pytest.mark.parametrize("robots,ticks,horizon", [(200, 60, 10), (96, 40, 20)])
def test_launch_forms_give_the_same_bits(robots, ticks, horizon):
    worker = Path(__file__).resolve().parent / "_loop_warm_records_worker.py"
    out = {}
    for fused in ("0", "1"):
        env = dict(os.environ, QMPC_LOOP_FUSED=fused)
        r = subprocess.run([sys.executable, str(worker), str(robots), str(ticks), str(horizon)], env=env, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        out[fused] = {l.split()[0]: l.split()[1:] for l in r.stdout.splitlines() if l.startswith(("FORM", "SHA"))}
    print(out)
    f0, f1 = " ".join(out["0"]["FORM"]), " ".join(out["1"]["FORM"])
    assert f0.startswith("('per_tick'") and f1.startswith("('persistent'")
    assert f0.split("LAST")[0].split(",")[1] == f1.split("LAST")[0].split(",")[1]      # the same solve variant in both forms
    for key in ("SHA_INSTANCES", "SHA_OUTCOME_STATES", "SHA_OUTCOME_RECORDS", "SHA_PUSH"):
        assert out["0"][key] == out["1"][key], key
    for o in out.values():
        assert int(o["SHA_INSTANCES"][2]) > 0                                     # swing phases happened
        assert o["SHA_OUTCOME_STATES"][0] == o["SHA_INSTANCES"][0]                # the outcome call gives the instances call's bytes
        assert o["SHA_PUSH"][0] == o["SHA_PUSH"][2]                               # windows that never act: the outcome call's bytes


# ---- 4. wave form against lane form ------------------------------------------------------------------------------------------------
def test_warm_ticks_against_the_wave_family(pkg, lib):
    N, B = 10, 20480
    p = _params(pkg, lib, N)
    lp, st, cmds = _fleet(pkg, lib, B, seed=45)
    ctrl = pkg.random_go1_variants(B, seed=27, base=p)
    ctrl["mu"] = np.maximum(ctrl["mu"], 0.5)
    plant = pkg.random_go1_plants(B, seed=28, base=p, force=(0.0, 10.0))
    s = _solver(pkg, lib, p, B)
    run = lambda x, t, tr: s.loop_run_instances(x, t, lp, ctrl=ctrl, plant=plant, trace=tr)      # noqa: E731
    x = _walk(run, st, cmds, 4, 9)[0]      # walking: some feet swing
    xw, fw, cw = run(x, 2, True)           # a cold tick, then ONE warm-started tick
    assert _last(pkg, s) == "wform_ws" and s.loop_instances_plan(B, True, True) == ("per_tick", "wform_ws")
    s.set_instances_policy("auto")
    assert s.loop_instances_plan(B, True, True) == ("per_tick", "lane_handoff")
    xa, fa, ca = run(x, 2, True)
    assert _last(pkg, s) == "lane_handoff"
    s.close()
    assert (cw == 0).any() and _same(ca, cw)
    limit = (xa["iterations"] == p.iterations_max) | (xw["iterations"] == p.iterations_max)
    both = (xa["status"] == pkg.OK) & (xw["status"] == pkg.OK)
    err = np.abs(fa[1] - fw[1]).max(axis=1)
    print(f"the warm tick, {B} robots: {int(limit.sum())} robots at the iteration limit left out, {int(both.sum())} converged in both, "
          f"worst force difference there {err[both & ~limit].max():.2e} N (all robots: {err.max():.2e}); iterations wave "
          f"{xw['iterations'].mean():.2f} lane {xa['iterations'].mean():.2f}")
    assert limit.sum() <= B // 100
    assert np.array_equal(xa["status"][~limit], xw["status"][~limit])
    assert both.mean() > 0.9 and err[both & ~limit].max() <= 1e-7


# ---- 5. the start-cold rule: robots that do not solve, and their neighbours -----------------------------------------------------------
@pytest.mark.parametrize("fused,auto", [("0", False), ("1", False), ("0", True)])
def test_frozen_and_halted_robots_leave_their_neighbours_alone(pkg, lib, monkeypatch, fused, auto):
    monkeypatch.setenv("QMPC_LOOP_FUSED", fused)
    if auto:      # the lane form at a small size
        monkeypatch.setenv("QMPC_LANE_INST_MIN", "1")
        monkeypatch.setenv("QMPC_LANE_MIN", "1")
    N, B, T0, T = 10, 130, 6, 30
    p = _params(pkg, lib, N)
    lp, st, cmds = _fleet(pkg, lib, B, seed=46)
    ctrl = pkg.random_go1_variants(B, seed=30, base=p)
    ctrl["mu"] = np.maximum(ctrl["mu"], 0.5)
    plant = pkg.random_go1_plants(B, seed=31, base=p, force=(0.0, 10.0))
    push = pkg.push_params(B, 1)
    push["start_tick"] = T0 + 5.0; push["ticks"] = 4.0
    push["force_world"][:, 0, 1] = 20.0
    op = pkg.default_outcome_params(lib, stop_when_down=True)
    bad_c, bad_p, bad_w, falls = 3, 8, 20, 33
    ctrl2, plant2, push2 = ctrl.copy(), plant.copy(), push.copy()
    ctrl2["mu"][bad_c] = -1.0                               # a rejected controller record
    plant2["inertia"][bad_p] = 0.0                          # a rejected plant record
    push2["force_world"][bad_w, 0, 2] = np.inf              # an invalid push window
    plant2["ext_force_world"][falls, 2] = -1000.0           # goes down and is halted (tests/test_gpu_loop_outcome.py)
    s = _solver(pkg, lib, p, B, auto=auto)
    want_form = ("persistent" if fused == "1" else "per_tick")
    assert s.loop_instances_plan(B, True, True)[0] == want_form

    def walk(c, q, w):
        x0, oc = s.loop_run_pushes(st, T0, w, lp, ctrl=c, plant=q, op=op)
        x0["movement_mode"] = cmds[:, 6]
        return (x0,) + s.loop_run_pushes(x0, T, w, lp, ctrl=c, plant=q, op=op, outcomes=oc, trace=True)

    base = walk(ctrl, plant, push)
    got = walk(ctrl2, plant2, push2)
    if auto:
        assert _last(pkg, s).startswith("lane")
    s.close()
    x0, x, oc, tf, tc = got
    for i in (bad_c, bad_p, bad_w):      # frozen: state untouched except status and iterations, zero trace rows
        a, b = st[i].copy(), x[i]
        assert b["status"] == pkg.BAD_PARAMS and b["iterations"] == 0 and b["tick"] == 0
        a["status"], a["iterations"], a["movement_mode"] = b["status"], b["iterations"], cmds[i, 6]      # (set between the two calls)
        assert a.tobytes() == b.tobytes()
        assert (tf[:, i] == 0).all() and (tc[:, i] == 0).all()
    # halted after its down tick (1000 N of load against 400 N of lift: down within the call): state.tick stays there, zero
    # trace rows from then on
    dt = int(oc["down_tick"][falls])
    assert T0 < dt < T0 + T, dt
    assert x["tick"][falls] == dt and (tf[dt - T0:, falls] == 0).all() and (tc[dt - T0:, falls] == 0).all()
    assert (tf[:dt - T0, falls] != 0).any()
    assert (oc["down_tick"][np.arange(B) != falls] == -1).all()
    rest = np.setdiff1d(np.arange(B), [bad_c, bad_p, bad_w, falls])
    assert (x["tick"][rest] == T0 + T).all() and (tc[:, rest] == 0).any()
    assert _same(x[rest], base[1][rest]) and _same(oc[rest], base[2][rest])
    assert _same(tf[:, rest], base[3][:, rest]) and _same(tc[:, rest], base[4][:, rest])
    assert not _same(tf[:, bad_c], base[3][:, bad_c])


# ---- 6. the other entry points (both forms: the worker above); 7. buffers and defaults -----------------------------------------------
def test_buffers_defaults_and_the_device_entry_points(pkg, lib, monkeypatch):
    """ticks = 0 allocates everything (checked through QMPC_QUERY_DEVICE_BYTES before and after the calls that follow); a handle
    that never opted in holds what it held; the flag set back restores the refusal; device entry points against host ones."""
    import torch

    monkeypatch.setenv("QMPC_LOOP_FUSED", "0")
    N, B, TT = 10, 200, 8
    p = _params(pkg, lib, N)
    lp, st, cmds = _fleet(pkg, lib, B, seed=47)
    st["movement_mode"] = cmds[:, 6]
    ctrl = pkg.random_go1_variants(B, seed=33, base=p)
    ctrl["mu"] = np.maximum(ctrl["mu"], 0.5)
    plant = pkg.random_go1_plants(B, seed=34, base=p)
    push = pkg.push_params(B, 1)
    push["start_tick"] = 2.0; push["ticks"] = 3.0; push["force_world"][:, 0, 0] = 15.0
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1).copy()).cuda()      # noqa: E731

    # a handle that never opts in: the refusal, and the bytes it held before there was a setting
    w = pkg.Solver(p, B, device=0, lib=lib)
    assert not w.loop_warm_records() and w.loop_instances_plan(B, True, True) is None
    with pytest.raises(pkg.QmpcError) as e:
        w.loop_run_instances(st, TT, lp, ctrl=ctrl)
    assert e.value.code == pkg.UNSUPPORTED
    lp0 = pkg.default_loop_params(lib)
    w.loop_run_instances(st, 0, lp0, ctrl=ctrl, plant=plant)
    w.loop_run_instances(st, TT, lp0, ctrl=ctrl, plant=plant)
    w.loop_run_instances(st, TT, lp, plant=plant)
    never = w.query(pkg.QUERY_DEVICE_BYTES)
    w.close()

    s = pkg.Solver(p, B, device=0, lib=lib)
    fresh = s.query(pkg.QUERY_DEVICE_BYTES)
    s.set_loop_warm_records(True)
    assert s.loop_warm_records() and s.query(pkg.QUERY_DEVICE_BYTES) == fresh      # the setter allocates nothing
    # ticks = 0 allocates: the per-instance and plant blocks (1028 B per robot) and the trajectory buffer (96 N B per robot)
    assert _same(s.loop_run_instances(st, 0, lp, ctrl=ctrl, plant=plant), st)
    held = s.query(pkg.QUERY_DEVICE_BYTES)
    assert held - fresh == (1028 + 96 * N) * B
    # ... and the calls that follow allocate nothing more on the device side (what a capture by the caller needs)
    d_st, d_ctrl, d_plant = dev(st), dev(ctrl), dev(plant)
    d_tf = torch.full((TT, B, 12), 7.0, dtype=torch.float64, device="cuda")
    d_tc = torch.full((TT, B, 4), 7.0, dtype=torch.float64, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    s.loop_run_instances_device(B, d_st.data_ptr(), TT, lp, d_ctrl=d_ctrl.data_ptr(), d_plant=d_plant.data_ptr(),
                                d_trace_forces=d_tf.data_ptr(), d_trace_contacts=d_tc.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    assert s.query(pkg.QUERY_DEVICE_BYTES) == held
    want = s.loop_run_instances(st, TT, lp, ctrl=ctrl, plant=plant, trace=True)
    assert _last(pkg, s) == s.loop_instances_plan(B, True, True)[1] and _last(pkg, s).startswith("wform")
    assert (want[0]["status"] == 0).all() and (want[0]["tick"] == TT).all()
    # the device-buffer entry points give the host-buffer ones' bytes: instances, outcomes, pushes
    assert d_st.cpu().numpy().tobytes() == want[0].tobytes() and _same(d_tf.cpu().numpy(), want[1]) and _same(d_tc.cpu().numpy(), want[2])
    wo = s.loop_run_outcomes(st, TT, lp, ctrl=ctrl, plant=plant, trace=True)
    wp = s.loop_run_pushes(st, TT, push, lp, ctrl=ctrl, plant=plant, trace=True)
    assert _same(wo[0], want[0]) and _same(wo[2], want[1]) and _same(wo[3], want[2])      # the outcome call: the instances call's bytes
    assert not _same(wp[0], wo[0]) and (wp[0]["status"] == 0).all()                       # these windows act
    for host, d_push in ((wo, None), (wp, dev(push.reshape(B)))):
        d_st, d_oc = dev(st), dev(pkg.loop_outcomes(B, lib))
        d_tf.fill_(7.0); d_tc.fill_(7.0)
        torch.cuda.synchronize()
        if d_push is None:
            s.loop_run_outcomes_device(B, d_st.data_ptr(), TT, d_oc.data_ptr(), lp, d_ctrl=d_ctrl.data_ptr(), d_plant=d_plant.data_ptr(),
                                       d_trace_forces=d_tf.data_ptr(), d_trace_contacts=d_tc.data_ptr(), stream=stream.cuda_stream)
        else:
            s.loop_run_pushes_device(B, d_st.data_ptr(), TT, d_oc.data_ptr(), d_push.data_ptr(), 1, lp, d_ctrl=d_ctrl.data_ptr(),
                                     d_plant=d_plant.data_ptr(), d_trace_forces=d_tf.data_ptr(), d_trace_contacts=d_tc.data_ptr(),
                                     stream=stream.cuda_stream)
        stream.synchronize()
        assert d_st.cpu().numpy().tobytes() == host[0].tobytes() and d_oc.cpu().numpy().tobytes() == host[1].tobytes()
        assert _same(d_tf.cpu().numpy(), host[2]) and _same(d_tc.cpu().numpy(), host[3])
    # setting the flag back restores the refusal, for every entry point, and the plan's answer
    s.set_loop_warm_records(False)
    assert not s.loop_warm_records() and s.loop_instances_plan(B, True, True) is None
    for call in (lambda: s.loop_run_instances(st, TT, lp, ctrl=ctrl), lambda: s.loop_run_outcomes(st, TT, lp, ctrl=ctrl),
                 lambda: s.loop_run_pushes(st, TT, push, lp, ctrl=ctrl)):
        with pytest.raises(pkg.QmpcError) as e:
            call()
        assert e.value.code == pkg.UNSUPPORTED
    with pytest.raises(pkg.QmpcError) as e:
        s.set_loop_warm_records(2)
    assert e.value.code == pkg.BAD_ARGUMENT
    s.close()
    # what a handle that never opted in holds after the same calls an earlier library could serve: the blocks and nothing new
    # (the trajectory buffer there is the plain warm tick's, which the plant-only warm call always allocated)
    print(f"device bytes: fresh {fresh}, opted in after ticks = 0 {held}, never opted in {never}")
    assert never - fresh == (1028 + 96 * N + 8 * 820) * B      # ... and the host-buffer calls' staging of the states


@pytest.mark.parametrize("fused", ["0", "1"])
def test_ticks_zero_then_a_capture_by_the_caller(pkg, lib, monkeypatch, fused):
    """After a call with ticks = 0 the device entry point runs inside a stream capture of the CALLER's: nothing is allocated, no
    capture is begun inside the caller's, and the trace row counter is reset by a node of the caller's graph.  The graph replayed
    once gives the bytes of the eager call.  The counter is left at TT - 1 by an eager call before the capture, and the trace
    buffers carry TT + 2 rows more than the call writes: a reset that did not act would show in those rows, inside the buffers."""
    import torch

    monkeypatch.setenv("QMPC_LOOP_FUSED", fused)
    N, B, TT = 10, 200, 8
    ROWS = 2 * TT + 2
    p = _params(pkg, lib, N)
    lp, st, cmds = _fleet(pkg, lib, B, seed=48)
    st["movement_mode"] = cmds[:, 6]
    ctrl = pkg.random_go1_variants(B, seed=35, base=p)
    ctrl["mu"] = np.maximum(ctrl["mu"], 0.5)
    plant = pkg.random_go1_plants(B, seed=36, base=p)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1).copy()).cuda()      # noqa: E731
    s = _solver(pkg, lib, p, B)
    assert s.loop_instances_plan(B, True, True)[0] == ("persistent" if fused == "1" else "per_tick")
    assert _same(s.loop_run_instances(st, 0, lp, ctrl=ctrl, plant=plant), st)
    held = s.query(pkg.QUERY_DEVICE_BYTES)
    d_ctrl, d_plant = dev(ctrl), dev(plant)
    stream = torch.cuda.Stream()

    def buffers():
        return (dev(st), torch.full((ROWS, B, 12), 7.0, dtype=torch.float64, device="cuda"),
                torch.full((ROWS, B, 4), 7.0, dtype=torch.float64, device="cuda"))

    def call(d_st, d_tf, d_tc):
        s.loop_run_instances_device(B, d_st.data_ptr(), TT, lp, d_ctrl=d_ctrl.data_ptr(), d_plant=d_plant.data_ptr(),
                                    d_trace_forces=d_tf.data_ptr(), d_trace_contacts=d_tc.data_ptr(), stream=stream.cuda_stream)

    e_st, e_tf, e_tc = buffers()
    torch.cuda.synchronize()
    call(e_st, e_tf, e_tc)      # eager: the reference, and it leaves the row counter at TT - 1
    stream.synchronize()
    assert (e_tf[TT:] == 7.0).all() and (e_tc[TT:] == 7.0).all() and not (e_tf[:TT] == 7.0).any()
    x = e_st.cpu().numpy().view(pkg.LOOP_STATE_DTYPE).reshape(B)
    assert (x["status"] == 0).all() and (x["tick"] == TT).all()
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
    written = [r for r in range(ROWS) if not (got[1][r] == 7.0).all()]
    print(f"QMPC_LOOP_FUSED={fused}: trace rows the replayed graph wrote: {written}")
    assert written == list(range(TT)) and (got[2][TT:] == 7.0).all()
    assert _same(got[0], e_st.cpu().numpy()) and _same(got[1], e_tf.cpu().numpy()) and _same(got[2], e_tc.cpu().numpy())
