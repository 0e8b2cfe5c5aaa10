"""GPU suite (-m gpu): warm-started closed loops with per-robot controller records on a ConvexMpc handle
(qmpc_set_convex_records + qmpc_set_convex_warm_records, include/qmpc.h).

A handle that opted in accepts lp->warm_start with ctrl in qmpc_loop_run_instances* / _outcomes* / _pushes*: the persistent kernel
(which always carried warm_t), the per-tick wave form (qmpc_solve_cw_inst_warm_kernel) and, with qmpc_set_convex_lane_records under
QMPC_INSTANCES_AUTO, the lane form (qmpc_lane_cinst_warm_kernel).  Every comparison is against code the library had before: the
plain warm-started ConvexMpc loop on handles that carry the same values (bytes), the other launch form (bytes), the wave family
against the lane family (status words, 1e-7 N: the cross-family bound of include/qmpc.h).

The conditions that keep a comparison from passing vacuously are checked on the reference run (the plain warm loop): every robot
reaches the last tick, at least 95 % end QMPC_OK, some feet swing and forces act, the warm start saves iterations against the
same call started cold (iterations_sum of the outcome records), and QMPC_QUERY_LAST_KERNEL names the expected family.

Sizes: QMPC_LOOP_FUSED=0 brings the per-tick wave form down to 200 robots (variant 3), 800 (5) and, at N = 20, 1100 (6);
QMPC_LANE_CINST_MIN=1 and QMPC_LANE_MIN=1 bring the lane form down to 65 robots (a tail across a wavefront) and 2500 (half-masked
wavefronts); 24576 robots is the default warm switch-over at N = 10 (the larger of the solve's 24576 and the plain warm loop's
18432)."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from records_fleet import convex_fleet as _fleet, same as _same, walk as _walk

pytestmark = pytest.mark.gpu

T0 = 6      # standing ticks before the robots walk
LANE_KNOBS = (("QMPC_LANE_CINST_MIN", "1"), ("QMPC_LANE_MIN", "1"), ("QMPC_LOOP_FUSED", "0"))


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


def _params(pkg, lib, N, mode=None):
    p = pkg.default_convex_params(N, pkg.MODE_CONVERGED if mode is None else mode, lib)
    p.ipm_mu0 = 1e-6
    return p


def _all_same(got, want):
    return len(got) == len(want) and all(_same(a, b) for a, b in zip(got, want))


def _last(pkg, s):
    return pkg.KERNEL_FAMILY[s.query(pkg.QUERY_LAST_KERNEL)]


def _solver(pkg, lib, p, B, lane=False):
    s = pkg.Solver(p, B, device=0, lib=lib)
    s.set_convex_records(True)
    s.set_convex_warm_records(True)
    if lane:
        s.set_instances_policy("auto")
        s.set_convex_lane_records(True)
    return s


def _check_reference(pkg, s, p, lp, st, cmds, ref, T, family):
    """the conditions on the plain warm loop's run `ref` (states, force trace, contact trace); the warm start was in effect: the
    same loop's outcome call (plant records only: the plain tick) sums fewer iterations than with warm_start = 0"""
    B = len(st)
    assert (ref[0]["tick"] == T0 + T).all() and (ref[0]["status"] == pkg.OK).mean() >= 0.95
    assert (ref[2] == 0).any() and (ref[1] != 0).any()
    # (the plain loop's ticks leave QMPC_QUERY_LAST_KERNEL alone: its plan is asked, and the records call's last kernel after it)
    if family:
        assert s.loop_instances_plan(B, False, True) == ("per_tick", family), s.loop_instances_plan(B, False, True)
    plant = pkg.plant_params(p, B)
    lp0 = pkg.default_loop_params(s.lib)
    x0 = s.loop_run(st, T0, lp)
    x0["movement_mode"] = cmds[:, 6]
    warm = s.loop_run_outcomes(x0, T, lp, plant=plant)[1]["iterations_sum"].sum()
    cold = s.loop_run_outcomes(x0, T, lp0, plant=plant)[1]["iterations_sum"].sum()
    print(f"B={B}: iterations over {T} ticks warm {warm:.0f} cold {cold:.0f}")
    assert warm < cold


# ---- 1. uniform records give the plain warm loop's bytes -----------------------------------------------------------------------
@pytest.mark.parametrize("N,B,T,knobs,form,family", [
    (10, 40, 30, (), "persistent", None), (20, 40, 30, (), "persistent", None),
    (10, 200, 20, (("QMPC_LOOP_FUSED", "0"),), "per_tick", "wform_lds"),
    (10, 800, 20, (("QMPC_LOOP_FUSED", "0"),), "per_tick", "wform_ws"),
    (20, 1100, 12, (("QMPC_LOOP_FUSED", "0"),), "per_tick", "wform_ws"),
    (10, 65, 20, LANE_KNOBS, "per_tick", "lane"), (10, 2500, 20, LANE_KNOBS, "per_tick", "lane"),
    (10, 24576, 15, (), "per_tick", "lane")])
def test_uniform_records_equal_the_plain_warm_loop(pkg, lib, monkeypatch, N, B, T, knobs, form, family):
    for k, v in knobs:
        monkeypatch.setenv(k, v)
    p = _params(pkg, lib, N)
    lp, st, cmds = _fleet(pkg, lib, B)
    s = _solver(pkg, lib, p, B, lane=family == "lane")
    assert s.loop_instances_plan(B, True, True) == (form, family) or (family is None and s.loop_instances_plan(B, True, True)[0] == form)
    if B == 24576:      # the default switch-over: one robot fewer stays on the wave kernels
        assert s.loop_instances_plan(B - 1, True, True) == ("per_tick", "wform_ws")
    if N == 20 and B == 1100:
        assert s.query(pkg.QUERY_LOOP_INSTANCES_PLAN, B | (3 << 32)) == 16 * 2 + 2
    ref = _walk(lambda x, t, tr: s.loop_run(x, t, lp, trace=tr), st, cmds, T0, T)
    _check_reference(pkg, s, p, lp, st, cmds, ref, T, family)
    ctrl, plant = pkg.instance_params(p, B), pkg.plant_params(p, B)
    got = _walk(lambda x, t, tr: s.loop_run_instances(x, t, lp, ctrl=ctrl, plant=plant, trace=tr), st, cmds, T0, T)
    if family:
        assert _last(pkg, s) == family
    only = _walk(lambda x, t, tr: s.loop_run_instances(x, t, lp, ctrl=ctrl, trace=tr), st, cmds, T0, T)
    s.close()
    assert _all_same(got, ref) and _all_same(only, ref)


# ---- 2. per-robot values reach the warm-started solve ----------------------------------------------------------------------------
@pytest.mark.parametrize("B,knobs,family", [(256, (("QMPC_LOOP_FUSED", "0"),), "wform_lds"), (260, LANE_KNOBS, "lane")])
def test_a_mixed_fleet_equals_its_parts_and_its_permutation(pkg, lib, monkeypatch, B, knobs, family):
    for k, v in knobs:
        monkeypatch.setenv(k, v)
    T, N = 20, 10
    p = _params(pkg, lib, N)
    lp, st, cmds = _fleet(pkg, lib, B, seed=5)
    sets = pkg.random_go1_convex_variants(2, seed=9, base=p)
    sets["mu"] = np.maximum(sets["mu"], 0.5)
    ctrl = sets[np.arange(B) % 2]
    s = _solver(pkg, lib, p, B, lane=family == "lane")
    assert s.loop_instances_plan(B, True, True) == ("per_tick", family)
    run = lambda c: (lambda x, t, tr: s.loop_run_instances(x, t, lp, ctrl=c, trace=tr))      # noqa: E731
    fleet = _walk(run(ctrl), st, cmds, T0, T)
    assert _last(pkg, s) == family
    perm = np.random.default_rng(2).permutation(B)
    shuf = _walk(run(ctrl[perm]), st[perm], cmds[perm], T0, T)
    s.close()
    assert _same(shuf[0], fleet[0][perm]) and _same(shuf[1], fleet[1][:, perm]) and _same(shuf[2], fleet[2][:, perm])
    for g in range(2):      # a plain warm loop on a handle carrying the set: controller and plant are the set's robot
        idx = np.arange(g, B, 2)
        one = pkg.Solver(pkg.params_with(p, sets[g]), len(idx), device=0, lib=lib)
        one.set_convex_records(True)      # (for the outcome call of _check_reference; the plain loop does not read it)
        want = _walk(lambda x, t, tr: one.loop_run(x, t, lp, trace=tr), st[idx], cmds[idx], T0, T)
        _check_reference(pkg, one, pkg.params_with(p, sets[g]), lp, st[idx], cmds[idx], want, T, family)
        one.close()
        assert _same(want[0], fleet[0][idx]) and _same(want[1], fleet[1][:, idx]) and _same(want[2], fleet[2][:, idx]), g
    assert not _same(fleet[1][:, 0::2], fleet[1][:, 1::2])


# ---- 3. the two launch forms agree byte for byte, outcome records included ----------------------------------------------------------
@pytest.mark.parametrize("robots,ticks,horizon", [(200, 40, 10), (96, 40, 20)])
def test_launch_forms_give_the_same_bits(robots, ticks, horizon):
    worker = Path(__file__).resolve().parent / "_convex_warm_records_worker.py"
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
    for key in ("SHA_INSTANCES", "SHA_OUTCOME_STATES", "SHA_OUTCOME_RECORDS", "SHA_PUSH", "SHA_PUSH_RECORDS"):
        assert out["0"][key] == out["1"][key], key
    for o in out.values():
        assert int(o["SHA_INSTANCES"][2]) > 0                                     # swing phases happened
        assert o["SHA_OUTCOME_STATES"][0] == o["SHA_INSTANCES"][0]                # the outcome call gives the instances call's bytes
        assert o["SHA_PUSH"][0] != o["SHA_INSTANCES"][0] and int(o["SHA_PUSH"][2]) > 0      # the windows act, robots were halted


# ---- 4. wave form against lane form ----------------------------------------------------------------------------------------------
def test_a_warm_tick_against_the_wave_family(pkg, lib, monkeypatch):
    for k, v in LANE_KNOBS:
        monkeypatch.setenv(k, v)
    N, B = 10, 2500
    p = _params(pkg, lib, N)
    lp, st, cmds = _fleet(pkg, lib, B, seed=45)
    ctrl = pkg.random_go1_convex_variants(B, seed=27, base=p)
    ctrl["mu"] = np.maximum(ctrl["mu"], 0.5)
    plant = pkg.random_go1_plants(B, seed=28, base=p, force=(0.0, 10.0))
    s = _solver(pkg, lib, p, B)
    run = lambda x, t, tr: s.loop_run_instances(x, t, lp, ctrl=ctrl, plant=plant, trace=tr)      # noqa: E731
    x = _walk(run, st, cmds, 4, 9)[0]      # walking: some feet swing
    xw, fw, cw = run(x, 2, True)           # a cold tick, then ONE warm-started tick
    assert _last(pkg, s) == "wform_ws" and s.loop_instances_plan(B, True, True) == ("per_tick", "wform_ws")
    s.set_instances_policy("auto")
    assert s.loop_instances_plan(B, True, True) == ("per_tick", "wform_ws")      # (the lane form is a setting of its own)
    s.set_convex_lane_records(True)
    assert s.loop_instances_plan(B, True, True) == ("per_tick", "lane")
    xa, fa, ca = run(x, 2, True)
    assert _last(pkg, s) == "lane"
    xc = s.loop_run_instances(x, 2, pkg.default_loop_params(lib), ctrl=ctrl, plant=plant)      # the same two ticks started cold
    s.close()
    assert (cw == 0).any() and _same(ca, cw) and (xw["status"] == pkg.OK).mean() >= 0.95 and (xw["tick"] == 15).all()
    err = np.abs(fa[1] - fw[1]).max()
    print(f"the warm tick, {B} robots: worst force difference {err:.2e} N; iterations wave {xw['iterations'].mean():.2f} lane "
          f"{xa['iterations'].mean():.2f} cold {xc['iterations'].mean():.2f}")
    assert xw["iterations"].sum() < xc["iterations"].sum()
    assert np.array_equal(xa["status"], xw["status"])
    assert err <= 1e-7


# ---- 5. robots that do not solve, and their neighbours ---------------------------------------------------------------------------------
@pytest.mark.parametrize("fused,lane", [("0", False), ("1", False), ("0", True)])
def test_frozen_and_halted_robots_leave_their_neighbours_alone(pkg, lib, monkeypatch, fused, lane):
    monkeypatch.setenv("QMPC_LOOP_FUSED", fused)
    if lane:
        monkeypatch.setenv("QMPC_LANE_CINST_MIN", "1")
        monkeypatch.setenv("QMPC_LANE_MIN", "1")
    N, B, T = 10, 130, 30
    p = _params(pkg, lib, N)
    lp, st, cmds = _fleet(pkg, lib, B, seed=46)
    ctrl = pkg.random_go1_convex_variants(B, seed=30, base=p)
    ctrl["mu"] = np.maximum(ctrl["mu"], 0.5)
    plant = pkg.random_go1_plants(B, seed=31, base=p, force=(0.0, 10.0))
    push = pkg.push_params(B, 1)
    push["start_tick"] = T0 + 5.0; push["ticks"] = 4.0
    push["force_world"][:, 0, 1] = 20.0
    op = pkg.default_outcome_params(lib, stop_when_down=True)
    bad_c, bad_p, bad_w, falls, nan_s = 3, 8, 20, 33, 50
    ctrl2, plant2, push2, st2 = ctrl.copy(), plant.copy(), push.copy(), st.copy()
    ctrl2["mu"][bad_c] = -1.0                               # a rejected controller record
    plant2["inertia"][bad_p] = 0.0                          # a rejected plant record
    push2["force_world"][bad_w, 0, 2] = np.inf              # an invalid push window
    plant2["ext_force_world"][falls, 2] = -1000.0           # goes down and is halted (tests/test_gpu_loop_outcome.py)
    st2["pos_world"][nan_s, 0] = np.nan                     # every solve of this robot fails (QMPC_NAN_INPUT): each starts cold
    s = _solver(pkg, lib, p, B, lane=lane)
    assert s.loop_instances_plan(B, True, True) == (("persistent", "wform_lds") if fused == "1" else ("per_tick", "lane" if lane else "wform_lds"))

    def walk(x, c, q, w):
        x0, oc = s.loop_run_pushes(x, T0, w, lp, ctrl=c, plant=q, op=op)
        x0["movement_mode"] = cmds[:, 6]
        return (x0,) + s.loop_run_pushes(x0, T, w, lp, ctrl=c, plant=q, op=op, outcomes=oc, trace=True)

    base = walk(st, ctrl, plant, push)
    if fused == "0":
        assert _last(pkg, s) == ("lane" if lane else "wform_lds")
    got = walk(st2, ctrl2, plant2, push2)
    s.close()
    x0, x, oc, tf, tc = got
    for i in (bad_c, bad_p, bad_w):      # frozen: state untouched except status and iterations, zero trace rows
        a, b = st[i].copy(), x[i]
        assert b["status"] == pkg.BAD_PARAMS and b["iterations"] == 0 and b["tick"] == 0
        a["status"], a["iterations"], a["movement_mode"] = b["status"], b["iterations"], cmds[i, 6]      # (set between the two calls)
        assert a.tobytes() == b.tobytes()
        assert (tf[:, i] == 0).all() and (tc[:, i] == 0).all()
    dt = int(oc["down_tick"][falls])
    assert T0 < dt < T0 + T, dt
    assert x["tick"][falls] == dt and (tf[dt - T0:, falls] == 0).all() and (tc[dt - T0:, falls] == 0).all()
    assert (tf[:dt - T0, falls] != 0).any()
    assert x["status"][nan_s] == pkg.NAN_INPUT
    rest = np.setdiff1d(np.arange(B), [bad_c, bad_p, bad_w, falls, nan_s])
    assert (base[1]["tick"] == T0 + T).all() and (base[1]["status"] == pkg.OK).mean() >= 0.95 and (base[4] == 0).any() and (base[3] != 0).any()
    assert _same(x[rest], base[1][rest]) and _same(oc[rest], base[2][rest])
    assert _same(tf[:, rest], base[3][:, rest]) and _same(tc[:, rest], base[4][:, rest])
    assert not _same(tf[:, bad_c], base[3][:, bad_c])


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_keep_their_codes(pkg, lib):
    B = 65
    p = _params(pkg, lib, 10)
    lp, st, _ = _fleet(pkg, lib, B)
    ctrl, plant = pkg.instance_params(p, B), pkg.plant_params(p, B)
    push = pkg.push_params(B, 1)

    def code(call):
        with pytest.raises(pkg.QmpcError) as e:
            call()
        return e.value.code

    def calls(s):
        return (lambda: s.loop_run_instances(st, 2, lp, ctrl=ctrl, plant=plant), lambda: s.loop_run_outcomes(st, 2, lp, ctrl=ctrl),
                lambda: s.loop_run_pushes(st, 2, push, lp, ctrl=ctrl))

    s = pkg.Solver(p, B, device=0, lib=lib)
    assert not s.convex_warm_records()
    # without the new setting: refused, whatever qmpc_set_loop_warm_records says
    s.set_convex_records(True)
    s.set_loop_warm_records(True)
    assert s.loop_instances_plan(B, True, True) is None
    assert all(code(c) == pkg.UNSUPPORTED for c in calls(s))
    # with it but without qmpc_set_convex_records: refused
    s.set_convex_records(False)
    s.set_convex_warm_records(True)
    assert s.convex_warm_records() and s.loop_instances_plan(B, True, True) is None
    assert all(code(c) == pkg.UNSUPPORTED for c in calls(s))
    # both on, and qmpc_set_loop_warm_records off: accepted
    s.set_convex_records(True)
    s.set_loop_warm_records(False)
    assert s.loop_instances_plan(B, True, True) == ("persistent", "wform_lds")
    for c in calls(s):
        c()
    # bad setter values
    for v in (2, -1):
        assert code(lambda: s.set_convex_warm_records(v)) == pkg.BAD_ARGUMENT
    assert lib.qmpc_set_convex_warm_records(None, 1) == pkg.BAD_ARGUMENT and s.convex_warm_records()
    s.set_convex_warm_records(False)
    assert not s.convex_warm_records() and all(code(c) == pkg.UNSUPPORTED for c in calls(s))
    s.close()
    # the reference mode
    r = _solver(pkg, lib, _params(pkg, lib, 10, pkg.MODE_REFERENCE), B)
    assert r.loop_instances_plan(B, True, True) is None and all(code(c) == pkg.UNSUPPORTED for c in calls(r))
    r.close()
    # a knot spacing other than the controller period of 5 ms
    ph = _params(pkg, lib, 10)
    ph.h = 0.01
    r = _solver(pkg, lib, ph, B)
    assert all(code(c) == pkg.UNSUPPORTED for c in calls(r))
    r.close()
    # the setting does nothing on a handle of another model
    q = pkg.Solver(pkg.default_params(10, pkg.MODE_CONVERGED, lib), B, device=0, lib=lib)
    q.set_convex_warm_records(True)
    assert q.loop_instances_plan(B, True, True) is None
    assert code(lambda: q.loop_run_instances(st, 2, lp, ctrl=ctrl)) == pkg.UNSUPPORTED
    q.close()


# ---- 7. ticks = 0, then a capture by the caller ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", ["0", "1"])
def test_ticks_zero_then_a_capture_by_the_caller(pkg, lib, monkeypatch, fused):
    """After a call with ticks = 0 the device entry point runs inside a stream capture of the CALLER's: nothing is allocated, and the
    graph replayed once gives the bytes of the eager call (tests/test_gpu_loop_warm_records.py has the QuatMpc twin)."""
    import torch

    monkeypatch.setenv("QMPC_LOOP_FUSED", fused)
    N, B, TT = 10, 200, 8
    ROWS = 2 * TT + 2
    p = _params(pkg, lib, N)
    lp, st, cmds = _fleet(pkg, lib, B, seed=48)
    st["movement_mode"] = cmds[:, 6]
    ctrl = pkg.random_go1_convex_variants(B, seed=35, base=p)
    ctrl["mu"] = np.maximum(ctrl["mu"], 0.5)
    plant = pkg.random_go1_plants(B, seed=36, base=p)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1).copy()).cuda()      # noqa: E731
    s = _solver(pkg, lib, p, B)
    assert s.loop_instances_plan(B, True, True) == (("persistent" if fused == "1" else "per_tick"), "wform_lds")
    fresh = s.query(pkg.QUERY_DEVICE_BYTES)
    assert _same(s.loop_run_instances(st, 0, lp, ctrl=ctrl, plant=plant), st)
    held = s.query(pkg.QUERY_DEVICE_BYTES)
    if fused == "0":      # the trajectory buffer the solution travels through: 96 N B per robot
        s0 = _solver(pkg, lib, p, B)
        s0.loop_run_instances(st, 0, pkg.default_loop_params(lib), ctrl=ctrl, plant=plant)
        assert held - fresh == s0.query(pkg.QUERY_DEVICE_BYTES) - fresh + 96 * N * B
        s0.close()
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
    assert (x["status"] == 0).mean() >= 0.95 and (x["tick"] == TT).all()
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
    assert written == list(range(TT)) and (got[2][TT:] == 7.0).all()
    assert _same(got[0], e_st.cpu().numpy()) and _same(got[1], e_tf.cpu().numpy()) and _same(got[2], e_tc.cpu().numpy())


# ---- 8. the device entry points equal the host calls -----------------------------------------------------------------------------------
@pytest.mark.parametrize("lane", [False, True])
def test_the_device_entry_points_equal_the_host_calls(pkg, lib, monkeypatch, lane):
    import torch

    for k, v in (LANE_KNOBS if lane else (("QMPC_LOOP_FUSED", "0"),)):
        monkeypatch.setenv(k, v)
    N, B, TT = 10, 200, 8
    p = _params(pkg, lib, N)
    lp, st, cmds = _fleet(pkg, lib, B, seed=47)
    st["movement_mode"] = cmds[:, 6]
    ctrl = pkg.random_go1_convex_variants(B, seed=33, base=p)
    ctrl["mu"] = np.maximum(ctrl["mu"], 0.5)
    plant = pkg.random_go1_plants(B, seed=34, base=p)
    push = pkg.push_params(B, 1)
    push["start_tick"] = 2.0; push["ticks"] = 3.0; push["force_world"][:, 0, 0] = 15.0
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1).copy()).cuda()      # noqa: E731
    s = _solver(pkg, lib, p, B, lane=lane)
    family = "lane" if lane else "wform_lds"
    assert s.loop_instances_plan(B, True, True) == ("per_tick", family)
    if lane:      # qmpc_prepare allocates what the lane form needs: the calls that follow allocate nothing on the device side
        s.prepare(B)
        s.prepare_instances()
    s.loop_run_instances(st, 0, lp, ctrl=ctrl, plant=plant)
    d_ctrl, d_plant = dev(ctrl), dev(plant)
    d_tf = torch.full((TT, B, 12), 7.0, dtype=torch.float64, device="cuda")
    d_tc = torch.full((TT, B, 4), 7.0, dtype=torch.float64, device="cuda")
    stream = torch.cuda.Stream()
    d_st = dev(st)
    torch.cuda.synchronize()
    held = s.query(pkg.QUERY_DEVICE_BYTES)
    s.loop_run_instances_device(B, d_st.data_ptr(), TT, lp, d_ctrl=d_ctrl.data_ptr(), d_plant=d_plant.data_ptr(),
                                d_trace_forces=d_tf.data_ptr(), d_trace_contacts=d_tc.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    assert s.query(pkg.QUERY_DEVICE_BYTES) == held and _last(pkg, s) == family
    want = s.loop_run_instances(st, TT, lp, ctrl=ctrl, plant=plant, trace=True)
    assert (want[0]["status"] == 0).mean() >= 0.95 and (want[0]["tick"] == TT).all()
    assert d_st.cpu().numpy().tobytes() == want[0].tobytes() and _same(d_tf.cpu().numpy(), want[1]) and _same(d_tc.cpu().numpy(), want[2])
    wo = s.loop_run_outcomes(st, TT, lp, ctrl=ctrl, plant=plant, trace=True)
    wp = s.loop_run_pushes(st, TT, push, lp, ctrl=ctrl, plant=plant, trace=True)
    assert _same(wo[0], want[0]) and _same(wo[2], want[1]) and _same(wo[3], want[2])      # the outcome call: the instances call's bytes
    assert not _same(wp[0], wo[0])                                                        # these windows act
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
    s.close()
