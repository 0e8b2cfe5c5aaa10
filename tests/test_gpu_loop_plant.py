"""GPU suite (-m gpu): every device build of the closed loop's post step against an independent reference.

The parity reference of the other closed-loop tests (host/ClosedLoopHost.h) includes csrc/qmpc_loop_math.h and so shares the
plant's one statement with the device.  Here the reference is tests/plant_reference.py: the model restated in numpy longdouble,
checked on its own and against the host build by tests/test_plant_reference_cpu.py, whose constants K (units of
2^-52 max(1, |reference|)) are imported, not re-tuned.

Method (tests/test_gpu_loop_outcome.py's _fleet and _chunks): 64 robots stand for 6 ticks, are perturbed on the host (a tilt of up
to 0.25 rad about a random body axis, N(0, 0.2) m/s, N(0, 0.5) rad/s; feet stay where they are; a tilt that would make w negative
is not applied: the quaternion sign cases are tests/test_plant_reference_cpu.py's), switch to their walking commands and advance in
ONE-TICK calls.  For every robot and tick the reference starts from the state before -- attitude, position, velocities,
foot_pos_world -- takes forces_body and contacts from the state after (the forces the tick applied), the mass and inertia of the
handle or the plant record, the effective wrench of the plant record and the push windows at the tick before, and must reproduce
the state after: plant state, forces in the other frame, swing-foot relocation, tick counter.  One T-tick cold call gives the bytes
of the T one-tick calls, which lets one-tick calls stand for the persistent kernel's many-tick launch.

T = 50 walking ticks, not 40: a leg that starts in swing lands at gait phase 0.45 .. 0.5, tick 41 .. 46 of the walk at 2.2 Hz and
5 ms, so a 40-tick walk has no landing to check.

Out of scope: the lane-kernel ticks from 16384 robots on (their post step is the per-tick kernel of the per-tick cases, and the
size does not fit a seconds-long test); the reference mode; the warm start (it changes the solve, not the plant)."""
import numpy as np
import pytest

import plant_reference as ref

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref.usable(), reason="np.longdouble carries fewer than 60 mantissa bits here")]

B, N, T0, T = 64, 10, 6, 50
TILT, DV, DW = 0.25, 0.2, 0.5
COMMANDS = [   # joy.{velx, vely, body_height, roll_rate, pitch_rate, yaw_rate}, movement_mode (tests/test_gpu_loop_outcome.py)
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


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _fleet(pkg, lib, convex, seed=1):
    """B robots standing at their initial poses (movement 0), yaw spread over (-3, 3), and the commands they walk with afterwards:
    tests/test_gpu_loop_outcome.py's for QuatMpc, tests/test_gpu_convex_records.py's (no roll / pitch rate) for ConvexMpc"""
    lp = pkg.default_loop_params(lib)
    rng = np.random.default_rng(seed)
    if convex:
        cmds = np.zeros((B, 7))
        cmds[:, 0] = 0.6 * rng.uniform(-0.5, 0.5, B); cmds[:, 1] = rng.uniform(-0.2, 0.2, B); cmds[:, 2] = rng.uniform(0.26, 0.32, B)
        cmds[:, 5] = rng.uniform(-0.5, 0.5, B); cmds[:, 6] = (rng.random(B) < 0.9).astype(float)
        cmds[cmds[:, 6] == 0, :2] = 0.0
        cmds[cmds[:, 6] == 0, 5] = 0.0
    else:
        cmds = np.array([COMMANDS[i % len(COMMANDS)] for i in range(B)])
        cmds[:, 0] += rng.uniform(-0.1, 0.1, B) * cmds[:, 6]
    stand = cmds.copy(); stand[:, 6] = 0.0
    st = pkg.loop_states(stand, lp, height=0.3, yaw=rng.uniform(-3, 3, B), lib=lib)
    return lp, st, cmds


def _perturb(st, seed=77):
    """tilt by a random body-axis rotation of up to TILT rad, add N(0, DV) m/s and N(0, DW) rad/s; feet stay"""
    rng = np.random.default_rng(seed)
    n = len(st)
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    ang = rng.uniform(0.0, TILT, n)
    dq = np.concatenate([np.cos(ang / 2)[:, None], np.sin(ang / 2)[:, None] * axis], axis=1)
    q = ref.quat_mul(st["quat"], dq)
    q = (q / np.sqrt((q * q).sum(axis=1, keepdims=True))).astype(np.float64)
    keep = q[:, 0] > 0
    st["quat"][keep] = q[keep]
    st["lin_vel_world"] += rng.normal(0.0, DV, (n, 3))
    st["ang_vel_body"] += rng.normal(0.0, DW, (n, 3))
    assert keep.sum() >= n - 8 and (st["quat"][:, 0] > 0).all()


def _plants(pkg, p):
    """robot i by i mod 8: the handle's robot (every field at the handle's value), heavier, lighter, a skewed inertia
    (test_device_equals_the_host_twin_under_model_mismatch's), a lateral force, a yaw torque, an unsymmetric inertia under a
    general wrench (where a transposed inverse would show), the handle's robot again"""
    plant = pkg.plant_params(p, B)
    k = np.arange(B) % 8
    I0 = np.asarray(p.inertia[:]).reshape(3, 3)
    plant["mass"][k == 1] += 3.0
    plant["mass"][k == 2] -= 2.0
    skewed = I0 * np.array([1.3, 0.8, 1.1])[:, None] ** 0.5 * np.array([1.3, 0.8, 1.1])[None, :] ** 0.5
    skewed[0, 1] = skewed[1, 0] = 0.002
    plant["inertia"][k == 3] = skewed.ravel()
    plant["ext_force_world"][k == 4] = [0.0, 12.0, 0.0]
    plant["ext_torque_body"][k == 5] = [0.0, 0.0, 0.8]
    uns = skewed.copy()
    uns[0, 1], uns[1, 0], uns[1, 2], uns[2, 1], uns[0, 2], uns[2, 0] = 0.004, 0.001, -0.003, 0.0005, 0.002, -0.001
    plant["inertia"][k == 6] = uns.ravel()
    plant["ext_force_world"][k == 6] = [3.0, -4.0, 5.0]
    plant["ext_torque_body"][k == 6] = [0.3, -0.2, 0.1]
    return plant


def _pushes(pkg):
    """two windows per robot over the walk (state.tick T0 .. T0 + T - 1): window 0 starts at the first walking tick and lasts 12
    ticks, window 1 starts 8 ticks later and lasts 10 -- they overlap for 4 ticks and both end mid-run; every fourth robot's
    second window has ticks = 0 and never acts; every third robot's second window carries a torque as well"""
    rng = np.random.default_rng(5)
    push = pkg.push_params(B, 2)
    for k, (start, ticks) in enumerate(((T0, 12), (T0 + 8, 10))):
        phi = rng.uniform(-np.pi, np.pi, B)
        push["start_tick"][:, k], push["ticks"][:, k] = start, ticks
        push["force_world"][:, k, 0], push["force_world"][:, k, 1] = 15.0 * np.cos(phi), 15.0 * np.sin(phi)
    push["torque_body"][::3, 1] = [0.0, -0.4, 0.5]
    push["ticks"][3::4, 1] = 0.0
    return push


# name, convex, entry point, plant records, push windows, QMPC_LOOP_FUSED, the form asserted
CASES = [
    ("quat_loop_run_persistent", False, "run", False, False, None, "persistent"),
    ("quat_loop_run_per_tick", False, "run", False, False, "0", "per_tick"),
    ("convex_loop_run", True, "run", False, False, None, None),
    ("instances_plant_persistent", False, "instances", True, False, None, "persistent"),
    ("instances_plant_per_tick", False, "instances", True, False, "0", "per_tick"),
    ("pushes", False, "pushes", True, True, None, "persistent"),
    ("convex_records_pushes", True, "pushes", True, True, None, "persistent"),
]


@pytest.mark.parametrize("name,convex,entry,with_plant,with_push,fused,form", CASES, ids=[c[0] for c in CASES])
def test_every_tick_is_the_reference_tick(pkg, lib, monkeypatch, name, convex, entry, with_plant, with_push, fused, form):
    if fused is not None:
        monkeypatch.setenv("QMPC_LOOP_FUSED", fused)      # read when the handle is created
    p = (pkg.default_convex_params if convex else pkg.default_params)(N, pkg.MODE_CONVERGED, lib)
    lp, st, cmds = _fleet(pkg, lib, convex)
    plant = _plants(pkg, p) if with_plant else None
    push = _pushes(pkg) if with_push else None
    s = pkg.Solver(p, B, device=0, lib=lib)
    if convex and entry != "run":
        s.set_convex_records(True)
    if form is not None:      # (a plain ConvexMpc handle has no plan to query: its case takes either form)
        assert s.loop_instances_plan(B, False, False)[0] == form

    def run(x, ticks):
        if entry == "run":
            return s.loop_run(x, ticks, lp)
        if entry == "instances":
            return s.loop_run_instances(x, ticks, lp, plant=plant)
        return s.loop_run_pushes(x, ticks, push, lp, plant=plant)[0]

    st0 = run(st, T0)
    st0["movement_mode"] = cmds[:, 6]
    _perturb(st0)
    seq, x = [], st0
    for _ in range(T):
        x = run(x, 1)
        seq.append(x)
    whole = run(st0, T)
    s.close()
    assert _same(whole, seq[-1])      # one T-tick cold call is the T one-tick calls

    if with_plant:
        mass, inertia = plant["mass"], plant["inertia"].reshape(B, 3, 3)
        force, torque = plant["ext_force_world"], plant["ext_torque_body"]
    else:
        mass, inertia = np.full(B, p.mass), np.broadcast_to(np.asarray(p.inertia[:]).reshape(3, 3), (B, 3, 3))
        force = torque = np.zeros((B, 3))

    worst = {g: 0.0 for g in list(ref.GROUPS) + ["norm", "grf_world", "forces_body"]}
    truncation = {g: 0.0 for g in ref.GROUPS}
    accepted_n = swing_n = landings = active_n = rejected_n = 0
    before = st0
    for after in seq:
        wf, wt, act = ref.effective_wrench(force, torque, push, before["tick"])
        want = ref.post_tick(before, after, mass, inertia, wf, wt, lp.dt)
        assert np.isfinite(ref.state13(after).astype(np.float64)).all()
        e = ref.units(ref.state13(after), want["x"]).astype(np.float64)
        for g, sl in ref.GROUPS.items():
            worst[g] = max(worst[g], float(e[:, sl].max()))
        worst["norm"] = max(worst["norm"], float((np.abs(np.sqrt((ref.ld(after["quat"]) ** 2).sum(axis=1)) - 1) / ref.U).max()))
        ok = (after["status"] == pkg.OK) | (after["status"] == pkg.MAX_ITER)
        fb, grf = after["forces_body"].reshape(B, 4, 3), after["grf_world"].reshape(B, 4, 3)
        # the applied forces in the other frame.  QuatMpc's tick rotates forces_body in every tick; ConvexMpc's tick writes both
        # frames only when the solve is accepted, so a rejected tick keeps both from the tick before (another attitude)
        rows = ok if convex else np.ones(B, dtype=bool)
        if rows.any():
            worst["grf_world"] = max(worst["grf_world"], float(ref.units_vec(grf[rows], want["grf_world"][rows]).max()))
            if convex:
                worst["forces_body"] = max(worst["forces_body"], float(ref.units_vec(fb[rows], want["body_of_grf"][rows]).max()))
        assert _same(after["forces_body"][~ok], before["forces_body"][~ok])      # a rejected solve: the previous forces stay
        if convex:
            assert _same(after["grf_world"][~ok], before["grf_world"][~ok])
        # swing feet sit at their FSM target, every other foot keeps its bytes; the counter advanced by one
        assert _same(after["foot_pos_world"].reshape(B, 4, 3), want["feet"])
        assert np.isin(after["contacts"], (0.0, 1.0)).all() and (after["contacts"][after["movement_mode"] == 0] == 1).all()
        assert np.array_equal(after["tick"], want["tick"])
        accepted_n += int((ok & (after["forces_body"] != 0).any(axis=1)).sum())
        rejected_n += int((~ok).sum())
        swing_n += int(want["swing"].any(axis=1).sum())
        landings += int(((before["contacts"] == 0) & (after["contacts"] == 1)).sum())
        active_n += int((act > 0).sum())
        if name == "quat_loop_run_persistent":      # the step's truncation error on these ticks (a figure for DESIGN.md, not a check)
            fine = ref.fine_step(ref.state13(before), fb, before["foot_pos_world"].reshape(B, 4, 3), mass, inertia, lp.dt, wf, wt, substeps=20)
            for g, sl in ref.GROUPS.items():
                truncation[g] = max(truncation[g], float(np.abs(fine - want["x"])[:, sl].max()))
        before = after

    print(f"{name}: worst error in units of 2^-52 max(1, |ref|): " + ", ".join(f"{g} {v:.3f}" for g, v in worst.items())
          + f"; accepted {accepted_n} of {B * T} robot-ticks ({rejected_n} rejected), {swing_n} with a swing leg, {landings} landings, "
          f"{active_n} with an active window" + ("; one-tick truncation error up to " + ", ".join(f"{g} {v:.2e}" for g, v in truncation.items()) if truncation["quat"] else ""))
    for g in ref.GROUPS:
        assert worst[g] <= ref.K[g], (name, g, worst[g])
    assert worst["norm"] <= 2.0                                  # |quat| = 1 within 2 ulp
    assert worst["grf_world"] <= ref.K["rot_product"] and worst["forces_body"] <= ref.K["rot_product"]
    # none of it passed emptily
    assert accepted_n >= 0.9 * B * T, (accepted_n, B * T)
    assert swing_n >= 200 and landings >= 20, (swing_n, landings)
    if with_push:
        assert active_n >= 100, active_n
