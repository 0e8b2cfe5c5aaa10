"""Worker of tests/test_gpu_convex_records.py: the closed loops with per-robot records on a ConvexMpc handle
(qmpc_set_convex_records) under a launch form chosen by the environment (QMPC_LOOP_FUSED=0 per-tick kernels, =1 persistent
kernel; read once per process, at qmpc_create).
argv: uniform robots ticks horizon[,horizon...]
          uniform controller + plant records through qmpc_loop_run_instances against qmpc_loop_run on the same handle: asserts
          that states, force trace and contact trace are the same bytes, prints the launch each horizon took
      random robots ticks horizon
          a heterogeneous fleet -- random controllers, random plants with disturbance wrenches, different commands, one frozen
          robot per kind of invalid record, push windows of which one fells its robot, stop_when_down -- through
          qmpc_loop_run_pushes: prints a SHA-256 of the final states, the traces and the outcome records, and the launch
      idle robots ticks horizon
          PLANT records only, so the tick's solve is the plain ConvexMpc tick of the size (under QMPC_LOOP_FUSED=0: the wrench
          form, the round-1 kernel beyond one resident round of the workspace form, the lane kernel under QMPC_VARIANT=4): one
          robot with an invalid plant record and one felled under stop_when_down.  Their records reach the solve with a NaN
          first word, which those kernels must reject before their first iteration.  Asserts what freezing and halting mean;
          prints the launch, the family of the last solve and how the other robots compare with the run on valid records."""
import hashlib
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
from conftest import load_pkg  # noqa: E402

pkg = load_pkg()
what, robots, ticks = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
lib = pkg.load_library()
lp = pkg.default_loop_params(lib)


def fleet(seed):
    """the commands of the ConvexMpc loop tests (tests/test_gpu_lane.py): no roll / pitch rate command"""
    rng = np.random.default_rng(seed)
    cmds = np.zeros((robots, 7))
    cmds[:, 0] = 0.6 * rng.uniform(-0.5, 0.5, robots); cmds[:, 1] = rng.uniform(-0.2, 0.2, robots)
    cmds[:, 2] = rng.uniform(0.26, 0.32, robots); cmds[:, 5] = rng.uniform(-0.5, 0.5, robots)
    cmds[:, 6] = (rng.random(robots) < 0.9).astype(float)
    cmds[cmds[:, 6] == 0, :2] = 0.0
    cmds[cmds[:, 6] == 0, 5] = 0.0
    stand = cmds.copy(); stand[:, 6] = 0.0
    return cmds, pkg.loop_states(stand, lp, height=0.3, yaw=rng.uniform(-3, 3, robots), lib=lib)


if what == "uniform":
    for horizon in (int(h) for h in sys.argv[4].split(",")):
        p = pkg.default_convex_params(horizon, pkg.MODE_CONVERGED, lib)
        cmds, st0 = fleet(29)
        s = pkg.Solver(p, robots, device=0, lib=lib)
        s.set_convex_records(True)
        form = s.loop_instances_plan(robots, True, False)
        ctrl, plant = pkg.instance_params(p, robots), pkg.plant_params(p, robots)
        a = s.loop_run(st0, 6, lp)
        b = s.loop_run_instances(st0, 6, lp, ctrl=ctrl, plant=plant)
        assert a.tobytes() == b.tobytes()
        a["movement_mode"] = b["movement_mode"] = cmds[:, 6]
        a, atf, atc = s.loop_run(a, ticks, lp, trace=True)
        b, btf, btc = s.loop_run_instances(b, ticks, lp, ctrl=ctrl, plant=plant, trace=True)
        s.close()
        assert (a["tick"] == 6 + ticks).all() and (a["status"] == 0).mean() > 0.95 and (atc == 0).any() and (atf != 0).any()
        assert a.tobytes() == b.tobytes() and atf.tobytes() == btf.tobytes() and atc.tobytes() == btc.tobytes(), horizon
        print("UNIFORM", horizon, form)
elif what == "idle":
    horizon = int(sys.argv[4])
    p = pkg.default_convex_params(horizon, pkg.MODE_CONVERGED, lib)
    cmds, st = fleet(17)
    st["movement_mode"] = cmds[:, 6]
    plant = pkg.random_go1_plants(robots, seed=8, base=p)
    bad = plant.copy()
    bad["mass"][4] = 0.0                                 # an invalid plant record: frozen
    push = pkg.push_params(robots)
    push["ticks"][7], push["force_world"][7, 0] = 60.0, [0.0, 0.0, -2500.0]      # falls from tick 0: down within 7 .. 11 ticks
    op = pkg.default_outcome_params(lib, stop_when_down=True)
    s = pkg.Solver(p, robots, device=0, lib=lib)
    s.set_convex_records(True)
    form = s.loop_instances_plan(robots, False, False)
    want = s.loop_run_pushes(st, ticks, push, lp, plant=plant, op=op, trace=True)
    x, oc, tf, tc = s.loop_run_pushes(st, ticks, push, lp, plant=bad, op=op, trace=True)
    family = pkg.KERNEL_FAMILY[s.query(pkg.QUERY_LAST_KERNEL)]
    s.close()
    # frozen: the state untouched but for status and iterations, zero trace rows, the outcome record untouched
    assert x["status"][4] == pkg.BAD_PARAMS and x["iterations"][4] == 0 and x["tick"][4] == 0
    for n in pkg.LOOP_STATE_DTYPE.names:
        if n not in ("status", "iterations"):
            assert x[n][4].tobytes() == st[n][4].tobytes(), n
    assert (tf[:, 4] == 0).all() and (tc[:, 4] == 0).all() and oc[4].tobytes() == pkg.loop_outcomes(robots, lib)[4].tobytes()
    # halted: the robot stays at its down tick, its trace rows are zero from there on, its solves after it never iterated
    k = int(oc["down_tick"][7])
    assert 7 <= k <= 11 and k < ticks and x["tick"][7] == k and oc["ticks"][7] == k, k
    assert (tf[k:, 7] == 0).all() and (tc[k:, 7] == 0).all() and (tf[:k, 7] != 0).any()
    rest = np.ones(robots, dtype=bool); rest[4] = False
    assert (x["tick"][rest & (oc["down_tick"] < 0)] == ticks).all() and (x["status"][rest] == want[0]["status"][rest]).all()
    same = (x[rest].tobytes() == want[0][rest].tobytes() and oc[rest].tobytes() == want[1][rest].tobytes() and
            tf[:, rest].tobytes() == want[2][:, rest].tobytes() and tc[:, rest].tobytes() == want[3][:, rest].tobytes())
    dp = float(np.abs(x["pos_world"][rest] - want[0]["pos_world"][rest]).max())
    print("IDLE", form, family, "others the same bytes:", same, f"max position difference {dp:.2e} m")
else:
    horizon = int(sys.argv[4])
    p = pkg.default_convex_params(horizon, pkg.MODE_CONVERGED, lib)
    cmds, st = fleet(11)
    ctrl = pkg.random_go1_convex_variants(robots, seed=3, base=p)
    ctrl["mu"] = np.maximum(ctrl["mu"], 0.5)          # walking robots: keep the friction cones usable
    plant = pkg.random_go1_plants(robots, seed=4, base=p, payload=(-1.0, 3.0), force=(0.0, 15.0))
    plant["ext_torque_body"][:, 2] = np.linspace(-0.5, 0.5, robots)
    plant["mass"][4] = 0.0                               # an invalid plant record: frozen
    ctrl["r_weights"][5, 3] = -1.0                       # an invalid controller record: frozen
    push = pkg.push_params(robots, 2)
    push["start_tick"][:, 0], push["ticks"][:, 0] = 8.0, 3.0
    push["force_world"][:, 0, 1] = np.linspace(-40.0, 40.0, robots)
    push["start_tick"][7, 1], push["ticks"][7, 1], push["force_world"][7, 1] = 10.0, 60.0, [0.0, 0.0, -2500.0]      # this one falls
    op = pkg.default_outcome_params(lib, stop_when_down=True)
    s = pkg.Solver(p, robots, device=0, lib=lib)
    s.set_convex_records(True)
    form = s.loop_instances_plan(robots, True, False)
    st, oc = s.loop_run_pushes(st, 6, push, lp, ctrl=ctrl, plant=plant, op=op)
    st["movement_mode"] = cmds[:, 6]
    st, oc, tf, tc = s.loop_run_pushes(st, ticks, push, lp, ctrl=ctrl, plant=plant, op=op, outcomes=oc, trace=True)
    s.close()
    frozen = [4, 5]
    assert (st["status"][frozen] == pkg.BAD_PARAMS).all() and (st["tick"][frozen] == 0).all()
    assert (tf[:, frozen] == 0).all() and (tc[:, frozen] == 0).all() and (oc["ticks"][frozen] == 0).all()
    ok = np.ones(robots, dtype=bool); ok[frozen] = False; ok[7] = False
    assert 10 < oc["down_tick"][7] < 6 + ticks and st["tick"][7] == oc["down_tick"][7]
    up = ok & (oc["down_tick"] < 0)
    assert up.sum() >= 0.8 * robots and (st["tick"][up] == 6 + ticks).all()
    print("FORM", form)
    print("SHA", hashlib.sha256(st.tobytes() + tf.tobytes() + tc.tobytes() + oc.tobytes()).hexdigest(),
          "swing-ticks", int((tc[:, ok] == 0).sum()), "statuses", sorted(set(st["status"][ok].astype(int).tolist())),
          "down", int(oc["down_tick"][7]))
