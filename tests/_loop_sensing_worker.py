"""Worker of test_launch_forms_give_the_same_bytes (tests/test_gpu_loop_sensing.py): runs the closed loop whose controllers read a
measured state (qmpc_loop_run_sensing) for the heterogeneous fleet of tests/_loop_actuation_worker.py -- different commands, plants
with a constant disturbance, two push windows per robot, ground records by i mod 4, actuation records by i mod 5 -- with sensing
records by i mod 3: the identity, a bias on all four channel groups, a random record with noise on all twelve channels; one robot
frozen by an invalid sensing record -- and prints a SHA-256 of the outcome records, tallies, lines and seen records, one of the
final states and traces, and the launch the call took.  The launch form is chosen by the environment (QMPC_LOOP_FUSED=0 per-tick
kernels, =1 persistent kernel), read when the handle is created.
argv: robots ticks horizon stop|nostop quat|convex"""
import hashlib
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
from conftest import load_pkg  # noqa: E402

pkg = load_pkg()
robots, ticks, horizon, stop, convex = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4] == "stop", sys.argv[5] == "convex"
lib = pkg.load_library()
lp = pkg.default_loop_params(lib)
op = pkg.default_outcome_params(lib, stop_when_down=stop)
p = (pkg.default_convex_params if convex else pkg.default_params)(horizon, pkg.MODE_CONVERGED, lib)
rng = np.random.default_rng(13)
cmds = np.zeros((robots, 7))
cmds[:, 0] = rng.uniform(-0.3, 0.3, robots); cmds[:, 1] = rng.uniform(-0.15, 0.15, robots)
cmds[:, 2] = rng.uniform(0.26, 0.32, robots); cmds[:, 5] = rng.uniform(-0.4, 0.4, robots)
cmds[:, 6] = (rng.random(robots) < 0.85).astype(float)
cmds[cmds[:, 6] == 0, :2] = 0.0
cmds[cmds[:, 6] == 0, 5] = 0.0
stand = cmds.copy(); stand[:, 6] = 0.0
st = pkg.loop_states(stand, lp, height=0.3, yaw=rng.uniform(-3, 3, robots), lib=lib)
plant = pkg.random_go1_plants(robots, seed=4, base=p, payload=(-1.0, 3.0), force=(0.0, 10.0))
push = pkg.random_go1_pushes(robots, seed=5, per_robot=2, start=(8, 30), ticks=(2, 12), impulse=(0.5, 3.0), dt=lp.dt)
push["start_tick"][:, 1] += 25.0
ground = pkg.ground_params(robots)
cls = np.arange(robots) % 4
ground["mu"][cls == 0] = 0.5 * p.mu
ground["fz_max"][cls == 1] = 45.0
kind = np.arange(robots) % 5
act = pkg.random_go1_actuations(robots, seed=6, delay=(0, 8), tau=(0.004, 0.03), dt=lp.dt)
act["delay_ticks"][kind == 0], act["alpha"][kind == 0] = 0.0, 1.0
act["delay_ticks"][kind == 2] = 0.0
line = pkg.actuation_lines(robots, pkg.stand_forces_body(p.mass))
sense = pkg.random_go1_senses(robots, seed=7)
k3 = np.arange(robots) % 3
sense["bias"][k3 == 0], sense["sigma"][k3 == 0] = 0.0, 0.0
sense["sigma"][k3 == 1] = 0.0
sense["bias"][k3 == 1] = np.array([0.01, -0.02, 0.005, 0.02, -0.03, 0.04, 0.05, -0.02, 0.01, 0.02, 0.01, -0.03])
sense["sigma"][7, 2] = -1.0                       # an invalid record: frozen
seen0 = pkg.sense_seen(robots)
s = pkg.Solver(p, robots, device=0, lib=lib)
if convex:
    s.set_convex_records(True)
form = s.loop_instances_plan(robots, False, False)
st, oc, ta, li, sn = s.loop_run_sensing(st, 6, sense, seen0, act, line, ground, push, lp, plant=plant, op=op)
st["movement_mode"] = cmds[:, 6]
st, oc, ta, li, sn, tf, tc = s.loop_run_sensing(st, ticks, sense, sn, act, li, ground, push, lp, plant=plant, op=op, outcomes=oc, tallies=ta,
                                                trace=True)
s.close()
assert st["status"][7] == pkg.BAD_PARAMS and st["tick"][7] == 0 and oc[7].tobytes() == pkg.loop_outcomes(1, lib).tobytes()
assert ta[7].tobytes() == pkg.ground_tallies(1).tobytes() and li[7].tobytes() == line[7].tobytes() and sn[7].tobytes() == seen0[7].tobytes()
ok = np.ones(robots, dtype=bool); ok[7] = False
assert (sn["ticks"][ok & (k3 != 0)] == st["tick"][ok & (k3 != 0)]).all() and (sn["ticks"][k3 == 0] == 0).all()
print("FORM", form)
print("OUTCOMES", hashlib.sha256(oc.tobytes() + ta.tobytes() + li.tobytes() + sn.tobytes()).hexdigest(), "down", int((oc["down_tick"] >= 0).sum()),
      "of", robots, "clipped ticks", int(ta["clipped_ticks"].sum()), "measurements", int(sn["ticks"].sum()))
print("SHA", hashlib.sha256(st.tobytes() + tf.tobytes() + tc.tobytes()).hexdigest(), "statuses", sorted(set(st["status"][ok].astype(int).tolist())))
