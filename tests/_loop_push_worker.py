"""Worker of test_launch_forms_give_the_same_bytes: runs the closed loop under push windows (qmpc_loop_run_pushes) for a
heterogeneous fleet -- random controllers and plants with a constant disturbance, different commands, two windows per robot (a
lateral shove and a later shove with a torque, overlapping for every fifth robot), every eighth robot pressed down by a 1000 N
window so that it certainly falls, one robot frozen by a NaN window -- and prints a SHA-256 of the outcome records, one of the
final states and traces, and the launch the call took.  The launch form is chosen by the environment (QMPC_LOOP_FUSED=0 per-tick
kernels, =1 persistent kernel), read when the handle is created.
argv: robots ticks horizon stop|nostop"""
import hashlib
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
from conftest import load_pkg  # noqa: E402

pkg = load_pkg()
robots, ticks, horizon, stop = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4] == "stop"
lib = pkg.load_library()
lp = pkg.default_loop_params(lib)
op = pkg.default_outcome_params(lib, stop_when_down=stop)
p = pkg.default_params(horizon, pkg.MODE_CONVERGED, lib)
rng = np.random.default_rng(11)
cmds = np.zeros((robots, 7))
cmds[:, 0] = rng.uniform(-0.4, 0.4, robots); cmds[:, 1] = rng.uniform(-0.15, 0.15, robots)
cmds[:, 2] = rng.uniform(0.26, 0.32, robots); cmds[:, 5] = rng.uniform(-0.4, 0.4, robots)
cmds[:, 6] = (rng.random(robots) < 0.85).astype(float)
stand = cmds.copy(); stand[:, 6] = 0.0
st = pkg.loop_states(stand, lp, height=0.3, yaw=rng.uniform(-3, 3, robots), lib=lib)
ctrl = pkg.random_go1_variants(robots, seed=3, base=p)
ctrl["mu"] = np.maximum(ctrl["mu"], 0.5)          # walking robots: keep the friction cones usable
plant = pkg.random_go1_plants(robots, seed=4, base=p, payload=(-1.0, 3.0), force=(0.0, 15.0))
push = pkg.random_go1_pushes(robots, seed=5, per_robot=2, start=(8, 30), ticks=(2, 12), impulse=(0.5, 4.0), dt=lp.dt)
push["start_tick"][:, 1] += 25.0                  # the second window later ...
push["start_tick"][::5, 1] = push["start_tick"][::5, 0] + 1.0      # ... or on top of the first
push["torque_body"][:, 1, 2] = rng.uniform(-2.0, 2.0, robots)
push["force_world"][7::8, 0] = [0.0, 0.0, -1000.0]                 # these robots fall
push["start_tick"][7::8, 0] = 6.0; push["ticks"][7::8, 0] = 45.0
push["torque_body"][4, 1, 0] = np.nan             # an invalid window: frozen
s = pkg.Solver(p, robots, device=0, lib=lib)
form = s.loop_instances_plan(robots, True, False)
st, oc = s.loop_run_pushes(st, 6, push, lp, ctrl=ctrl, plant=plant, op=op)
st["movement_mode"] = cmds[:, 6]
st, oc, tf, tc = s.loop_run_pushes(st, ticks, push, lp, ctrl=ctrl, plant=plant, op=op, outcomes=oc, trace=True)
s.close()
assert st["status"][4] == pkg.BAD_PARAMS and st["tick"][4] == 0 and oc[4].tobytes() == pkg.loop_outcomes(1, lib).tobytes()
pressed = np.zeros(robots, dtype=bool); pressed[7::8] = True
# (lift <= 4 x 200 N, weight >= 116 N, mass <= 15.84 kg: at least 19.9 m/s^2 downward, 0.15 m of drop within 25 ticks of the window's 45)
assert (oc["down_tick"][pressed] > 6).all() and (oc["down_tick"][pressed] <= 6 + 45).all()
live = oc["down_tick"] < 0
ok = ~pressed; ok[4] = False
assert live[ok].any() and (oc["ticks"][live & ok] == 6 + ticks).all()
if stop:
    assert (st["tick"][~live] == oc["down_tick"][~live]).all() and (st["tick"][live & ok] == 6 + ticks).all()
else:
    assert (st["tick"][ok | pressed] == 6 + ticks).all()
print("FORM", form)
print("OUTCOMES", hashlib.sha256(oc.tobytes()).hexdigest(), "down", int((~live).sum()), "of", robots)
print("SHA", hashlib.sha256(st.tobytes() + tf.tobytes() + tc.tobytes()).hexdigest(),
      "swing-ticks", int((tc[:, ok] == 0).sum()), "statuses", sorted(set(st["status"][ok].astype(int).tolist())))
