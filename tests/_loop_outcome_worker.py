"""Worker of test_launch_forms_give_the_same_records: runs the closed loop with outcome records (qmpc_loop_run_outcomes) for a
heterogeneous fleet -- random controllers and plants, different commands, every eighth robot pressed down with 1000 N so that it
certainly falls, one frozen robot per kind of invalid record and one robot with a NaN state -- and prints a SHA-256 of the
outcome records, one of the final states and traces, and the launch the call took.  The launch form is chosen by the
environment (QMPC_LOOP_FUSED=0 per-tick kernels, =1 persistent kernel), read when the handle is created.
argv: robots ticks horizon ctrl|noctrl cold|warm stop|nostop"""
import hashlib
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
from conftest import load_pkg  # noqa: E402

pkg = load_pkg()
robots, ticks, horizon = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
with_ctrl, warm, stop = sys.argv[4] == "ctrl", sys.argv[5] == "warm", sys.argv[6] == "stop"
lib = pkg.load_library()
lp = pkg.default_loop_params(lib)
lp.warm_start = 1.0 if warm else 0.0
op = pkg.default_outcome_params(lib, stop_when_down=stop)
p = pkg.default_params(horizon, pkg.MODE_CONVERGED, lib)
rng = np.random.default_rng(11)
cmds = np.zeros((robots, 7))
cmds[:, 0] = rng.uniform(-0.4, 0.4, robots); cmds[:, 1] = rng.uniform(-0.15, 0.15, robots)
cmds[:, 2] = rng.uniform(0.26, 0.32, robots); cmds[:, 5] = rng.uniform(-0.4, 0.4, robots)
cmds[:, 6] = (rng.random(robots) < 0.85).astype(float)
stand = cmds.copy(); stand[:, 6] = 0.0
st = pkg.loop_states(stand, lp, height=0.3, yaw=rng.uniform(-3, 3, robots), lib=lib)
ctrl = pkg.random_go1_variants(robots, seed=3, base=p) if with_ctrl else None
if ctrl is not None:
    ctrl["mu"] = np.maximum(ctrl["mu"], 0.5)          # walking robots: keep the friction cones usable
plant = pkg.random_go1_plants(robots, seed=4, base=p, payload=(-1.0, 3.0), force=(0.0, 15.0))
plant["ext_force_world"][7::8, 2] = -1000.0          # these robots fall
st["quat"][2] = np.nan                               # rejected records every tick (QMPC_NAN_INPUT); down after its first tick
plant["mass"][4] = 0.0                               # an invalid plant record: frozen
if ctrl is not None:
    ctrl["r_weights"][5, 3] = -1.0                   # an invalid controller record: frozen
s = pkg.Solver(p, robots, device=0, lib=lib)
form = s.loop_instances_plan(robots, ctrl is not None, warm)
st, oc = s.loop_run_outcomes(st, 6, lp, ctrl=ctrl, plant=plant, op=op)
st["movement_mode"] = cmds[:, 6]
st, oc, tf, tc = s.loop_run_outcomes(st, ticks, lp, ctrl=ctrl, plant=plant, op=op, outcomes=oc, trace=True)
s.close()
frozen = [4] + ([5] if ctrl is not None else [])
assert (st["status"][frozen] == pkg.BAD_PARAMS).all() and (st["tick"][frozen] == 0).all()
assert oc[frozen].tobytes() == pkg.loop_outcomes(len(frozen), lib).tobytes()
loaded = np.zeros(robots, dtype=bool); loaded[7::8] = True; loaded[frozen] = False
assert (oc["down_tick"][loaded] > 0).all() and oc["down_tick"][2] == 1
ok = np.ones(robots, dtype=bool); ok[frozen] = False; ok[2] = False; ok[loaded] = False
live = oc["down_tick"] < 0
assert (live[ok]).mean() > 0.9 and (oc["ticks"][live & ok] == 6 + ticks).all()
if stop:
    halted = ~live
    assert (st["tick"][halted] == oc["down_tick"][halted]).all() and (st["tick"][live & ok] == 6 + ticks).all()
else:
    assert (st["tick"][ok | loaded] == 6 + ticks).all()
print("FORM", form)
print("OUTCOMES", hashlib.sha256(oc.tobytes()).hexdigest(), "down", int((~live).sum()), "of", robots)
print("SHA", hashlib.sha256(st.tobytes() + tf.tobytes() + tc.tobytes()).hexdigest(),
      "swing-ticks", int((tc[:, ok] == 0).sum()), "statuses", sorted(set(st["status"][ok].astype(int).tolist())))
