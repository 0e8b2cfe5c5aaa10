"""Worker of tests/test_gpu_loop_warm_records.py: the warm-started closed loop with controller AND plant records
(qmpc_set_loop_warm_records) for a heterogeneous fleet -- random controllers and plants, different commands, one frozen robot
per kind of invalid record and one robot with a NaN state -- through qmpc_loop_run_instances, qmpc_loop_run_outcomes and
qmpc_loop_run_pushes with windows that never act.  Prints a SHA-256 of what each call returned and the launch the calls took.
The launch form is chosen by the environment (QMPC_LOOP_FUSED=0 per-tick kernels, =1 persistent kernel).
argv: robots ticks horizon"""
import hashlib
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
from conftest import load_pkg  # noqa: E402

pkg = load_pkg()
robots, ticks, horizon = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
lib = pkg.load_library()
lp = pkg.default_loop_params(lib)
lp.warm_start = 1.0
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
st["quat"][2] = np.nan                               # rejected records every tick (QMPC_NAN_INPUT): it keeps ticking
plant["mass"][4] = 0.0                               # an invalid plant record: frozen
ctrl["r_weights"][5, 3] = -1.0                       # an invalid controller record: frozen
s = pkg.Solver(p, robots, device=0, lib=lib)
assert s.loop_instances_plan(robots, True, True) is None and not s.loop_warm_records()
s.set_loop_warm_records(True)
form = s.loop_instances_plan(robots, True, True)
st = s.loop_run_instances(st, 6, lp, ctrl=ctrl, plant=plant)
st["movement_mode"] = cmds[:, 6]
xi, tf, tc = s.loop_run_instances(st, ticks, lp, ctrl=ctrl, plant=plant, trace=True)
last = pkg.KERNEL_FAMILY[s.query(pkg.QUERY_LAST_KERNEL)]
xo, oc, tfo, tco = s.loop_run_outcomes(st, ticks, lp, ctrl=ctrl, plant=plant, trace=True)
push = pkg.push_params(robots, 2)
push["start_tick"] = 1e9; push["ticks"] = 5.0; push["force_world"] = 50.0      # never acts
xp, ocp, tfp, tcp = s.loop_run_pushes(st, ticks, push, lp, ctrl=ctrl, plant=plant, trace=True)
s.close()
frozen = [4, 5]
assert (xi["status"][frozen] == pkg.BAD_PARAMS).all() and (xi["tick"][frozen] == 0).all()
assert (tf[:, frozen] == 0).all() and (tc[:, frozen] == 0).all()
ok = np.ones(robots, dtype=bool); ok[frozen] = False; ok[2] = False
assert xi["status"][2] == pkg.NAN_INPUT and (xi["tick"][ok] == 6 + ticks).all()
sha = lambda *a: hashlib.sha256(b"".join(np.ascontiguousarray(x).tobytes() for x in a)).hexdigest()      # noqa: E731
print("FORM", form, "LAST", last)
print("SHA_INSTANCES", sha(xi, tf, tc), "swing-ticks", int((tc[:, ok] == 0).sum()), "statuses", sorted(set(xi["status"][ok].astype(int).tolist())),
      "mean-iterations", round(float(oc["iterations_sum"][ok].sum() / oc["ticks"][ok].sum()), 2))
print("SHA_OUTCOME_STATES", sha(xo, tfo, tco))
print("SHA_OUTCOME_RECORDS", sha(oc))
print("SHA_PUSH", sha(xp, ocp, tfp, tcp), "SHA_OUTCOME_ALL", sha(xo, oc, tfo, tco))
