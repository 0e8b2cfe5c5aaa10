"""Worker of tests/test_gpu_convex_warm_records.py: the warm-started closed loop with controller AND plant records on a ConvexMpc
handle (qmpc_set_convex_records + qmpc_set_convex_warm_records) for a heterogeneous fleet -- random controllers, plants with
disturbance wrenches, different commands, push windows that act, stop_when_down with robots that go down, one frozen robot per
kind of invalid record and one robot with a NaN state -- through qmpc_loop_run_instances, qmpc_loop_run_outcomes and
qmpc_loop_run_pushes.  Prints a SHA-256 of what each call returned and the launch the calls took.  The launch form is chosen by
the environment (QMPC_LOOP_FUSED=0 per-tick kernels, =1 persistent kernel).
argv: robots ticks horizon"""
import hashlib
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
from conftest import load_pkg  # noqa: E402

pkg = load_pkg()
robots, ticks, horizon = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
T0 = 6
lib = pkg.load_library()
lp = pkg.default_loop_params(lib)
lp.warm_start = 1.0
p = pkg.default_convex_params(horizon, pkg.MODE_CONVERGED, lib)
p.ipm_mu0 = 1e-6
rng = np.random.default_rng(11)
cmds = np.zeros((robots, 7))      # (no roll / pitch rate command: the commands of the ConvexMpc loop tests)
cmds[:, 0] = rng.uniform(-0.3, 0.3, robots); cmds[:, 1] = rng.uniform(-0.15, 0.15, robots)
cmds[:, 2] = rng.uniform(0.26, 0.32, robots); cmds[:, 5] = rng.uniform(-0.4, 0.4, robots)
cmds[:, 6] = (rng.random(robots) < 0.85).astype(float)
cmds[cmds[:, 6] == 0, :2] = 0.0
cmds[cmds[:, 6] == 0, 5] = 0.0
stand = cmds.copy(); stand[:, 6] = 0.0
st = pkg.loop_states(stand, lp, height=0.3, yaw=rng.uniform(-3, 3, robots), lib=lib)
ctrl = pkg.random_go1_convex_variants(robots, seed=3, base=p)
ctrl["mu"] = np.maximum(ctrl["mu"], 0.5)          # walking robots: keep the friction cones usable
plant = pkg.random_go1_plants(robots, seed=4, base=p, payload=(-1.0, 3.0), force=(0.0, 15.0))
st["pos_world"][2, 0] = np.nan                       # rejected records every tick (QMPC_NAN_INPUT): it keeps ticking
plant["mass"][4] = 0.0                               # an invalid plant record: frozen
ctrl["r_weights"][5, 3] = -1.0                       # an invalid controller record: frozen
falls = np.arange(robots) % 16 == 7
push = pkg.push_params(robots, 2)
push["start_tick"][:, 0], push["ticks"][:, 0] = T0 + 8.0, 3.0
push["force_world"][:, 0, 1] = np.linspace(-40.0, 40.0, robots)
push["start_tick"][falls, 1], push["ticks"][falls, 1], push["force_world"][falls, 1] = T0 + 2.0, 60.0, [0.0, 0.0, -2500.0]
op = pkg.default_outcome_params(lib, stop_when_down=True)
s = pkg.Solver(p, robots, device=0, lib=lib)
s.set_convex_records(True)
assert s.loop_instances_plan(robots, True, True) is None and not s.convex_warm_records()
s.set_convex_warm_records(True)
form = s.loop_instances_plan(robots, True, True)
st = s.loop_run_instances(st, T0, lp, ctrl=ctrl, plant=plant)
st["movement_mode"] = cmds[:, 6]
xi, tf, tc = s.loop_run_instances(st, ticks, lp, ctrl=ctrl, plant=plant, trace=True)
last = pkg.KERNEL_FAMILY[s.query(pkg.QUERY_LAST_KERNEL)]
xo, oc, tfo, tco = s.loop_run_outcomes(st, ticks, lp, ctrl=ctrl, plant=plant, trace=True)
xp, ocp, tfp, tcp = s.loop_run_pushes(st, ticks, push, lp, ctrl=ctrl, plant=plant, op=op, trace=True)
s.close()
frozen = [4, 5]
assert (xi["status"][frozen] == pkg.BAD_PARAMS).all() and (xi["tick"][frozen] == 0).all()
assert (tf[:, frozen] == 0).all() and (tc[:, frozen] == 0).all()
ok = np.ones(robots, dtype=bool); ok[frozen] = False; ok[2] = False
assert xi["status"][2] == pkg.NAN_INPUT and (xi["tick"][ok] == T0 + ticks).all()
dt = ocp["down_tick"]
halted = ok & falls & (dt >= 0)
assert halted.any() and (xp["tick"][halted] == dt[halted]).all() and (xp["tick"][halted] < T0 + ticks).all()
sha = lambda *a: hashlib.sha256(b"".join(np.ascontiguousarray(x).tobytes() for x in a)).hexdigest()      # noqa: E731
print("FORM", form, "LAST", last)
print("SHA_INSTANCES", sha(xi, tf, tc), "swing-ticks", int((tc[:, ok] == 0).sum()), "statuses", sorted(set(xi["status"][ok].astype(int).tolist())),
      "mean-iterations", round(float(oc["iterations_sum"][ok].sum() / oc["ticks"][ok].sum()), 2))
print("SHA_OUTCOME_STATES", sha(xo, tfo, tco))
print("SHA_OUTCOME_RECORDS", sha(oc))
print("SHA_PUSH", sha(xp, tfp, tcp), "halted", int(halted.sum()))
print("SHA_PUSH_RECORDS", sha(ocp))
