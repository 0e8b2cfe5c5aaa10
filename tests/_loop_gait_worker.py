"""Worker of the forced-launch-form tests of tests/test_gpu_loop_gait.py: runs the closed loop in which every robot walks its own
gait (qmpc_loop_run_gaits) in the launch form the environment chooses (QMPC_LOOP_FUSED=0 per-tick kernels, =1 persistent kernel;
read when the handle is created).
  fleet     the heterogeneous fleet of tests/_loop_sensing_worker.py -- different commands, plants with a constant disturbance,
            two push windows per robot, ground, actuation and sensing records -- with gait records by i mod 7: the identity, then
            the six named gaits at 1.7 / 2.2 / 3.0 Hz; robot 7 frozen by an invalid record (pronk).  6 ticks standing, then
            `ticks` on the commands.  Prints the launch the call took and SHA-256s of records, final states and traces.
  schedule  18 robots, the six gaits x three frequencies, walking from tick 0 from qmpc_loop_state_set_gait, one tick per call:
            after every tick the schedule fields read back must equal, bit for bit, the FSM restated in Python
            (tests/test_loop_gait_cpu.py: Leg) driven by the contact flags of the state before the tick, and every status must be
            OK or MAX_ITER.  Prints the stance sets each gait reached.
argv: fleet|schedule robots ticks horizon quat|convex"""
import hashlib
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
from conftest import load_pkg  # noqa: E402
from test_loop_gait_cpu import FREQS, SCHEDULE, TABLE, Leg  # noqa: E402

pkg = load_pkg()
what, robots, ticks, horizon, convex = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5] == "convex"
lib = pkg.load_library()
lp = pkg.default_loop_params(lib)
p = (pkg.default_convex_params if convex else pkg.default_params)(horizon, pkg.MODE_CONVERGED, lib)


def solver(B):
    s = pkg.Solver(p, B, device=0, lib=lib)
    if convex:
        s.set_convex_records(True)
    return s


def schedule_fleet():
    """(names, frequencies, records, states walking from tick 0) of the six gaits x three frequencies"""
    names = [n for n in TABLE for _ in FREQS]
    freqs = [f for _ in TABLE for f in FREQS]
    B = len(names)
    gait = pkg.gait_params(B, names, gait_freq=freqs)
    cmds = np.tile([0.15, 0.0, 0.30, 0.0, 0.0, 0.1, 1.0], (B, 1))
    st = pkg.loop_states_set_gait(pkg.loop_states(cmds, lp, height=0.3, yaw=np.linspace(-2, 2, B), lib=lib), gait, lib)
    return names, freqs, gait, st


def run_schedule(s, T):
    names, freqs, gait, st = schedule_fleet()
    B = len(names)
    fsm = [[Leg(*(TABLE[names[i]][k][l] for k in range(3))) for l in range(4)] for i in range(B)]
    for i in range(B):      # tick 0 starts from the reset rule
        for l in range(4):
            assert tuple(float(st["leg"][i, l][k]) for k in SCHEDULE) == fsm[i][l].fields(), (i, l)
    sets = {n: set() for n in TABLE}
    x, oc = st, None
    for t in range(T):
        flags = x["foot_pos_world"][:, 2::3] <= lp.contact_height
        x, oc, *_ = s.loop_run_gaits(x, 1, gait, lp=lp, outcomes=oc)
        for i in range(B):
            for l in range(4):
                fsm[i][l].update(freqs[i] * (5.0 / 1000.0), bool(flags[i, l]))
                assert tuple(float(x["leg"][i, l][k]) for k in SCHEDULE) == fsm[i][l].fields(), (t, i, l, names[i], freqs[i])
                assert x["contacts"][i, l] == fsm[i][l].state and x["gait_counter"][i, l] == fsm[i][l].phase
            sets[names[i]].add(tuple(int(c) for c in x["contacts"][i]))
        assert np.isin(x["status"], (pkg.OK, pkg.MAX_ITER)).all(), (t, x["status"].tolist())
    assert (x["tick"] == T).all()
    return sets, x


if what == "schedule":
    s = solver(18)
    form = s.loop_instances_plan(18, False, False)
    sets, x = run_schedule(s, ticks)
    s.close()
    print("FORM", form)
    print("SETS", {n: sorted(v) for n, v in sets.items()})
    print("SHA", hashlib.sha256(x.tobytes()).hexdigest())
    sys.exit(0)

op = pkg.default_outcome_params(lib, stop_when_down=True)
rng = np.random.default_rng(13)
cmds = np.zeros((robots, 7))
cmds[:, 0] = rng.uniform(-0.3, 0.3, robots); cmds[:, 1] = rng.uniform(-0.15, 0.15, robots)
cmds[:, 2] = rng.uniform(0.26, 0.32, robots); cmds[:, 5] = rng.uniform(-0.4, 0.4, robots)
if convex:
    cmds[:, 3:5] = 0.0
cmds[:, 6] = (rng.random(robots) < 0.85).astype(float)
cmds[cmds[:, 6] == 0, :2] = 0.0
cmds[cmds[:, 6] == 0, 5] = 0.0
stand = cmds.copy(); stand[:, 6] = 0.0
st = pkg.loop_states(stand, lp, height=0.3, yaw=rng.uniform(-3, 3, robots), lib=lib)
plant = pkg.random_go1_plants(robots, seed=4, base=p, payload=(-1.0, 3.0), force=(0.0, 10.0))
push = pkg.random_go1_pushes(robots, seed=5, per_robot=2, start=(8, 30), ticks=(2, 12), impulse=(0.5, 3.0), dt=lp.dt)
ground = pkg.ground_params(robots)
cls = np.arange(robots) % 4
ground["mu"][cls == 0] = 0.5 * p.mu
ground["fz_max"][cls == 1] = 45.0
act = pkg.random_go1_actuations(robots, seed=6, delay=(0, 8), tau=(0.004, 0.03), dt=lp.dt)
act["delay_ticks"][np.arange(robots) % 5 == 0], act["alpha"][np.arange(robots) % 5 == 0] = 0.0, 1.0
line = pkg.actuation_lines(robots, pkg.stand_forces_body(p.mass))
sense = pkg.random_go1_senses(robots, seed=7)
sense["bias"][np.arange(robots) % 3 == 0], sense["sigma"][np.arange(robots) % 3 == 0] = 0.0, 0.0
k7 = np.arange(robots) % 7
names = ["trot" if k == 0 else list(TABLE)[k - 1] for k in k7]
gait = pkg.gait_params(robots, names, gait_freq=np.where(k7 == 0, lp.gait_freq, np.array(FREQS)[np.arange(robots) % 3]))
gait["first_stance"][7] = 1.0                     # an invalid record (pronk): frozen
s = solver(robots)
form = s.loop_instances_plan(robots, False, False)
st, oc, ta, li, sn = s.loop_run_gaits(st, 6, gait, sense, None, act, line, ground, push, lp, plant=plant, op=op)
st["movement_mode"] = cmds[:, 6]
st, oc, ta, li, sn, tf, tc = s.loop_run_gaits(st, ticks, gait, sense, sn, act, li, ground, push, lp, plant=plant, op=op, outcomes=oc, tallies=ta,
                                              trace=True)
s.close()
assert st["status"][7] == pkg.BAD_PARAMS and st["tick"][7] == 0 and oc[7].tobytes() == pkg.loop_outcomes(1, lib).tobytes()
ok = np.ones(robots, dtype=bool); ok[7] = False
assert (st["tick"][ok & (oc["down_tick"] < 0)] == 6 + ticks).all()
print("FORM", form)
print("OUTCOMES", hashlib.sha256(oc.tobytes() + ta.tobytes() + li.tobytes() + sn.tobytes()).hexdigest(), "down", int((oc["down_tick"] >= 0).sum()),
      "of", robots, "clipped ticks", int(ta["clipped_ticks"].sum()))
print("SHA", hashlib.sha256(st.tobytes() + tf.tobytes() + tc.tobytes()).hexdigest(), "statuses", sorted(set(st["status"][ok].astype(int).tolist())))
