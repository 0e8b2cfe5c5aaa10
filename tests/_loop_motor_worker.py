"""Worker of the forced-launch-form test of tests/test_gpu_loop_motor.py: the motor rule of qmpc_loop_run_motors checked tick by
tick, without the host class, in the launch form the environment chooses (QMPC_LOOP_FUSED=0 per-tick kernels, =1 persistent
kernel; read when the handle is created).
  rule   `robots` walking robots with mixed gaits (walking from tick 0 from qmpc_loop_state_set_gait) and a shove each.  An
         unlimited run of `ticks` ticks gives every robot's peak torque per joint type; the limits are 0.6 x those.  Then one tick
         per call: after every tick, from the state the call received and the tally it returned, with the Jacobians of the
         library's own qmpc_leg_kinematics at the returned joint_pos --
           forward kinematics of joint_pos equals R'(foot - p) to 1e-4 m (the inverse kinematics carries a single-precision atan2);
           the sat_ticks increments are the joints of stance legs whose |-(J'c)_j| exceeds the limit, c the tick's forces_body;
           every clipped stance leg has grf_world = R u' to 1e-9 relative, u' solved in numpy from J'u' = -t;
           peak_tau is updated by exactly the demanded maxima, to 1e-9 relative; clipped_ticks and first_clipped_tick follow;
           against the gaits call for one tick on the same input: a robot with no clipped leg has its bytes in full, a robot with
           one has its grf_world bytes on the unclipped legs;
           every status is OK or MAX_ITER.
         At the end: at least 90 % of the robots have clipped_ticks > 0 and unreachable_leg_ticks is 0 everywhere.
         Prints the launch form, the worst figures and a SHA-256 of final states and tallies.
argv: rule robots ticks horizon quat|convex"""
import hashlib
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
from conftest import load_pkg  # noqa: E402
from test_loop_gait_cpu import FREQS, TABLE  # noqa: E402

pkg = load_pkg()
what, robots, ticks, horizon, convex = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5] == "convex"
assert what == "rule"
lib = pkg.load_library()
lp = pkg.default_loop_params(lib)
p = (pkg.default_convex_params if convex else pkg.default_params)(horizon, pkg.MODE_CONVERGED, lib)
B, T = robots, ticks


def rot(quat):
    """quat_to_rot of csrc/qmpc_loop_math.h, [B, 3, 3] row-major body -> world"""
    w, x, y, z = (quat[:, i] for i in range(4))
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.stack([np.stack([1.0 - (tyy + tzz), txy - twz, txz + twy], -1),
                     np.stack([txy + twz, 1.0 - (txx + tzz), tyz - twx], -1),
                     np.stack([txz - twy, tyz + twx, 1.0 - (txx + tyy)], -1)], -2)


rng = np.random.default_rng(21)
cmds = np.zeros((B, 7))
cmds[:, 0] = rng.uniform(0.1, 0.3, B); cmds[:, 1] = rng.uniform(-0.1, 0.1, B)
cmds[:, 2] = rng.uniform(0.27, 0.31, B); cmds[:, 5] = rng.uniform(-0.3, 0.3, B)
cmds[:, 6] = 1.0
k7 = np.arange(B) % 7
names = ["trot" if k == 0 else list(TABLE)[k - 1] for k in k7]
gait = pkg.gait_params(B, names, gait_freq=np.where(k7 == 0, lp.gait_freq, np.array(FREQS)[np.arange(B) % 3]))
st0 = pkg.loop_states_set_gait(pkg.loop_states(cmds, lp, height=0.3, yaw=rng.uniform(-3, 3, B), lib=lib), gait, lib)
push = pkg.push_params(B, 1)
ang = rng.uniform(0, 2 * np.pi, B)
for i in range(B):      # a shove of 40 N for 6 ticks, from tick 10 on, in a random horizontal direction
    push[i, 0] = (10.0, 6.0, [40.0 * np.cos(ang[i]), 40.0 * np.sin(ang[i]), 0.0], [0.0, 0.0, 0.0])
s = pkg.Solver(p, B, device=0, lib=lib)
if convex:
    s.set_convex_records(True)
geom = s.default_go1_geometry()
form = s.loop_instances_plan(B, False, False)

free = s.loop_run_motors(st0, T, pkg.motor_params(B), gait=gait, push=push, lp=lp)
pk = free[5]["peak_tau"].reshape(B, 4, 3).max(axis=1)      # per robot and joint type
assert (pk > 0).all() and (free[5]["sat_ticks"] == 0).all() and (free[5]["clipped_ticks"] == 0).all()
motor = pkg.motor_params(B, np.tile(0.6 * pk, (1, 4)))
tmax = motor["tau_max"].reshape(B, 4, 3)

x, oc, mt = st0, None, pkg.motor_tallies(B, lib)
worst = {"fk": 0.0, "grf": 0.0, "peak": 0.0}
clipped_legs = 0
for t in range(T):
    got = s.loop_run_motors(x, 1, motor, mt, gait=gait, push=push, lp=lp, outcomes=oc)
    ref = s.loop_run_gaits(x, 1, gait, push=push, lp=lp, outcomes=oc)
    nx, noc, nmt = got[0], got[1], got[5]
    assert np.isin(nx["status"], (pkg.OK, pkg.MAX_ITER)).all(), (t, nx["status"].tolist())
    R = rot(x["quat"])
    fkp, J = s.leg_kinematics(geom, nmt["joint_pos"])
    J = J.reshape(B, 4, 3, 3)      # J[b, l, j, i] = d p_i / d q_j (column-major)
    d = x["foot_pos_world"].reshape(B, 4, 3) - x["pos_world"][:, None, :]
    pb = np.einsum("bki,blk->bli", R, d)      # R'(foot - p)
    worst["fk"] = max(worst["fk"], float(np.abs(fkp.reshape(B, 4, 3) - pb).max()))
    c = nx["forces_body"].reshape(B, 4, 3)
    stance = nx["contacts"] != 0
    tau = -np.einsum("blji,bli->blj", J, c)
    bind = stance[:, :, None] & (np.abs(tau) > tmax)
    assert np.array_equal(nmt["sat_ticks"] - mt["sat_ticks"], bind.reshape(B, 12).astype(float)), t
    clip = bind.any(axis=2)      # (no singular leg: unreachable_leg_ticks stays 0, checked below)
    tt = np.where(bind, np.copysign(tmax, tau), tau)
    grf = nx["grf_world"].reshape(B, 4, 3)
    ref_grf = ref[0]["grf_world"].reshape(B, 4, 3)
    for b, l in zip(*np.nonzero(clip)):
        up = np.linalg.solve(J[b, l], -tt[b, l])      # rows of J[b, l] are the rows of J': (J'u')_j = sum_i J[j, i] u_i
        want = R[b] @ up
        err = float(np.abs(grf[b, l] - want).max() / max(np.abs(want).max(), 1e-300))
        worst["grf"] = max(worst["grf"], err)
        clipped_legs += 1
    dem = np.where(stance[:, :, None], np.abs(tau), 0.0).reshape(B, 12)
    want_pk = np.maximum(mt["peak_tau"], dem)
    worst["peak"] = max(worst["peak"], float((np.abs(nmt["peak_tau"] - want_pk) / np.maximum(want_pk, 1e-300)).max()))
    any_clip = clip.any(axis=1)
    assert np.array_equal(nmt["clipped_ticks"] - mt["clipped_ticks"], any_clip.astype(float)), t
    first = np.where((mt["first_clipped_tick"] < 0) & any_clip, nx["tick"], mt["first_clipped_tick"])
    assert np.array_equal(nmt["first_clipped_tick"], first), t
    for b in range(B):
        if not any_clip[b]:
            assert nx[b].tobytes() == ref[0][b].tobytes() and noc[b].tobytes() == ref[1][b].tobytes(), (t, b)
        else:
            assert grf[b][~clip[b]].tobytes() == ref_grf[b][~clip[b]].tobytes(), (t, b)
            assert nx["forces_body"][b].tobytes() == ref[0]["forces_body"][b].tobytes(), (t, b)      # the command is the command
    x, oc, mt = nx, noc, nmt
s.close()
print("FORM", form)
print("WORST", worst, "clipped legs", clipped_legs, "robots clipped", int((mt["clipped_ticks"] > 0).sum()), "of", B)
assert worst["fk"] <= 1e-4 and worst["grf"] <= 1e-9 and worst["peak"] <= 1e-9, worst
assert (mt["clipped_ticks"] > 0).mean() >= 0.9 and (mt["unreachable_leg_ticks"] == 0).all()
assert (x["tick"] == T).all()
print("SHA", hashlib.sha256(x.tobytes() + mt.tobytes() + oc.tobytes()).hexdigest())
