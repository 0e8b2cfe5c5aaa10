"""Input sets of the attitude-error tests (tests/test_attitude_sets_cpu.py, tests/test_gpu_attitude_sets.py,
tests/golden/make_attitude_fixtures.py): the body up to and beyond pi away from its desired attitude -- where the state generators
keep quat_d within about 0.55 rad of quat, the yaw part of the error second order.  Not a test module.

The cost term is w (1 - |q_ref'q|): it has a sign branch, its attitude Hessian w |q_ref'q| goes to 0 as the error goes to pi and
its gradient w G(q)'q_ref is of order w.  quat, rot, velocities, feet and contacts stay as the generator draws them; only
quat_d is replaced, by normalise(quat (x) axis_angle(axis, +-theta)) with the axis given in the body frame.

The CPU suite and the GPU suite build their records here, so both see the same ones."""
import numpy as np

from stance_sets import copies_identical, plain_plan, swing_rows, tiled  # noqa: F401  (the tests take them from here)

# 3.1: |q_ref'q| = cos(1.55) = 0.021 at knot 0, so rounding cannot choose the branch.  3.5: past pi, q_ref'q < 0 by geometry
# with both quaternions as the generator signs them.  Exactly pi is left out: there the last bit of a dot product decides
# the branch and both answers are valid.
ANGLES = (0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.1, 3.5)
AXES = ("yaw", "body x", "body y", "random")
# the horizons' envelopes (CPU oracle, tests/test_attitude_sets_cpu.py): N = 20 converges on every record up to 1.5 rad (at 2.0
# rad 1 of 96 random-axis records fails, from 2.5 rad on 7 ... 30 %); the 8-point model at N = 16 up to 2.0 rad.
ANGLES_N20 = ANGLES[:3]
ANGLES_BIPED8 = ANGLES[:4]
# 8-point model, N = 16: the angles up to which the sets are held to the oracle's iteration counts; 2.0 rad is a set of its own
# (tests/test_attitude_sets_cpu.py::test_lane_core_matches_oracle_on_every_attitude_set has the cause and the measured shares)
ANGLES_BIPED8_COUNTS = ANGLES[:3]
# the warm start from the closed loop's low initial barrier (ipm_mu0 = 1e-6) converges with room up to here: at 3.0 rad it
# takes up to 89 and at 3.1 rad all 120 iterations of the cap (CPU oracle)
WARM_LOW_BARRIER_MAX = 2.5
_SEED = 0xA771


def cell(k, angles=ANGLES):
    """(angle, axis kind, sense) of record k: from k alone.  The sense alternates, the axis kind changes every second and the
    angle every eighth record, so the first 8 len(angles) records hold one of every cell and every whole multiple as many of each."""
    k = np.asarray(k)
    return np.asarray(angles)[(k // 8) % len(angles)], (k // 2) % 4, 1.0 - 2.0 * (k % 2)


def _axes(kind):
    """unit axes in the body frame; the random ones from a fixed seed, axis k the same whatever the size of the set"""
    n = len(kind)
    ax = np.random.default_rng(_SEED).standard_normal((4096, 3))[:n]
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    for j, e in enumerate(((0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0))):
        ax[kind == j] = e
    return ax


def _quat_mul(a, b):
    aw, ax, ay, az = (a[..., i] for i in range(4))
    bw, bx, by, bz = (b[..., i] for i in range(4))
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], axis=-1)


def with_error(rec, angles, shift=0):
    """A copy of rec with quat_d = normalise(quat (x) axis_angle(axis_k, sense_k angle_k)); `shift` moves every record to the
    neighbouring angle of the grid (the last one down, the others up)"""
    rec = rec.copy()
    k = np.arange(len(rec))
    ang, kind, sense = cell(k, angles)
    if shift:
        i = (k // 8) % len(angles)
        ang = np.asarray(angles)[np.where(i + 1 < len(angles), i + 1, i - 1)]
    h = 0.5 * sense * ang
    dq = np.concatenate([np.cos(h)[:, None], np.sin(h)[:, None] * _axes(kind)], axis=1)
    qd = _quat_mul(rec["quat"], dq)
    rec["quat_d"] = qd / np.linalg.norm(qd, axis=1, keepdims=True)
    return rec


def error_angle(rec):
    """[B] angle in [0, 2 pi) of the rotation quat^-1 (x) quat_d as the two quaternions are signed (beyond pi: quat'quat_d < 0)"""
    q = rec["quat"] * np.array([1.0, -1.0, -1.0, -1.0])
    d = _quat_mul(q / (rec["quat"] ** 2).sum(axis=1, keepdims=True), rec["quat_d"])
    return 2.0 * np.arctan2(np.linalg.norm(d[:, 1:], axis=1), d[:, 0])


def grid_angle(rec, angles=ANGLES):
    """[B] the grid angle nearest to error_angle(rec): what the tests group and print by"""
    a = np.asarray(angles)
    return a[np.abs(error_angle(rec)[:, None] - a[None, :]).argmin(axis=1)]


def quat(pkg, N):
    """QuatMpc records: N = 5, 10: 384, six of every (angle, axis, sense) cell of all eight angles.  N = 20: 192, eight of every
    cell up to 1.5 rad."""
    if N == 20:
        return with_error(pkg.random_go1_trot_states(192, config_id=3), ANGLES_N20)
    return with_error(pkg.random_go1_trot_states(384, config_id=2), ANGLES)


def biped8(pkg, N=16, far=False):
    """Records of the 8-point model: 192, eight of every cell up to 1.5 rad.  far=True: the second set, 96 records at 2.0 rad
    (twelve of every cell), on which the final steps of the solver sit on its step tolerance: held to status, forces and swing
    forces, the share of equal iteration counts printed only."""
    if far:
        return with_error(pkg.random_biped8_states(96, config_id=5), ANGLES_BIPED8[3:])
    return with_error(pkg.random_biped8_states(192, config_id=5), ANGLES_BIPED8_COUNTS)


def variants(pkg, p):
    """Per-instance records for quat(pkg, 10): a robot of its own per instance (pkg.random_go1_variants around `p`: mass,
    inertia, friction, force bound, Q and R) and the attitude weight w -- the factor of the cost term these sets are about,
    which random_go1_variants leaves alone -- scaled by U(0.5, 1.25).  The upper end is the reference's: with U(0.5, 2) the CPU
    oracle alone ends one record at 3.5 rad NOT_PD and needs 63 iterations on one at 3.0 rad, with U(0.5, 1.5) the NOT_PD record
    remains; with U(0.5, 1.25) it converges on every record in at most 45 (tests/test_attitude_sets_cpu.py holds that)."""
    ip = pkg.random_go1_variants(384, seed=19, base=p)
    ip["w"] *= 0.5 + 0.75 * np.random.default_rng(19).uniform(0.0, 1.0, 384)
    return ip


# the robots of the closed-loop test: (axis kind, error angle); two stay where their reference is
LOOP_ERRORS = (("yaw", 1.0), ("yaw", 2.0), ("yaw", 3.0), ("yaw", 3.5), ("random", 1.0), ("random", 2.0), (None, 0.0), (None, 0.0))
LOOP_YAWS = (0.0, 0.4, -1.0, 2.0, 0.7, -0.3, 0.0, 1.3)


def loop_states(pkg, lib, lp):
    """Eight standing robots of the device closed loop (pkg.loop_states, stand mode, 0.3 m) whose bodies start LOOP_ERRORS away
    from the attitude reference quat_d the loop carries as state.  Yaw errors: the robot stands turned by the angle, feet with
    it (they follow the body's yaw), and quat_d is the unturned attitude; past pi quat'quat_d < 0 as the two are signed.
    Random-axis errors: the body is turned about a random body axis over feet that stay where they stand on the ground."""
    cmds = [[0.0, 0.0, 0.30, 0.0, 0.0, 0.0, 0.0]] * len(LOOP_ERRORS)
    ref = pkg.loop_states(cmds, lp, height=0.3, yaw=LOOP_YAWS, lib=lib)
    st = pkg.loop_states(cmds, lp, height=0.3, lib=lib,
                         yaw=[y + (a if kind == "yaw" else 0.0) for y, (kind, a) in zip(LOOP_YAWS, LOOP_ERRORS)])
    st["quat_d"] = ref["quat"]
    axes = _axes(np.full(len(LOOP_ERRORS), 3))
    for i, (kind, a) in enumerate(LOOP_ERRORS):
        if kind == "random":
            q = _quat_mul(ref["quat"][i], np.concatenate([[np.cos(0.5 * a)], np.sin(0.5 * a) * axes[i]]))
            st["quat"][i] = q / np.linalg.norm(q)
    return st


def attitude_distance(rec):
    """[B] angle in [0, pi] between the attitudes quat and quat_d, whatever their signs"""
    return 2.0 * np.arccos(np.minimum(1.0, np.abs((rec["quat"] * rec["quat_d"]).sum(axis=-1))))


def warm_pairs(pkg, N, angle_max=None):
    """(first tick, second tick) of a warm start: the first tick is quat(pkg, N); the second has lin_vel_body + 0.02, quat_d at
    the neighbouring angle of the grid (the next one up; from the last one down), and on every third record the stance set
    mirrored left to right (FL <-> FR, RL <-> RR: the trot diagonals change places, so two legs land and two lift off).
    angle_max: only the records whose two ticks both stay at or below it."""
    grid = ANGLES_N20 if N == 20 else ANGLES
    base = pkg.random_go1_trot_states(192 if N == 20 else 384, config_id=3 if N == 20 else 2)
    first, second = with_error(base, grid), with_error(base, grid, shift=1)
    second["lin_vel_body"] += 0.02
    second["contacts"][::3] = second["contacts"][::3][:, [1, 0, 3, 2]]
    if angle_max is not None:
        keep = np.maximum(grid_angle(first), grid_angle(second)) <= angle_max
        first, second = first[keep], second[keep]
    return first, second
