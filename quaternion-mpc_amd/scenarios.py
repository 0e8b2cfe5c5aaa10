"""Synthetic LeggedState records for the quaternion-MPC hot path.

The generator is the one fixed in SURVEY.md section 8(d): a counter-based RNG
(SplitMix64; seed ``0x5EED0000 + config_id``, stream = instance index) so that
the CPU oracle and the GPU see the very same arrays, on any machine, at any
batch size (instance i does not depend on the batch it is drawn in).

Field meaning follows ``struct qmpc_input`` in ``include/qmpc.h`` (which in turn
cites the LeggedState fields read by QuatMpc.cpp:109-276).
"""
from __future__ import annotations

import numpy as np

_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def _mix(z: np.ndarray) -> np.ndarray:
    """SplitMix64 finaliser on a uint64 array (wrap-around arithmetic)."""
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        return z ^ (z >> np.uint64(31))


def _uniform(seed: int, index: np.ndarray, ndraw: int) -> np.ndarray:
    """[len(index), ndraw] doubles in [0,1): draw j of stream i."""
    with np.errstate(over="ignore"):
        key = _mix(np.uint64(seed) + (index.astype(np.uint64) + np.uint64(1)) * _GOLDEN)
        ctr = (np.arange(1, ndraw + 1, dtype=np.uint64) * _GOLDEN)[None, :]
        bits = _mix(key[:, None] + ctr)
    return (bits >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def _normal(u1: np.ndarray, u2: np.ndarray) -> np.ndarray:
    return np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(2.0 * np.pi * u2)


def quat_mul(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    aw, ax, ay, az = (a[..., i] for i in range(4))
    bw, bx, by, bz = (b[..., i] for i in range(4))
    return np.stack(
        [
            aw * bw - ax * bx - ay * by - az * bz,
            aw * bx + ax * bw + ay * bz - az * by,
            aw * by - ax * bz + ay * bw + az * bx,
            aw * bz + ax * by - ay * bx + az * bw,
        ],
        axis=-1,
    )


def quat_to_rot(q: np.ndarray) -> np.ndarray:
    """Body->world rotation matrix of unit quaternion (w,x,y,z); [...,9] row-major
    (what Eigen's toRotationMatrix gives at BaseInterface.cpp:196)."""
    w, x, y, z = (q[..., i] for i in range(4))
    R = np.stack(
        [
            1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
            2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
            2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y),
        ],
        axis=-1,
    )
    return R


def _axis_angle(axis: np.ndarray, ang: np.ndarray) -> np.ndarray:
    h = 0.5 * ang
    return np.concatenate([np.cos(h)[..., None], np.sin(h)[..., None] * axis], axis=-1)


def _input_dtype():
    from . import INPUT_DTYPE

    return INPUT_DTYPE


NOMINAL_FEET = np.array(  # yaml default footholds, gazebo_go1_quat_mpc.yaml:15-33
    [[0.20, 0.14, -0.30], [0.20, -0.14, -0.30], [-0.20, 0.14, -0.30], [-0.20, -0.14, -0.30]]
)


def random_go1_trot_states(batch: int, config_id: int = 2, first: int = 0, tilt_max: float = 0.5,
                           vel_sigma: float = 0.3) -> np.ndarray:
    """`batch` records, instance indices first .. first+batch-1."""
    seed = 0x5EED0000 + int(config_id)
    idx = np.arange(first, first + batch, dtype=np.uint64)
    u = _uniform(seed, idx, 48)
    c = iter(range(48))
    nx = lambda: u[:, next(c)]  # noqa: E731
    rec = np.zeros(batch, dtype=_input_dtype())

    yaw = (2.0 * nx() - 1.0) * np.pi
    tilt_dir = 2.0 * np.pi * nx()
    tilt = tilt_max * nx()
    zaxis = np.zeros((batch, 3)); zaxis[:, 2] = 1.0
    haxis = np.stack([np.cos(tilt_dir), np.sin(tilt_dir), np.zeros(batch)], axis=-1)
    q_yaw = _axis_angle(zaxis, yaw)
    q = quat_mul(q_yaw, _axis_angle(haxis, tilt))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    rec["quat"] = q
    rec["rot"] = quat_to_rot(q)
    rec["lin_vel_body"] = np.stack([vel_sigma * _normal(nx(), nx()) for _ in range(3)], axis=-1)
    rec["ang_vel_body"] = np.stack([0.5 * _normal(nx(), nx()) for _ in range(3)], axis=-1)
    feet = np.tile(NOMINAL_FEET[None], (batch, 1, 1))
    for leg in range(4):
        for ax in range(3):
            feet[:, leg, ax] += 0.1 * nx() - 0.05
    rec["foot_pos_body"] = feet.reshape(batch, 12)  # [3*leg + axis] = Eigen 3x4 col-major
    g = nx()
    contacts = np.ones((batch, 4))
    a = g < 0.4            # FL + RR stance
    b = (g >= 0.4) & (g < 0.8)  # FR + RL stance
    contacts[a] = [1, 0, 0, 1]
    contacts[b] = [0, 1, 1, 0]
    rec["contacts"] = contacts
    rec["pos_ref_body"] = np.stack([0.02 * _normal(nx(), nx()) for _ in range(3)], axis=-1)
    rec["vel_ref_body"] = np.stack([nx() - 0.5, 0.2 * nx() - 0.1, np.zeros(batch)], axis=-1)
    small = np.stack([0.05 * _normal(nx(), nx()) for _ in range(2)] + [np.zeros(batch)], axis=-1)
    ang = np.linalg.norm(small, axis=-1)
    ax_ = np.where(ang[:, None] > 0, small / np.maximum(ang, 1e-300)[:, None], haxis)
    qd = quat_mul(q_yaw, _axis_angle(ax_, ang))
    qd /= np.linalg.norm(qd, axis=-1, keepdims=True)
    rec["quat_d"] = qd
    return rec


def go1_stand_input(feet: np.ndarray | None = None) -> np.ndarray:
    """Single stand-pose record (BASELINE config 0): identity attitude, rest,
    all four feet in contact, references at rest."""
    rec = np.zeros(1, dtype=_input_dtype())
    rec["quat"][0] = [1, 0, 0, 0]
    rec["rot"][0] = np.eye(3).reshape(9)
    f = NOMINAL_FEET if feet is None else np.asarray(feet, dtype=float)
    rec["foot_pos_body"][0] = f.reshape(12)
    rec["contacts"][0] = 1.0
    rec["quat_d"][0] = [1, 0, 0, 0]
    return rec


def random_go1_convex_states(batch: int, config_id: int = 12, first: int = 0, vel_sigma: float = 0.3) -> np.ndarray:
    """`batch` records of ``struct qmpc_convex_input`` (legged::ConvexMpc::grf_update's inputs,
    ConvexMpc.cpp:81-198), same counter-based generator: yaw U(-pi,pi), roll/pitch N(0,0.1^2),
    world-frame velocities N(0, vel_sigma^2) / N(0,0.5^2), footholds = Rz(yaw)(nominal + U(-.05,.05)^3),
    contacts 40/40/20 % as for the quaternion path, yaw-rate command U(-0.5,0.5)."""
    from . import CONVEX_INPUT_DTYPE

    seed = 0x5EED0000 + int(config_id)
    idx = np.arange(first, first + batch, dtype=np.uint64)
    u = _uniform(seed, idx, 48)
    c = iter(range(48))
    nx = lambda: u[:, next(c)]  # noqa: E731
    rec = np.zeros(batch, dtype=CONVEX_INPUT_DTYPE)
    yaw = (2.0 * nx() - 1.0) * np.pi
    roll = 0.1 * _normal(nx(), nx())
    pitch = 0.1 * _normal(nx(), nx())
    rec["euler"] = np.stack([roll, pitch, yaw], axis=-1)
    pos = np.stack([0.05 * _normal(nx(), nx()), 0.05 * _normal(nx(), nx()), 0.3 + 0.02 * _normal(nx(), nx())], axis=-1)
    rec["pos_world"] = pos
    rec["ang_vel_world"] = np.stack([0.5 * _normal(nx(), nx()) for _ in range(3)], axis=-1)
    rec["lin_vel_world"] = np.stack([vel_sigma * _normal(nx(), nx()) for _ in range(3)], axis=-1)
    cy, sy = np.cos(yaw), np.sin(yaw)
    feet = np.tile(NOMINAL_FEET[None], (batch, 1, 1))
    for leg in range(4):
        for ax in range(3):
            feet[:, leg, ax] += 0.1 * nx() - 0.05
    fw = np.empty_like(feet)
    fw[:, :, 0] = cy[:, None] * feet[:, :, 0] - sy[:, None] * feet[:, :, 1]
    fw[:, :, 1] = sy[:, None] * feet[:, :, 0] + cy[:, None] * feet[:, :, 1]
    fw[:, :, 2] = feet[:, :, 2]
    rec["foot_pos_abs_com"] = fw.reshape(batch, 12)
    g = nx()
    contacts = np.ones((batch, 4))
    contacts[g < 0.4] = [1, 0, 0, 1]
    contacts[(g >= 0.4) & (g < 0.8)] = [0, 1, 1, 0]
    rec["contacts"] = contacts
    rec["pos_d_world"] = np.stack([pos[:, 0], pos[:, 1], np.full(batch, 0.3)], axis=-1)
    vx, vy = nx() - 0.5, 0.2 * nx() - 0.1
    rec["lin_vel_d_world"] = np.stack([cy * vx - sy * vy, sy * vx + cy * vy, np.zeros(batch)], axis=-1)
    rec["yaw_rate_d"] = nx() - 0.5
    return rec


def random_biped8_states(batch: int, config_id: int = 5, first: int = 0, tilt_max: float = 0.3,
                         vel_sigma: float = 0.3) -> np.ndarray:
    """`batch` records of ``struct qmpc_input8`` for BASELINE config 5: a SYNTHETIC biped with two
    0.2 x 0.1 m feet, 4 corner contact points each (points 0-3 left foot, 4-7 right foot), hip height
    0.85 m.  The humanoid branch is not in the reference checkout, so this footprint is this
    repository's choice; same counter-based generator as the Go1 states.  Support:
    40 % both feet, 30 % left only, 30 % right only."""
    from . import INPUT8_DTYPE

    seed = 0x5EED0000 + int(config_id)
    idx = np.arange(first, first + batch, dtype=np.uint64)
    u = _uniform(seed, idx, 64)
    c = iter(range(64))
    nx = lambda: u[:, next(c)]  # noqa: E731
    rec = np.zeros(batch, dtype=INPUT8_DTYPE)
    yaw = (2.0 * nx() - 1.0) * np.pi
    tilt_dir = 2.0 * np.pi * nx()
    tilt = tilt_max * nx()
    zaxis = np.zeros((batch, 3)); zaxis[:, 2] = 1.0
    haxis = np.stack([np.cos(tilt_dir), np.sin(tilt_dir), np.zeros(batch)], axis=-1)
    q_yaw = _axis_angle(zaxis, yaw)
    q = quat_mul(q_yaw, _axis_angle(haxis, tilt))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    rec["quat"] = q
    rec["rot"] = quat_to_rot(q)
    rec["lin_vel_body"] = np.stack([vel_sigma * _normal(nx(), nx()) for _ in range(3)], axis=-1)
    rec["ang_vel_body"] = np.stack([0.5 * _normal(nx(), nx()) for _ in range(3)], axis=-1)
    feet = np.zeros((batch, 8, 3))
    corners = np.array([[0.1, 0.05], [0.1, -0.05], [-0.1, 0.05], [-0.1, -0.05]])
    for foot, ysign in ((0, 1.0), (1, -1.0)):
        centre = np.stack([0.06 * nx() - 0.03, ysign * 0.1 + 0.06 * nx() - 0.03, -0.85 + 0.06 * nx() - 0.03], axis=-1)
        for k in range(4):
            feet[:, 4 * foot + k, 0] = centre[:, 0] + corners[k, 0]
            feet[:, 4 * foot + k, 1] = centre[:, 1] + corners[k, 1]
            feet[:, 4 * foot + k, 2] = centre[:, 2]
    rec["foot_pos_body"] = feet.reshape(batch, 24)
    g = nx()
    contacts = np.ones((batch, 8))
    contacts[(g >= 0.4) & (g < 0.7), 4:] = 0.0      # left foot only
    contacts[g >= 0.7, :4] = 0.0                    # right foot only
    rec["contacts"] = contacts
    rec["pos_ref_body"] = np.stack([0.02 * _normal(nx(), nx()) for _ in range(3)], axis=-1)
    rec["vel_ref_body"] = np.stack([nx() - 0.5, 0.2 * nx() - 0.1, np.zeros(batch)], axis=-1)
    small = np.stack([0.05 * _normal(nx(), nx()) for _ in range(2)] + [np.zeros(batch)], axis=-1)
    ang = np.linalg.norm(small, axis=-1)
    ax_ = np.where(ang[:, None] > 0, small / np.maximum(ang, 1e-300)[:, None], haxis)
    qd = quat_mul(q_yaw, _axis_angle(ax_, ang))
    qd /= np.linalg.norm(qd, axis=-1, keepdims=True)
    rec["quat_d"] = qd
    return rec


def random_go1_variants(batch: int, seed: int = 0, first: int = 0, base=None) -> np.ndarray:
    """`batch` per-instance records (``struct qmpc_instance_params``, for Solver.solve_instances) of Go1 variants around
    `base` (default: the Go1 values of qmpc_default_params), instance indices first .. first+batch-1, same counter-based
    generator as the states: mass U(10, 16) kg; inertia scaled by the mass ratio times U(0.8, 1.2) per axis (D I D with
    D = diag(sqrt(scale)), so it stays symmetric positive definite); mu U(0.3, 0.9); fz_max U(80, 200) N; Q and R each
    scaled by one U(0.5, 2) factor; w unchanged."""
    from . import default_params, instance_params

    base = default_params(10) if base is None else base
    rec = instance_params(base, batch)
    idx = np.arange(first, first + batch, dtype=np.uint64)
    u = _uniform(0x5EED1000 + int(seed), idx, 8)
    mass = 10.0 + 6.0 * u[:, 0]
    scale = (mass / base.mass)[:, None] * (0.8 + 0.4 * u[:, 1:4])
    d = np.sqrt(scale)
    inertia = np.asarray(base.inertia[:], dtype=np.float64).reshape(3, 3)
    rec["mass"] = mass
    rec["inertia"] = (d[:, :, None] * inertia[None] * d[:, None, :]).reshape(batch, 9)
    rec["mu"] = 0.3 + 0.6 * u[:, 4]
    rec["fz_max"] = 80.0 + 120.0 * u[:, 5]
    rec["q_weights"] *= (0.5 + 1.5 * u[:, 6])[:, None]
    rec["r_weights"] *= (0.5 + 1.5 * u[:, 7])[:, None]
    return rec


def random_go1_convex_variants(batch: int, seed: int = 0, first: int = 0, base=None) -> np.ndarray:
    """`batch` per-instance records for Solver.convex_solve_instances: the spread of random_go1_variants around `base`
    (default: the ConvexMpc values of qmpc_default_convex_params).  The same generator and counters: with the same seed robot i
    has the mass, the per-axis inertia factors, the friction, the force bound and the two cost factors of
    random_go1_variants' robot i -- one fleet under both controllers."""
    from . import default_convex_params

    return random_go1_variants(batch, seed, first, default_convex_params(10) if base is None else base)


def random_go1_plants(batch: int, seed: int = 0, first: int = 0, base=None, payload=(0.0, 4.0), inertia_scale=(0.8, 1.2),
                      force=(0.0, 0.0)) -> np.ndarray:
    """`batch` TRUE-plant records (``struct qmpc_plant_params``, for Solver.loop_run_instances) of Go1 robots around `base`
    (default: qmpc_default_params' Go1), robot indices first .. first+batch-1, the counter-based generator of
    random_go1_variants: a payload U(payload) kg on top of the base mass, the inertia scaled by the mass ratio times
    U(inertia_scale) per axis (D I D, D = diag(sqrt(scale)): symmetric positive definite), and a constant horizontal
    disturbance force of magnitude U(force) N at the CoM in a uniformly random direction (no disturbance torque)."""
    from . import default_params, plant_params

    base = default_params(10) if base is None else base
    rec = plant_params(base, batch)
    idx = np.arange(first, first + batch, dtype=np.uint64)
    u = _uniform(0x5EED2000 + int(seed), idx, 6)
    mass = base.mass + payload[0] + (payload[1] - payload[0]) * u[:, 0]
    scale = (mass / base.mass)[:, None] * (inertia_scale[0] + (inertia_scale[1] - inertia_scale[0]) * u[:, 1:4])
    d = np.sqrt(scale)
    inertia = np.asarray(base.inertia[:], dtype=np.float64).reshape(3, 3)
    rec["mass"] = mass
    rec["inertia"] = (d[:, :, None] * inertia[None] * d[:, None, :]).reshape(batch, 9)
    mag = force[0] + (force[1] - force[0]) * u[:, 4]
    ang = 2.0 * np.pi * u[:, 5]
    rec["ext_force_world"][:, 0] = mag * np.cos(ang)
    rec["ext_force_world"][:, 1] = mag * np.sin(ang)
    return rec


def random_go1_pushes(batch: int, seed: int = 0, first: int = 0, per_robot: int = 1, start=(0.0, 91.0), ticks=(4.0, 20.0),
                      impulse=(0.0, 10.0), dt: float = 0.005) -> np.ndarray:
    """`batch` x `per_robot` push windows (``struct qmpc_push_params``, for Solver.loop_run_pushes), robot indices
    first .. first+batch-1, the counter-based generator of random_go1_plants (a shard equals its block of the whole): window k
    of a robot starts at tick floor(U(start)), lasts max(1, floor(U(ticks))) ticks and carries an impulse of U(impulse) N s in
    a horizontal, uniformly random direction -- a force of magnitude impulse / (ticks * dt) N at the CoM, no torque.  Four
    uniforms per window, in the order start, ticks, impulse, direction."""
    from . import push_params

    rec = push_params(batch, per_robot)
    idx = np.arange(first, first + batch, dtype=np.uint64)
    u = _uniform(0x5EED3000 + int(seed), idx, 4 * int(per_robot)).reshape(batch, int(per_robot), 4)
    rec["start_tick"] = np.floor(start[0] + (start[1] - start[0]) * u[:, :, 0])
    n = np.maximum(1.0, np.floor(ticks[0] + (ticks[1] - ticks[0]) * u[:, :, 1]))
    rec["ticks"] = n
    mag = (impulse[0] + (impulse[1] - impulse[0]) * u[:, :, 2]) / (n * dt)
    ang = 2.0 * np.pi * u[:, :, 3]
    rec["force_world"][:, :, 0] = mag * np.cos(ang)
    rec["force_world"][:, :, 1] = mag * np.sin(ang)
    return rec


def random_go1_grounds(batch: int, seed: int = 0, first: int = 0, mu=(0.1, 0.9), fz_max=None) -> np.ndarray:
    """`batch` ground records (``struct qmpc_ground_params``, for Solver.loop_run_ground), robot indices first .. first+batch-1,
    the counter-based generator of random_go1_pushes (a shard equals its block of the whole): one true friction coefficient
    U(mu) per robot, copied to its four legs, and -- with fz_max = (lo, hi) -- one normal-force limit U(fz_max) N per robot,
    copied likewise (None: +inf, no limit).  Two uniforms per robot, in the order mu, fz_max."""
    from . import ground_params

    rec = ground_params(batch)
    idx = np.arange(first, first + batch, dtype=np.uint64)
    u = _uniform(0x5EED4000 + int(seed), idx, 2)
    rec["mu"] = (mu[0] + (mu[1] - mu[0]) * u[:, 0])[:, None]
    if fz_max is not None:
        rec["fz_max"] = (fz_max[0] + (fz_max[1] - fz_max[0]) * u[:, 1])[:, None]
    return rec


def random_go1_actuations(batch: int, seed: int = 0, first: int = 0, delay=(0, 4), tau=None, dt: float = 0.005) -> np.ndarray:
    """`batch` actuation records (``struct qmpc_actuation_params``, for Solver.loop_run_actuation), robot indices first ..
    first+batch-1, the counter-based generator of random_go1_pushes (a shard equals its block of the whole): one delay per robot,
    an integer uniform on delay[0] .. delay[1] ticks, and -- with tau = (lo, hi) -- one actuator time constant U(tau) seconds per
    robot, sampled at the tick dt (None: no lag, alpha = 1).  Two uniforms per robot, in the order delay, tau."""
    from . import actuation_params

    idx = np.arange(first, first + batch, dtype=np.uint64)
    u = _uniform(0x5EED5000 + int(seed), idx, 2)
    d = np.minimum(np.floor(delay[0] + (delay[1] - delay[0] + 1) * u[:, 0]), delay[1])
    t = None if tau is None else tau[0] + (tau[1] - tau[0]) * u[:, 1]
    return actuation_params(batch, delay_ticks=d, tau=t, dt=dt)


def random_go1_senses(batch: int, seed: int = 0, first: int = 0, pos_noise=(0.0, 0.01), att_noise=(0.0, 0.01), vel_noise=(0.0, 0.05),
                      gyro_noise=(0.0, 0.02), gyro_bias=(0.0, 0.02), pos_bias=(0.0, 0.02)) -> np.ndarray:
    """`batch` sensing records (``struct qmpc_sense_params``, for Solver.loop_run_sensing), robot indices first .. first+batch-1,
    the counter-based generator of random_go1_pushes (a shard equals its block of the whole).  Per robot one noise level per
    channel group, U(*_noise), copied to the group's three axes -- position [m], attitude [rad], world-frame velocity [m/s], body
    rate [rad/s] -- and per axis a gyro bias and a position bias, uniform on +-U-range: magnitude U(*_bias) with a random sign.
    The noise seed of robot i is seed * 2^32 + i, so no two robots of a sweep share their noise.  The default ranges are
    ASSUMPTIONS about a small quadruped's leg-odometry / IMU estimator (a centimetre of position noise, a degree of attitude,
    centimetres per second of velocity, a degree per second of gyro noise and bias), not measurements of a Go1: sweep them.
    Sixteen uniforms per robot, in the order pos, att, vel, gyro noise, gyro bias magnitude x 3, its sign x 3, position bias
    magnitude x 3, its sign x 3."""
    from . import sense_params

    idx = np.arange(first, first + batch, dtype=np.uint64)
    u = _uniform(0x5EED6000 + int(seed), idx, 16)
    lin = lambda r, v: r[0] + (r[1] - r[0]) * v      # noqa: E731
    sign = lambda v: np.where(v < 0.5, -1.0, 1.0)      # noqa: E731
    return sense_params(batch, seed=(int(seed) % (1 << 21)) * float(1 << 32) + idx.astype(np.float64),
                        pos_noise=lin(pos_noise, u[:, 0])[:, None] * np.ones(3), att_noise=lin(att_noise, u[:, 1])[:, None] * np.ones(3),
                        vel_noise=lin(vel_noise, u[:, 2])[:, None] * np.ones(3), gyro_noise=lin(gyro_noise, u[:, 3])[:, None] * np.ones(3),
                        gyro_bias=lin(gyro_bias, u[:, 4:7]) * sign(u[:, 7:10]), pos_bias=lin(pos_bias, u[:, 10:13]) * sign(u[:, 13:16]))


def random_go1_gaits(batch: int, seed: int = 0, first: int = 0, gaits=("trot", "pace", "bound", "trot_overlap", "crawl", "amble"),
                     gait_freq=(1.5, 3.0)) -> np.ndarray:
    """`batch` gait records (``struct qmpc_gait_params``, for Solver.loop_run_gaits), robot indices first .. first+batch-1, the
    counter-based generator of random_go1_pushes (a shard equals its block of the whole).  Per robot one of the named `gaits`,
    uniformly, and a frequency U(gait_freq) [Hz].  The frequency range is an ASSUMPTION: the reference's configurations ship
    1.7, 2.0 and 2.2 Hz for the Go1's trot, the range here brackets them by about a third on either side and is not a
    measurement of what a Go1 can step at in any of the other gaits -- sweep it.  (At the 5 ms tick a record is valid up to
    12.5 Hz.)  Two uniforms per robot: the gait's index, the frequency."""
    from . import gait_params

    idx = np.arange(first, first + batch, dtype=np.uint64)
    u = _uniform(0x5EED7000 + int(seed), idx, 2)
    names = list(gaits)
    k = np.minimum(np.floor(len(names) * u[:, 0]).astype(np.int64), len(names) - 1)
    return gait_params(batch, gait=[names[j] for j in k], gait_freq=gait_freq[0] + (gait_freq[1] - gait_freq[0]) * u[:, 1])


def random_go1_motors(batch: int, seed: int = 0, first: int = 0, scale=(0.5, 1.2)) -> np.ndarray:
    """`batch` motor records (``struct qmpc_motor_params``, for Solver.loop_run_motors), robot indices first .. first+batch-1, the
    counter-based generator of random_go1_pushes (a shard equals its block of the whole).  Per robot the Go1's joint torque
    limits -- 23.7 / 23.7 / 35.55 N m for hip / thigh / calf -- times one factor U(scale) per joint type.  The range is an
    ASSUMPTION: a worn or derated motor on the low side, a generously specified one on the high side; it is not a measurement
    of any robot -- sweep it.  Three uniforms per robot."""
    from . import GO1_TAU_MAX, motor_params

    idx = np.arange(first, first + batch, dtype=np.uint64)
    u = _uniform(0x5EED8000 + int(seed), idx, 3)
    k = scale[0] + (scale[1] - scale[0]) * u
    return motor_params(batch, tau_max=np.tile(k * np.asarray(GO1_TAU_MAX), (1, 4)))
