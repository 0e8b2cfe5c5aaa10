"""An independent statement of the closed loop's plant and of the few lines of the post step around it (a helper beside
tests/kkt_independent.py, not a test).

Plain numpy in np.longdouble (64-bit mantissa on x86), vectorised over robots.  It is written from the MODEL, not from the text of
csrc/qmpc_loop_math.h, and imports or parses nothing of the package's C sources:

    p' = v
    v' = (R(q) sum_l u_l + f_ext) / m + g                 g = (0, 0, -9.81)
    q' = 1/2 q (x) (0, w)                                 Hamilton product, q = (w, x, y, z), w in the body frame
    w' = I^-1 (sum_l r_l x u_l + tau_ext)                 r_l = R(q)' (foot_l - p); NO gyroscopic term (the header's choice)

u_l are the body-frame foot forces, f_ext acts at the CoM in the world frame, tau_ext in the body frame.  R(q) is the textbook
matrix of a unit quaternion, R = I + 2 w [v]x + 2 [v]x [v]x with q = (w, v).  One tick is one explicit-midpoint step of length dt
with feet and forces held, then q / |q|.  The midpoint stage's quaternion is not exactly unit (|q|^2 - 1 = O(dt^2 |w|^2)); the
textbook matrix is applied to it as it stands, which is part of the discretisation the header defines, not of the ODE.

I^-1 is the inverse of the record's inertia by Gauss-Jordan elimination with partial pivoting in longdouble.

Also here: a fine classical RK4 integration of the same ODE (the truncation-error tests), the effective wrench of a tick under push
windows from the definition in include/qmpc.h, the longdouble statements of the attitude conversions, and the bookkeeping of one
tick's post step (applied forces in both frames, swing-foot relocation, tick counter)."""
import numpy as np

LD = np.longdouble
GRAVITY = LD("9.81")
U = LD(2) ** -52      # the unit the bounds are counted in: one ulp of a double in [1, 2)


def usable() -> bool:
    """np.longdouble must carry at least 60 mantissa bits (x87 extended: 63), or the reference is no better than the double code"""
    return bool(np.finfo(LD).eps <= LD(2) ** -60)


def ld(a):
    return np.asarray(a, dtype=LD)


# ---- quaternions and rotations -------------------------------------------------------------------------------------------------
def quat_mul(a, b):
    """Hamilton product of (..., 4) quaternions (w, x, y, z)"""
    a, b = ld(a), ld(b)
    aw, av = a[..., :1], a[..., 1:]
    bw, bv = b[..., :1], b[..., 1:]
    w = aw * bw - (av * bv).sum(axis=-1, keepdims=True)
    v = aw * bv + bw * av + np.cross(av, bv)
    return np.concatenate([w, v], axis=-1)


def hat(v):
    """[v]x of (..., 3) vectors: hat(v) @ a = v x a"""
    v = ld(v)
    z = np.zeros(v.shape[:-1], dtype=LD)
    x, y, w = v[..., 0], v[..., 1], v[..., 2]
    return np.stack([np.stack([z, -w, y], axis=-1), np.stack([w, z, -x], axis=-1), np.stack([-y, x, z], axis=-1)], axis=-2)


def rot(q):
    """body -> world rotation of (..., 4) quaternions: the textbook matrix I + 2 w [v]x + 2 [v]x^2"""
    q = ld(q)
    K = hat(q[..., 1:])
    return np.eye(3, dtype=LD) + 2 * q[..., :1, None] * K + 2 * (K @ K)


def rot_by_product(q, v):
    """q (x) (0, v) (x) q*: the rotation of v by a UNIT quaternion, as a second statement of rot(q) @ v"""
    q, v = ld(q), ld(v)
    qc = q * ld([1, -1, -1, -1])
    pure = np.concatenate([np.zeros(v.shape[:-1] + (1,), dtype=LD), v], axis=-1)
    return quat_mul(quat_mul(q, pure), qc)[..., 1:]


def rot_z(R):
    """the yaw-only rotation beside R: yaw = atan2(R[1, 0], R[0, 0])"""
    R = ld(R)
    yaw = np.arctan2(R[..., 1, 0], R[..., 0, 0])
    c, s, z, o = np.cos(yaw), np.sin(yaw), np.zeros_like(yaw), np.ones_like(yaw)
    return np.stack([np.stack([c, -s, z], axis=-1), np.stack([s, c, z], axis=-1), np.stack([z, z, o], axis=-1)], axis=-2)


def euler(q):
    """roll, pitch, yaw (ZYX) of (..., 4) quaternions; the pitch's sine is clamped to [-1, 1]"""
    q = ld(q)
    w, x, y, z = (q[..., k] for k in range(4))
    roll = np.arctan2(2 * (w * x + y * z), 1 - 2 * (x * x + y * y))
    pitch = np.arcsin(np.clip(2 * (w * y - z * x), -1, 1))
    yaw = np.arctan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z))
    return np.stack([roll, pitch, yaw], axis=-1)


def inv(A):
    """inverse of (B, 3, 3) matrices by Gauss-Jordan elimination with partial pivoting"""
    A = ld(A)
    B, n = A.shape[0], A.shape[-1]
    M = np.concatenate([A, np.broadcast_to(np.eye(n, dtype=LD), A.shape)], axis=-1).copy()
    rows = np.arange(B)
    for c in range(n):
        piv = c + np.argmax(np.abs(M[:, c:, c]), axis=1)
        top, low = M[rows, c].copy(), M[rows, piv].copy()
        M[rows, c], M[rows, piv] = low, top
        M[:, c] = M[:, c] / M[:, c, c][:, None]
        for r in range(n):
            if r != c:
                M[:, r] = M[:, r] - M[:, r, c][:, None] * M[:, c]
    return M[:, :, n:]


# ---- the plant -----------------------------------------------------------------------------------------------------------------
def rate(x, u, feet, mass, Iinv, f_ext=None, tau_ext=None):
    """x' of (B, 13) states [p q v w] under (B, L, 3) body-frame forces at (B, L, 3) world-frame feet"""
    x, u, feet = ld(x), ld(u), ld(feet)
    p, q, v, w = x[:, 0:3], x[:, 3:7], x[:, 7:10], x[:, 10:13]
    R = rot(q)
    Rt = np.swapaxes(R, -1, -2)
    r = np.einsum("bij,blj->bli", Rt, feet - p[:, None, :])
    tau = np.cross(r, u).sum(axis=1)
    F = np.einsum("bij,bj->bi", R, u.sum(axis=1))
    if f_ext is not None:
        F = F + ld(f_ext)
    if tau_ext is not None:
        tau = tau + ld(tau_ext)
    vd = F / ld(mass)[:, None]
    vd[:, 2] -= GRAVITY
    qd = quat_mul(q, np.concatenate([np.zeros((len(x), 1), dtype=LD), w], axis=1)) / 2
    wd = np.einsum("bij,bj->bi", ld(Iinv), tau)
    return np.concatenate([v, qd, vd, wd], axis=1)


def _unit(x):
    x = x.copy()
    x[:, 3:7] = x[:, 3:7] / np.sqrt((x[:, 3:7] ** 2).sum(axis=1, keepdims=True))
    return x


def midpoint_step(x, u, feet, mass, inertia, dt, f_ext=None, tau_ext=None):
    """one tick of the plant: explicit midpoint, then the quaternion re-normalised.  inertia (B, 3, 3) is inverted here."""
    x, dt = ld(x), LD(dt)
    Iinv = inv(ld(inertia).reshape(-1, 3, 3))
    k1 = rate(x, u, feet, mass, Iinv, f_ext, tau_ext)
    k2 = rate(x + dt / 2 * k1, u, feet, mass, Iinv, f_ext, tau_ext)
    return _unit(x + dt * k2)


def fine_step(x, u, feet, mass, inertia, dt, f_ext=None, tau_ext=None, substeps=400):
    """the same ODE over dt by classical RK4 in `substeps` steps, forces and feet held; re-normalised at the end"""
    x, h = ld(x), LD(dt) / substeps
    Iinv = inv(ld(inertia).reshape(-1, 3, 3))
    f = lambda y: rate(y, u, feet, mass, Iinv, f_ext, tau_ext)      # noqa: E731
    for _ in range(substeps):
        k1 = f(x)
        k2 = f(x + h / 2 * k1)
        k3 = f(x + h / 2 * k2)
        k4 = f(x + h * k3)
        x = x + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
    return _unit(x)


# ---- the effective wrench of a tick (include/qmpc.h, "timed push disturbances per robot") -----------------------------------------
def effective_wrench(force, torque, push, tick_before):
    """force / torque (B, 3): the plant record's constant disturbance (zeros without plant records); push: None or (B, K) records
    with start_tick, ticks, force_world, torque_body; tick_before (B,): state.tick before the tick.  Window k acts when
    t >= start_tick and t < start_tick + ticks; ticks <= 0 never acts.  Returns the sums (B, 3), (B, 3) and the number of active
    windows per robot."""
    f, tq = ld(force).copy(), ld(torque).copy()
    active_n = np.zeros(len(f), dtype=int)
    if push is None:
        return f, tq, active_n
    t = np.asarray(tick_before, dtype=np.float64)
    for k in range(push.shape[1]):
        w = push[:, k]
        active = (w["ticks"] > 0) & (t >= w["start_tick"]) & (t < w["start_tick"] + w["ticks"])
        f[active] += ld(w["force_world"][active])
        tq[active] += ld(w["torque_body"][active])
        active_n += active
    return f, tq, active_n


# ---- one tick's post step ---------------------------------------------------------------------------------------------------------
def state13(s):
    """(B, 13) [p q v w] of loop-state records"""
    return np.concatenate([ld(s["pos_world"]), ld(s["quat"]), ld(s["lin_vel_world"]), ld(s["ang_vel_body"])], axis=1)


def post_tick(before, after, mass, inertia, force, torque, dt):
    """What the post step of one tick must leave, from the state records before and after it.  The plant starts from `before`
    (attitude, position, velocities, foot_pos_world) under after["forces_body"] -- the forces the tick applied -- with the given
    mass (B,), inertia (B, 3, 3) and effective wrench (B, 3) each.  Returns a dict:
      x          (B, 13) the plant state after the tick
      grf_world  (B, 4, 3) R(q_before) forces_body
      body_of_grf (B, 4, 3) R(q_before)' after["grf_world"]  (ConvexMpc's tick: forces_body = R' u)
      feet       (B, 4, 3) float64: a leg with contacts == 0 under movement_mode != 0 sits at its leg's fsm_pos, every other foot
                 where it was -- copies, to be compared byte for byte
      tick       (B,) before["tick"] + 1"""
    B = len(before)
    u = ld(after["forces_body"]).reshape(B, 4, 3)
    feet0 = before["foot_pos_world"].reshape(B, 4, 3)
    x = midpoint_step(state13(before), u, feet0, mass, inertia, dt, force, torque)
    R = rot(before["quat"])
    grf = np.einsum("bij,blj->bli", R, u)
    body = np.einsum("bji,blj->bli", R, ld(after["grf_world"]).reshape(B, 4, 3))
    swing = (after["contacts"] == 0) & (after["movement_mode"] != 0)[:, None]
    feet = np.where(swing[:, :, None], after["leg"]["fsm_pos"], feet0)
    return {"x": x, "grf_world": grf, "body_of_grf": body, "feet": feet, "swing": swing, "tick": before["tick"] + 1}


# ---- the bound ------------------------------------------------------------------------------------------------------------------
# K: the bound on |double result - reference| in units of 2^-52 max(1, |reference|), for the host build AND every device build
# (tests/test_gpu_loop_plant.py imports these and does not re-tune them).  Each is 4 x the worst value measured by
# tests/test_plant_reference_cpu.py on the host build (2048 rows per set, walking / harsh), rounded up to a power of two.  The
# margin is for a device compiler rounding a product differently where it is free to; it cannot hide a wrong term, which is an
# error of order 1e-3 (10^12 units) or more on these inputs.
K = {
    "pos_world": 2,          # measured 0.487 / 0.485
    "quat": 8,               # measured 0.938 / 1.055
    "lin_vel_world": 4,      # measured 0.272 / 0.536
    "ang_vel_body": 128,     # measured 10.69 / 28.48: I^-1 ~ 14 .. 35 amplifies the cancellation in sum r x u
    "rot": 8,                # quat_to_rot's entries: measured 1.044
    "rot_product": 8,        # R f and R' f, unit: the vector's largest component; measured 1.555 / 1.743
    "rot_z": 8,              # measured 1.043
    "euler": 4,              # measured 0.883 (|pitch| <= 1 rad)
    "inv": 4,                # inv3: |B A - 1| and |B - A^-1| / |A^-1| in units of 2^-52 cond_inf(A); measured 0.572
}
GROUPS = {"pos_world": slice(0, 3), "quat": slice(3, 7), "lin_vel_world": slice(7, 10), "ang_vel_body": slice(10, 13)}


def units(got, want):
    """|got - want| in units of 2^-52 max(1, |want|), per component (got: float64, want: longdouble)"""
    want = ld(want)
    return np.abs(ld(got) - want) / (U * np.maximum(1, np.abs(want)))


def units_vec(got, want):
    """|got - want| in units of 2^-52 max(1, |want|_inf of the 3-vector): for products of a rotation with a vector, whose
    components cancel"""
    want = ld(want)
    return np.abs(ld(got) - want) / (U * np.maximum(1, np.abs(want).max(axis=-1, keepdims=True)))
