"""CPU suite: the closed loop's plant against an independent reference (tests/plant_reference.py).

First half -- the reference alone, against closed forms and a fine integration, so that it cannot be a faithful copy of a wrong
formula: free fall, torque-free spin, a constant torque, the sign and frame of r x f, and the order of the step.

Second half -- the host build of csrc/qmpc_loop_math.h (tests/native/plant_step_host.cpp, compiled host-only by hipcc like
tests/native/loop_instances_host.cpp) against the reference, on a seeded counter-based generator of inputs: plant_step,
plant_step_ext, quat_to_rot, rot_to_rot_z, quat_to_euler, inv3 and loop_push_wrench, within the constants K of
tests/plant_reference.py (4 x the worst error measured here, rounded up to a power of two, in units of 2^-52 max(1, |reference|)).
tests/test_gpu_loop_plant.py holds every device build of the tick to the same reference and the same constants."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import plant_reference as ref

HERE = Path(__file__).resolve().parent
SRC = HERE / "native" / "plant_step_host.cpp"
HIPCC = "/opt/rocm/bin/hipcc"
LD = ref.LD
DT = 0.005
ROWS = 2048      # per set

pytestmark = pytest.mark.skipif(not ref.usable(), reason="np.longdouble carries fewer than 60 mantissa bits here")


# ---- the generator: counter-based, seeded -------------------------------------------------------------------------------------
def _uniform(seed, stream, n, k, first=0):
    """(n, k) uniforms in [0, 1): SplitMix64's finaliser of the counter (row, column) under (seed, stream); row i is the same
    whatever n is"""
    m = np.uint64
    idx = (np.arange(first, first + n, dtype=np.uint64)[:, None] * m(k) + np.arange(k, dtype=np.uint64)[None, :])
    z = idx * m(0x9E3779B97F4A7C15) + np.full_like(idx, seed) * m(0xD1B54A32D192ED03) + np.full_like(idx, stream) * m(0x8CB92BA72F3D8DD7)
    z = (z ^ (z >> m(30))) * m(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> m(27))) * m(0x94D049BB133111EB)
    z = z ^ (z >> m(31))
    return (z >> m(11)).astype(np.float64) / 2.0 ** 53


def _between(u, a, b):
    return a + (b - a) * u


def _attitude(u, tilt_max):
    """yaw in (-pi, pi), then a tilt of up to tilt_max about a random axis: (n, 4) doubles, unit to rounding.  u: (n, 5)"""
    yaw = _between(u[:, 0], -np.pi, np.pi)
    axis = _between(u[:, 1:4], -1.0, 1.0) + 1e-3
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    ang = tilt_max * u[:, 4]
    z = np.zeros_like(yaw)
    qy = np.stack([np.cos(yaw / 2), z, z, np.sin(yaw / 2)], axis=1)
    qt = np.concatenate([np.cos(ang / 2)[:, None], np.sin(ang / 2)[:, None] * axis], axis=1)
    q = ref.quat_mul(qy, qt)
    q = q / np.sqrt((q * q).sum(axis=1, keepdims=True))
    return q.astype(np.float64), yaw


GO1_MASS = 12.84
GO1_INERTIA = np.diag([0.0168128557, 0.063009565, 0.0716547275]) * (12.84 / 5.204)
FOOTHOLDS = np.array([[0.20, 0.14], [0.20, -0.14], [-0.20, 0.14], [-0.20, -0.14]])


def _feet(u, p, yaw, spread):
    """feet near the Go1 footholds under the body: (n, 4, 3).  u: (n, 12)"""
    c, s = np.cos(yaw), np.sin(yaw)
    fx = p[:, None, 0] + c[:, None] * FOOTHOLDS[None, :, 0] - s[:, None] * FOOTHOLDS[None, :, 1]
    fy = p[:, None, 1] + s[:, None] * FOOTHOLDS[None, :, 0] + c[:, None] * FOOTHOLDS[None, :, 1]
    feet = np.stack([fx, fy, np.zeros_like(fx)], axis=2)
    return feet + _between(u.reshape(-1, 4, 3), -spread, spread) * np.array([1.0, 1.0, 0.4]) + np.array([0.0, 0.0, 0.4 * spread])


def walking(n, seed=20240501):
    """tilt <= 0.3 rad, |v| <~ 1 m/s, |w| <~ 2 rad/s, height 0.2 - 0.4 m, feet near the footholds, vertical forces summing to about
    the weight, 0 - 2 legs with zero force; the Go1's mass and inertia; no disturbance"""
    u = _uniform(seed, 1, n, 48)
    q, yaw = _attitude(u[:, 0:5], 0.3)
    p = np.stack([_between(u[:, 5], -2, 2), _between(u[:, 6], -2, 2), _between(u[:, 7], 0.2, 0.4)], axis=1)
    v = _between(u[:, 8:11], -0.6, 0.6)
    w = _between(u[:, 11:14], -1.2, 1.2)
    feet = _feet(u[:, 14:26], p, yaw, 0.05)
    unloaded = np.floor(u[:, 26] * 3).astype(int)      # 0, 1 or 2 legs in swing: the diagonal pair's members
    first = np.floor(u[:, 27] * 4).astype(int)
    load = np.ones((n, 4))
    load[unloaded >= 1, :] *= (np.arange(4)[None, :] != first[unloaded >= 1, None])
    load[unloaded >= 2, :] *= (np.arange(4)[None, :] != (3 - first[unloaded >= 2, None]))
    fz = GO1_MASS * 9.81 / load.sum(axis=1, keepdims=True) * _between(u[:, 28:32], 0.7, 1.3) * load
    fxy = _between(u[:, 32:40], -0.2, 0.2).reshape(n, 4, 2) * fz[:, :, None]
    f = np.concatenate([fxy, fz[:, :, None]], axis=2)
    x = np.concatenate([p, q, v, w], axis=1)
    return {"x": x, "u": f, "feet": feet, "mass": np.full(n, GO1_MASS), "inertia": np.broadcast_to(GO1_INERTIA, (n, 3, 3)).copy(),
            "f_ext": np.zeros((n, 3)), "tau_ext": np.zeros((n, 3))}


def harsh(n, seed=20240502):
    """tilt <= 1 rad, every third quaternion with negative w, forces to 120 N per leg and component, unbalanced, mass 10 - 17 kg,
    a skewed inertia (symmetric off-diagonals AND an antisymmetric part, so that a transposed inverse shows), f_ext to 40 N,
    tau_ext to 2 N m, every fifth row with one exactly zero component in each"""
    u = _uniform(seed, 2, n, 64)
    q, yaw = _attitude(u[:, 0:5], 1.0)
    q *= np.where(q[:, :1] < 0, -1.0, 1.0)
    q[::3] = -q[::3]
    assert (q[::3, 0] < 0).all() and (q[1::3, 0] > 0).all()
    p = np.stack([_between(u[:, 5], -3, 3), _between(u[:, 6], -3, 3), _between(u[:, 7], 0.15, 0.5)], axis=1)
    v = _between(u[:, 8:11], -2, 2)
    w = _between(u[:, 11:14], -4, 4)
    feet = _feet(u[:, 14:26], p, yaw, 0.12)
    f = _between(u[:, 26:38], -120, 120).reshape(n, 4, 3)
    mass = _between(u[:, 38], 10, 17)
    inertia = GO1_INERTIA[None] * _between(u[:, 39:42], 0.7, 1.3)[:, :, None]
    off = _between(u[:, 42:45], -0.004, 0.004)
    skew = _between(u[:, 45:48], -0.002, 0.002)
    for k, (a, b) in enumerate(((0, 1), (0, 2), (1, 2))):
        inertia[:, a, b] = off[:, k] + skew[:, k]
        inertia[:, b, a] = off[:, k] - skew[:, k]
    f_ext = _between(u[:, 48:51], -40, 40)
    tau_ext = _between(u[:, 51:54], -2, 2)
    f_ext[::5, 1] = 0.0
    tau_ext[::5, 2] = -0.0
    x = np.concatenate([p, q, v, w], axis=1)
    return {"x": x, "u": f, "feet": feet, "mass": mass, "inertia": inertia, "f_ext": f_ext, "tau_ext": tau_ext}


def _reference_step(s, dt=DT, rows=slice(None), step=ref.midpoint_step):
    return step(s["x"][rows], s["u"][rows], s["feet"][rows], s["mass"][rows], s["inertia"][rows], dt, s["f_ext"][rows], s["tau_ext"][rows])


# ================================================================================================================================
# first half: the reference is itself right
# ================================================================================================================================
def test_free_fall_is_the_parabola():
    """no forces: the midpoint rule is exact for p'' = g, so only longdouble rounding remains after 200 ticks"""
    s = walking(16)
    s["u"][:] = 0.0
    x0 = ref.ld(s["x"])
    x, T = x0, 0
    for _ in range(200):
        x = ref.midpoint_step(x, s["u"], s["feet"], s["mass"], s["inertia"], DT)
        T += 1
    t = LD(DT) * T
    g = ref.ld([0, 0, -1]) * ref.GRAVITY
    want_p = x0[:, 0:3] + x0[:, 7:10] * t + g * t * t / 2
    want_v = x0[:, 7:10] + g * t
    ep, ev = float(np.abs(x[:, 0:3] - want_p).max()), float(np.abs(x[:, 7:10] - want_v).max())
    print(f"free fall over {T} ticks: position error {ep:.2e}, velocity error {ev:.2e}")
    assert ep < 1e-16 and ev < 1e-16
    assert float(np.abs(x[:, 10:13] - x0[:, 10:13]).max()) == 0.0      # and nothing turns the body faster


def test_torque_free_spin_is_second_order():
    """inertia = identity, no forces, constant w: after T the attitude is q0 (x) (cos(|w| T / 2), sin(|w| T / 2) w / |w|); the
    error of the re-normalised midpoint step falls by 4 +- 0.5 when dt halves"""
    n, T = 8, LD("0.32")
    s = walking(n)
    s["u"][:] = 0.0
    s["inertia"][:] = np.eye(3)
    s["x"][:, 10:13] = _between(_uniform(7, 3, n, 3), -1.0, 1.0) * 3.0
    w = ref.ld(s["x"][:, 10:13])
    wn = np.sqrt((w * w).sum(axis=1, keepdims=True))
    want = ref.quat_mul(s["x"][:, 3:7], np.concatenate([np.cos(wn * T / 2), np.sin(wn * T / 2) * w / wn], axis=1))
    errs = []
    for steps in (16, 32, 64, 128):
        x = ref.ld(s["x"])
        for _ in range(steps):
            x = ref.midpoint_step(x, s["u"], s["feet"], s["mass"], s["inertia"], T / steps)
        assert float(np.abs(x[:, 10:13] - w).max()) == 0.0
        errs.append(np.sqrt(((x[:, 3:7] - want) ** 2).sum(axis=1)).astype(np.float64))
    errs = np.array(errs)
    ratios = errs[:-1] / errs[1:]
    print("torque-free spin: attitude errors", errs.max(axis=1), "ratios", ratios.min(), "..", ratios.max())
    assert errs[0].max() < 1e-2 and errs[-1].min() > 1e-9      # truncation, not rounding, is what is measured
    assert (np.abs(ratios - 4.0) <= 0.5).all()


def test_constant_torque_about_a_principal_axis():
    """from rest, a body torque about one principal axis and no forces: w(T) = I^-1 tau T to rounding (w' is constant: the model
    has no gyroscopic term), whatever the body does meanwhile"""
    n, T = 6, 100
    s = walking(n)
    s["u"][:] = 0.0
    s["x"][:, 10:13] = 0.0
    axis = np.arange(n) % 3
    tau = np.zeros((n, 3))
    tau[np.arange(n), axis] = _between(_uniform(7, 4, n, 1)[:, 0], -2, 2)
    x = ref.ld(s["x"])
    for _ in range(T):
        x = ref.midpoint_step(x, s["u"], s["feet"], s["mass"], s["inertia"], DT, None, tau)
    want = ref.ld(tau) / ref.ld(np.diagonal(s["inertia"], axis1=1, axis2=2)) * (LD(DT) * T)
    err = float(np.abs(x[:, 10:13] - want).max())
    print("constant torque: worst error of w(T)", err, "of", float(np.abs(want).max()))
    assert err < 1e-16 * float(np.abs(want).max()) * T
    assert float(np.abs(x[:, 3:7] - ref.ld(s["x"][:, 3:7])).max()) > 1e-2      # (the body did turn)


def test_sign_and_frame_of_the_lever_arm():
    """one force along body z on a tilted, yawed body.  Foot straight under the CoM (body frame): no angular acceleration.  The
    same foot offset by +d along body x: r x f = (d, 0, -h) x (0, 0, F) = (0, -d F, 0), the body pitches about -y.  The linear
    acceleration is R(q) (0, 0, F) / m + g either way."""
    n = 12
    s = harsh(n)
    xs = ref.ld(s["x"])
    xs[:, 3:7] /= np.sqrt((xs[:, 3:7] ** 2).sum(axis=1, keepdims=True))      # unit in longdouble: the two rotations then agree
    q, p = xs[:, 3:7], xs[:, 0:3]
    F, h, d = LD(90), LD("0.3"), LD("0.07")
    u = np.zeros((n, 1, 3), dtype=LD)
    u[:, 0, 2] = F
    Iinv = ref.inv(s["inertia"])

    def foot(body):      # world position of a body-frame point, by the quaternion product (not by rot())
        return (p + ref.rot_by_product(q, np.broadcast_to(ref.ld(body), (n, 3))))[:, None, :]

    centred = ref.rate(xs, u, foot([0, 0, -h]), s["mass"], Iinv)
    assert float(np.abs(centred[:, 10:13]).max()) < 1e-14      # of d F / Iyy ~ 10^2
    offset = ref.rate(xs, u, foot([d, 0, -h]), s["mass"], Iinv)
    want = np.einsum("bij,j->bi", Iinv, ref.ld([0, -d * F, 0]))
    assert float(np.abs(offset[:, 10:13] - want).max()) < 1e-14 * float(np.abs(want).max())
    assert (want[:, 1] < 0).all() and (offset[:, 11] < 0).all()
    acc = ref.rot_by_product(q, np.broadcast_to(ref.ld([0, 0, F]), (n, 3))) / ref.ld(s["mass"])[:, None]
    acc[:, 2] -= ref.GRAVITY
    for got in (centred, offset):
        assert float(np.abs(got[:, 7:10] - acc).max()) < 1e-15
    # world-frame disturbance: f_ext is NOT rotated, tau_ext is added in the body frame
    f_ext, tau_ext = ref.ld([3, -4, 5]), ref.ld([0.5, 0, -0.25])
    both = ref.rate(xs, u, foot([0, 0, -h]), s["mass"], Iinv, np.broadcast_to(f_ext, (n, 3)), np.broadcast_to(tau_ext, (n, 3)))
    assert float(np.abs(both[:, 7:10] - (acc + f_ext / ref.ld(s["mass"])[:, None])).max()) < 1e-15
    assert float(np.abs(both[:, 10:13] - np.einsum("bij,j->bi", Iinv, tau_ext)).max()) < 1e-14
    # and rot() is the rotation by the quaternion product, for unit quaternions
    vecs = ref.ld(_between(_uniform(7, 5, n, 3), -1, 1))
    assert float(np.abs(np.einsum("bij,bj->bi", ref.rot(q), vecs) - ref.rot_by_product(q, vecs)).max()) < 1e-15


def test_the_inverse_is_an_inverse():
    A = harsh(64)["inertia"]
    B = ref.inv(A)
    assert float(np.abs(B @ ref.ld(A) - np.eye(3)).max()) < 1e-16
    assert float(np.abs(ref.inv(np.array([[[0.0, 2.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 4.0]]])) -
                        ref.ld([[0, 1, 0], [0.5, 0, 0], [0, 0, 0.25]])).max()) == 0.0      # needs the pivoting


def _one_step_errors(s, dts, step):
    out = []
    for dt in dts:
        fine = _reference_step(s, dt, step=ref.fine_step)
        d = _reference_step(s, dt, step=step) - fine
        out.append(np.sqrt((d * d).sum(axis=1)).astype(np.float64))
    return np.array(out)


def test_order_of_the_step():
    """The one-step difference between the midpoint reference and a fine integration of the same ODE (classical RK4 in
    longdouble, 400 substeps per tick, forces and feet held) falls by a factor in [5, 12] each time dt halves over
    20 ms -> 10 ms -> 5 ms: the local error of an order-2 method is O(dt^3), factor 8; order 1 gives 4, order 3 gives 16.  40 states: 20 walking, 20 harsh."""
    dts = (0.02, 0.01, 0.005)
    for name, s in (("walking", walking(20)), ("harsh", harsh(20))):
        e = _one_step_errors(s, dts, ref.midpoint_step)
        r = e[:-1] / e[1:]
        print(f"{name}: one-step error at 5 ms up to {e[-1].max():.3e}; factors per halving {r.min():.2f} .. {r.max():.2f}")
        assert (r >= 5).all() and (r <= 12).all()


def test_truncation_error_of_one_tick_is_reported():
    """the worst one-tick truncation error at 5 ms on walking-sized inputs, per component group: a measured property of the plant
    (DESIGN.md records it), printed, not asserted beyond its being a truncation error at all.  The set's forces are not balanced
    about the CoM (net torques are printed beside it), which is what the angular velocity's error comes from."""
    s = walking(256)
    d = np.abs(_reference_step(s) - _reference_step(s, step=ref.fine_step)).astype(np.float64)
    worst = {g: float(d[:, sl].max()) for g, sl in ref.GROUPS.items()}
    k1 = ref.rate(s["x"], s["u"], s["feet"], s["mass"], ref.inv(s["inertia"]))
    tau = np.einsum("bij,bj->bi", ref.ld(s["inertia"]), k1[:, 10:13])
    print("one-tick truncation error at 5 ms, walking set:", {g: f"{v:.2e}" for g, v in worst.items()},
          f"; net torque up to {float(np.abs(tau).max()):.1f} N m, angular acceleration up to {float(np.abs(k1[:, 10:13]).max()):.0f} rad/s^2")
    assert 1e-12 < min(worst.values()) and max(worst.values()) < 1.0


# ================================================================================================================================
# second half: the host build against the reference
# ================================================================================================================================
@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = tmp_path_factory.mktemp("plant_step_host") / "plant_step_host"
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-o", str(exe), str(SRC)], check=True)

    def call(rows):
        """rows: lists [op, array, array, ...]; returns one float64 array per row"""
        text = "\n".join(" ".join([r[0]] + [float(v).hex() for a in r[1:] for v in np.asarray(a, dtype=np.float64).ravel()]) for r in rows)
        out = subprocess.run([str(exe)], input=text + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        assert len(lines) == len(rows)
        return [np.array([float.fromhex(t) for t in l.split()]) for l in lines]

    return call


def _step_rows(s, ext, dt=DT):
    rows = []
    for i in range(len(s["x"])):
        r = ["stepx" if ext else "step", s["mass"][i], s["inertia"][i], dt, s["x"][i], s["u"][i], s["feet"][i]]
        rows.append(r + [s["f_ext"][i], s["tau_ext"][i]] if ext else r)
    return rows


def _group_units(got, want):
    e = ref.units(got, want).astype(np.float64)
    return {g: float(e[:, sl].max()) for g, sl in ref.GROUPS.items()}


@pytest.mark.parametrize("name", ["walking", "harsh"])
def test_plant_step_equals_the_reference(run, name):
    """plant_step on the walking set, plant_step_ext on the harsh set (and on the walking set, whose zero disturbance must give
    plant_step's bytes): every component within K_g 2^-52 max(1, |reference|)"""
    s = {"walking": walking, "harsh": harsh}[name](ROWS)
    got = np.array(run(_step_rows(s, ext=name == "harsh")))
    worst = _group_units(got, _reference_step(s))
    print(f"{name}: worst error per group in units of 2^-52 max(1, |ref|):", {g: round(v, 3) for g, v in worst.items()})
    for g, v in worst.items():
        assert v <= ref.K[g], (name, g, v)
    assert float(np.abs(np.sqrt((ref.ld(got[:, 3:7]) ** 2).sum(axis=1)) - 1).max()) <= 2 * 2.0 ** -52      # |q| = 1 within 2 ulp
    if name == "walking":
        assert np.array(run(_step_rows(s, ext=True))).tobytes() == got.tobytes()


def test_plant_step_edges(run):
    """zero disturbance with -0.0 components, all legs unloaded, yaw near +-pi, identity at rest, another dt"""
    s = walking(40)
    s["f_ext"][:, 0], s["tau_ext"][:, 1] = -0.0, -0.0                      # rows 0 .. 39: signed zeros add nothing
    s["u"][8:16] = 0.0                                                      # all legs unloaded: free fall
    s["u"][12:16, :, 0] = -0.0
    for i, yaw in enumerate((np.pi, -np.pi, np.nextafter(np.pi, 0), -np.nextafter(np.pi, 0), 3.1415, -3.1415, 3.0, -3.0)):
        s["x"][16 + i, 3:7] = [np.cos(yaw / 2), 0.0, 0.0, np.sin(yaw / 2)]
    s["x"][24:28, 3:7] = [1.0, 0.0, 0.0, 0.0]                               # identity
    s["x"][26:28, 7:13] = 0.0                                               # ... at rest
    s["x"][27, 7:13] = -0.0
    plain = np.array(run(_step_rows(s, ext=False)))
    extended = np.array(run(_step_rows(s, ext=True)))
    assert plain.tobytes() == extended.tobytes()
    want = _reference_step(s)
    for g, v in _group_units(plain, want).items():
        assert v <= ref.K[g], (g, v)
    assert (plain[8:16, 10:13] == s["x"][8:16, 10:13]).all()                # no force, no torque: w keeps its value
    half = np.array(run(_step_rows(s, ext=True, dt=0.0025)))
    for g, v in _group_units(half, _reference_step(s, 0.0025)).items():
        assert v <= ref.K[g], (g, v)


def _attitudes():
    """the quaternions of both sets, the edge attitudes beside them"""
    q = np.concatenate([walking(ROWS)["x"][:, 3:7], harsh(ROWS)["x"][:, 3:7]])
    edge = [[1.0, 0.0, 0.0, 0.0], [-1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0, -1.0]]
    for yaw in (np.pi, -np.pi, np.nextafter(np.pi, 0), -np.nextafter(np.pi, 0), 3.1415, -3.1415, 3.14159265, -3.14159265):
        edge.append([np.cos(yaw / 2), 0.0, 0.0, np.sin(yaw / 2)])
    return q, np.array(edge)


def test_quat_to_rot_and_the_products(run):
    q, edge = _attitudes()
    q = np.concatenate([q, edge])
    got = np.array(run([["rot", a] for a in q]))
    e = float(ref.units(got.reshape(-1, 3, 3), ref.rot(q)).max())
    f = np.concatenate([walking(ROWS)["u"][:, 0], harsh(ROWS)["u"][:, 0], np.full((len(edge), 3), 50.0)])
    both = np.array(run([["rotv", a, b] for a, b in zip(q, f)]))
    R = ref.rot(q)
    ef = float(ref.units_vec(both[:, 0:3], np.einsum("bij,bj->bi", R, f)).max())
    et = float(ref.units_vec(both[:, 3:6], np.einsum("bji,bj->bi", R, f)).max())
    print(f"quat_to_rot: worst {e:.3f}; R f: worst {ef:.3f}, R' f: worst {et:.3f} (units of 2^-52 max(1, |ref|))")
    assert e <= ref.K["rot"] and max(ef, et) <= ref.K["rot_product"]
    assert (got[-len(edge)] == np.eye(3).ravel()).all() and (got[-len(edge) + 1] == np.eye(3).ravel()).all()      # q and -q


def test_rot_to_rot_z(run):
    q, edge = _attitudes()
    q = np.concatenate([q, edge])
    R = np.array(run([["rot", a] for a in q]))
    got = np.array(run([["rotz", r] for r in R])).reshape(-1, 3, 3)
    want = ref.rot_z(R.reshape(-1, 3, 3))
    e = float(ref.units(got, want).max())
    print(f"rot_to_rot_z: worst {e:.3f}")
    assert e <= ref.K["rot_z"]
    assert (got[:, 2] == [0.0, 0.0, 1.0]).all() and (got[:, :, 2] == [0.0, 0.0, 1.0]).all()
    # and it is the yaw of the attitude: for a yaw-only quaternion, R itself
    assert float(np.abs(ref.ld(got[-8:]) - ref.rot(q[-8:])).max()) < 4 * 2.0 ** -52


def test_quat_to_euler(run):
    """roll / pitch / yaw on both sets (|pitch| <= 1 rad: asin is well conditioned) under the rule; at pitch = +-pi/2 the clamp:
    the pitch is +-pi/2 to the conditioning of asin at 1, sqrt(2 x 4 ulp), and exactly +-pi/2 where the sine rounds to 1 or above"""
    q, edge = _attitudes()
    q = np.concatenate([q, edge])
    got = np.array(run([["euler", a] for a in q]))
    e = float(ref.units(got, ref.euler(q)).max())
    print(f"quat_to_euler: worst {e:.3f}")
    assert e <= ref.K["euler"]
    # yaw-only attitudes near +-pi: the yaw itself comes back
    yaws = np.array([np.pi, -np.pi, np.nextafter(np.pi, 0), -np.nextafter(np.pi, 0), 3.1415, -3.1415, 3.14159265, -3.14159265])
    assert np.abs(got[-8:, 2] - yaws).max() <= 4 * 2.0 ** -52 * np.pi and (got[-8:, :2] == 0).all()
    # gimbal: pitch +-pi/2 exactly, with yaw on top, and sines that round beyond 1
    s = np.sqrt(0.5)
    up = np.nextafter(s, 1.0)
    gimbal = np.array([[s, 0.0, s, 0.0], [s, 0.0, -s, 0.0], [up, 0.0, up, 0.0], [up, 0.0, -up, 0.0], [-up, 0.0, -up, 0.0]])
    g = np.array(run([["euler", a] for a in gimbal]))
    assert np.isfinite(g).all()
    assert (np.abs(np.abs(g[:, 1]) - np.pi / 2) <= np.sqrt(2 * 4 * 2.0 ** -52)).all()
    assert (np.sign(g[:, 1]) == [1, -1, 1, -1, 1]).all()
    assert (g[2:, 1] == np.array([1, -1, 1]) * (np.pi / 2)).all()      # 2 w y = 1 + 4 ulp: clamped, not NaN


def test_inv3(run):
    """the cofactor inverse against the elimination in longdouble: B A = 1 within K 2^-52 cond(A), on the harsh set's skewed
    inertias and on badly scaled general matrices"""
    A = harsh(ROWS)["inertia"]
    G = _between(_uniform(20240503, 6, ROWS, 9), -1, 1).reshape(-1, 3, 3) * np.array([1e-3, 1.0, 50.0])[None, :, None]
    G += np.eye(3) * np.array([1e-3, 1.0, 50.0]) * 2
    A = np.concatenate([A, G])
    B = np.array(run([["inv", a] for a in A])).reshape(-1, 3, 3)
    want = ref.inv(A)
    cond = np.abs(ref.ld(A)).sum(axis=2).max(axis=1) * np.abs(want).sum(axis=2).max(axis=1)
    res = np.abs(ref.ld(B) @ ref.ld(A) - np.eye(3)).max(axis=(1, 2)) / (ref.U * cond)
    print(f"inv3: worst residual {float(res.max()):.3f} in units of 2^-52 cond; cond up to {float(cond.max()):.1f}")
    assert float(res.max()) <= ref.K["inv"]
    assert float((np.abs(ref.ld(B) - want).max(axis=(1, 2)) / (ref.U * cond * np.abs(want).max(axis=(1, 2)))).max()) <= ref.K["inv"]


# ---- the push wrench ------------------------------------------------------------------------------------------------------------
PUSH_DTYPE = np.dtype([("start_tick", "<f8"), ("ticks", "<f8"), ("force_world", "<f8", (3,)), ("torque_body", "<f8", (3,))])


def _push_cases(n, seed=20240504):
    """n robots x 4 windows around tick t: starts t - 3 .. t + 1 (so: at the tick itself, before, after), lengths -2 .. 4 (so:
    never, ending AT t -- exclusive --, covering t), some fractional; components zero (either sign) in a third of the places; a
    constant disturbance on two robots of three, with zeros of both signs"""
    u = _uniform(seed, 7, n, 48)
    t = np.floor(_between(u[:, 0], 0, 50))
    push = np.zeros((n, 4), dtype=PUSH_DTYPE)
    for k in range(4):
        c = u[:, 1 + 10 * k: 11 + 10 * k]
        push["start_tick"][:, k] = t + np.floor(_between(c[:, 0], -3, 2))
        push["ticks"][:, k] = np.floor(_between(c[:, 1], -2, 5))
        frac = c[:, 2] < 0.2
        push["ticks"][frac, k] += 0.5
        push["start_tick"][frac, k] -= 0.25
        w = _between(c[:, 3:9], -1, 1) * np.array([60.0, 60.0, 60.0, 3.0, 3.0, 3.0])
        w[np.abs(w) < np.array([20.0] * 3 + [1.0] * 3)] = 0.0
        w[(w == 0) & (c[:, 3:9] < 0.5)] = -0.0
        push["force_world"][:, k], push["torque_body"][:, k] = w[:, :3], w[:, 3:]
    const = _between(u[:, 41:47], -1, 1) * np.array([15.0, 15.0, 15.0, 1.0, 1.0, 1.0])
    const[::3] = 0.0
    const[1::6, 0] = -0.0
    const[4::6, 5] = -0.0
    return t, push, const[:, :3].copy(), const[:, 3:].copy()


def test_loop_push_wrench(run, pkg):
    assert PUSH_DTYPE == pkg.PUSH_PARAMS_DTYPE
    n = ROWS
    t, push, f0, t0 = _push_cases(n)
    # hand-made rows: the boundaries of a window [10, 13) beside an overlapping one [12, 20) and a constant disturbance
    hand_t = np.array([9.0, 10.0, 11.0, 12.0, 13.0, 19.0, 20.0, 12.0])
    hp = np.zeros((len(hand_t), 4), dtype=PUSH_DTYPE)
    hp["start_tick"][:, 0], hp["ticks"][:, 0], hp["force_world"][:, 0] = 10.0, 3.0, [30.0, 0.0, -0.0]
    hp["start_tick"][:, 1], hp["ticks"][:, 1], hp["force_world"][:, 1], hp["torque_body"][:, 1] = 12.0, 8.0, [0.1, -7.0, 0.0], [0.0, 0.0, 1.5]
    hp["start_tick"][:, 2], hp["ticks"][:, 2], hp["force_world"][:, 2] = 12.0, 0.0, [1e3, 1e3, 1e3]          # ticks = 0: never
    hp["start_tick"][:, 3], hp["ticks"][:, 3], hp["torque_body"][:, 3] = 12.0, -5.0, [9.0, 9.0, 9.0]         # ticks < 0: never
    hf, ht = np.tile([0.3, 0.0, -0.0], (len(hand_t), 1)), np.tile([-0.0, 0.2, 0.0], (len(hand_t), 1))
    hf[-1], ht[-1] = 0.0, 0.0
    t, push, f0, t0 = np.concatenate([t, hand_t]), np.concatenate([push, hp]), np.concatenate([f0, hf]), np.concatenate([t0, ht])
    rows = [["push", push.shape[1], t[i], f0[i], t0[i]] + [v for w in push[i] for v in (w["start_tick"], w["ticks"], w["force_world"], w["torque_body"])]
            for i in range(len(t))]
    got = np.array(run(rows))
    wf, wt, active = ref.effective_wrench(f0, t0, push, t)
    assert [int(a) for a in active[n:]] == [0, 1, 1, 2, 1, 1, 0, 2]      # start inclusive, end exclusive, ticks <= 0 never
    assert (active == 0).sum() > n // 20 and (active >= 2).sum() > n // 10 and (push["start_tick"] == t[:, None]).sum() > n // 4
    assert ((push["start_tick"] + push["ticks"] == t[:, None]) & (push["ticks"] > 0)).sum() > n // 20      # windows ending AT t
    # values: the reference's sum within one rounding per added window
    act = (push["ticks"] > 0) & (t[:, None] >= push["start_tick"]) & (t[:, None] < push["start_tick"] + push["ticks"])
    for got_c, want_c, const, field in ((got[:, :3], wf, f0, "force_world"), (got[:, 3:], wt, t0, "torque_body")):
        terms = push[field] * act[:, :, None]
        added = (terms != 0).sum(axis=1)
        size = np.abs(const) + np.abs(terms).sum(axis=1)
        assert (np.abs(ref.ld(got_c) - want_c) <= added * 2.0 ** -53 * size).all(), field
        untouched = added == 0
        assert untouched.sum() > n // 4
        assert got_c[untouched].tobytes() == const[untouched].tobytes(), field      # -0.0 stays -0.0
        # an exactly zero running value is REPLACED: one active window alone gives its bytes
        alone = (added == 1) & (const == 0)
        only = terms.sum(axis=1)
        assert alone.sum() > n // 20 and got_c[alone].tobytes() == only[alone].tobytes(), field
