"""Input sets of the body-rate tests (tests/test_motion_sets_cpu.py, tests/test_gpu_motion_sets.py,
tests/golden/make_motion_fixtures.py): body rates of 1 ... 12 rad/s and body speeds up to 3 m/s, FED to the problem -- where the
default parameters drop the measured angular velocity (drop_ang_vel = 1, the reference's x_init) and the state generators draw
it at sigma = 0.5 rad/s and the velocity at sigma = 0.3 m/s.  Not a test module.

The rate enters through the quaternion kinematics qdot = Omega(w) q / 2: the attitude blocks of the linearisation, the knot
expansions and the trial rollouts, all near zero over the whole horizon while w0 = 0.  The body velocity multiplies the
attitude-dependent block of dp = R(q) v.  quat, rot, feet, contacts and references stay as the generator draws them;
ang_vel_body is replaced by sense rate axis (axis in the body frame) and lin_vel_body rescaled to the speed class, its
direction kept.  Every parameter object of these sets comes from params() below: drop_ang_vel = 0.

The CPU suite and the GPU suite build their records here, so both see the same ones."""
import numpy as np

from stance_sets import copies_identical, plain_plan, swing_rows, tiled  # noqa: F401  (the tests take them from here)

RATES = (1.0, 2.0, 4.0, 8.0, 12.0)          # rad/s
AXES = ("yaw", "body x", "body y", "random")
SPEEDS = (None, 1.0, 3.0)                   # m/s; None: as the generator draws it (sigma = 0.3 m/s per component)
GRID = 8 * len(RATES) * len(SPEEDS)         # 120 records hold one of every (speed, rate, axis, sense) cell
_SEED = 0x3A7E


def params(src, default, N, mode=0, *lib):
    """The parameter object of these sets: getattr(src, default)(N, mode[, lib]) of the package or of the oracle with
    drop_ang_vel = 0.  The one place the tests take parameters from, so none can run with the rate dropped by oversight."""
    p = getattr(src, default)(N, mode, *lib)
    p.drop_ang_vel = 0
    return p


def cell(k):
    """(rate, axis kind, sense, speed class) of record k: from k alone.  The sense alternates, the axis kind changes every
    second, the rate every eighth and the speed class every 40th record, so the first 120 records hold one of every cell and
    every whole multiple as many of each."""
    k = np.asarray(k)
    return np.asarray(RATES)[(k // 8) % len(RATES)], (k // 2) % 4, 1.0 - 2.0 * (k % 2), (k // 40) % len(SPEEDS)


def _axes(kind):
    """unit axes in the body frame; the random ones from a fixed seed, axis k the same whatever the size of the set"""
    n = len(kind)
    ax = np.random.default_rng(_SEED).standard_normal((4096, 3))[:n]
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    for j, e in enumerate(((0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0))):
        ax[kind == j] = e
    return ax


def with_motion(rec, shift=0):
    """A copy of rec with ang_vel_body = sense_k rate_k axis_k and |lin_vel_body| set to the speed class of record k; `shift`
    moves every record to the neighbouring rate of the grid (the last one down, the others up)"""
    rec = rec.copy()
    k = np.arange(len(rec))
    rate, kind, sense, speed = cell(k)
    if shift:
        i = (k // 8) % len(RATES)
        rate = np.asarray(RATES)[np.where(i + 1 < len(RATES), i + 1, i - 1)]
    rec["ang_vel_body"] = (sense * rate)[:, None] * _axes(kind)
    for c, v in enumerate(SPEEDS):
        if v is not None:
            m = speed == c
            rec["lin_vel_body"][m] *= (v / np.linalg.norm(rec["lin_vel_body"][m], axis=1))[:, None]
    return rec


def grid_rate(rec):
    """[B] the grid rate nearest to |ang_vel_body|: what the tests group and print by"""
    a = np.asarray(RATES)
    return a[np.abs(np.linalg.norm(rec["ang_vel_body"], axis=1)[:, None] - a[None, :]).argmin(axis=1)]


def quat(pkg, N):
    """QuatMpc records: 360, three of every (speed, rate, axis, sense) cell; N = 20 from config 3, N = 5, 10 from config 2"""
    return with_motion(pkg.random_go1_trot_states(3 * GRID, config_id=3 if N == 20 else 2))


def biped8(pkg, N=16):
    """Records of the 8-point model: 240, two of every cell"""
    return with_motion(pkg.random_biped8_states(2 * GRID, config_id=5))


def variants(pkg, p):
    """Per-instance records for quat(pkg, 10): a robot of its own per instance (pkg.random_go1_variants around `p`: mass,
    inertia, friction, force bound, Q and R).  The CPU oracle, solved per record with that record's parameters, converges on
    every one (tests/test_motion_sets_cpu.py holds that and has the measured iteration counts)."""
    return pkg.random_go1_variants(3 * GRID, seed=23, base=p)


# the robots of the closed-loop test: (axis kind, initial body rate in rad/s); two start at rest
LOOP_RATES = (("yaw", 2.0), ("yaw", 4.0), ("yaw", 8.0), ("random", 2.0), ("random", 4.0), ("random", 8.0), (None, 0.0), (None, 0.0))
LOOP_YAWS = (0.0, 0.4, -1.0, 2.0, 0.7, -0.3, 0.0, 1.3)


def loop_states(pkg, lib, lp):
    """Eight standing robots of the device closed loop (pkg.loop_states, stand mode, 0.3 m) that start with the body rates
    LOOP_RATES about the body's z and about a random body axis, senses alternating; attitude, feet and references at rest."""
    cmds = [[0.0, 0.0, 0.30, 0.0, 0.0, 0.0, 0.0]] * len(LOOP_RATES)
    st = pkg.loop_states(cmds, lp, height=0.3, yaw=LOOP_YAWS, lib=lib)
    axes = _axes(np.array([0 if kind == "yaw" else 3 for kind, _ in LOOP_RATES]))
    for i, (kind, rate) in enumerate(LOOP_RATES):
        st["ang_vel_body"][i] = (1.0 - 2.0 * (i % 2)) * rate * axes[i]
    return st


def warm_pairs(pkg, N, rate_max=None):
    """(first tick, second tick) of a warm start: the first tick is quat(pkg, N); the second has the body rate at the
    neighbouring rate of the grid (the next one up; from the last one down), lin_vel_body + 0.02, and on every third record the
    stance set mirrored left to right (FL <-> FR, RL <-> RR: the trot diagonals change places, so two legs land and two lift
    off).  rate_max: only the records whose two ticks both stay at or below it."""
    base = pkg.random_go1_trot_states(3 * GRID, config_id=3 if N == 20 else 2)
    first, second = with_motion(base), with_motion(base, shift=1)
    second["lin_vel_body"] += 0.02
    second["contacts"][::3] = second["contacts"][::3][:, [1, 0, 3, 2]]
    if rate_max is not None:
        keep = np.maximum(grid_rate(first), grid_rate(second)) <= rate_max
        first, second = first[keep], second[keep]
    return first, second
