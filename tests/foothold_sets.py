"""Input sets of the foothold tests (tests/test_foothold_sets_cpu.py, tests/test_gpu_foothold_sets.py,
tests/golden/make_foothold_fixtures.py): footholds and position / velocity / acceleration references far from nominal -- where
the state generators place every foot within 5 cm of the nominal 40 x 28 cm rectangle at z = -0.30 m (the 8-point model within
3 cm of two fixed foot centres), draw pos_ref_body at sigma = 2 cm and vel_ref_body within 0.5 / 0.1 m/s with z = 0, and leave
acc_ref_body at 0.  Not a test module.

The foot positions are the operand of the wrench map, of G = sum V D^-1 V', of the two 6 x 6 factorisations per knot, of the B
blocks of the linearisation and of the lever-arm terms of every rollout; the references enter the cost gradient of every knot,
and with acc_ref = 0 the quadratic term of the reference trajectory is dead code.  Quaternion, rotation, velocities and contacts
stay as the generator draws them; the feet are replaced by the foothold kind of the record and one reference field is moved by
its reference class.  j below is the generator's own jitter, foot - NOMINAL_FEET.

The CPU suite and the GPU suite build their records here, so both see the same ones."""
import numpy as np

from stance_sets import copies_identical, plain_plan, swing_rows, tiled  # noqa: F401  (the tests take them from here)

KINDS = ("bunched", "stretched", "narrow", "short", "ahead", "aside", "uneven", "crossed", "crouched", "tall")
CLASSES = ("as drawn", "pos_ref + 0.3 u", "vel_ref + 3 u", "acc_ref + 5 u")
GRID = len(KINDS) * len(CLASSES)            # 40 records hold one of every (kind, class) cell
# QuatMpc at N = 20: the CPU oracle leaves its envelope at the full displacements (aside + 0.25: 90 MAX_ITER and 6 NOT_PD of
# 96; crossed: 5 of 320 MAX_ITER; ahead + 0.30: up to 104 iterations), so `ahead` is + 0.10, `aside` + 0.05, `crossed` left out
AHEAD, ASIDE = {False: 0.30, True: 0.10}, {False: 0.25, True: 0.05}
KINDS8 = ("as drawn", "tandem", "wide", "close", "step", "ahead", "aside")
GRID8 = len(KINDS8) * len(CLASSES)          # 28
UNEVEN = (0.12, -0.12, -0.12, 0.12)
_SEED = 0xF007


def cell(k):
    """(foothold kind, reference class) of record k: from k alone.  The kind changes with every record, the class every
    tenth, so the first 40 records hold one of every cell and every whole multiple as many of each."""
    k = np.asarray(k)
    return k % len(KINDS), (k // len(KINDS)) % len(CLASSES)


def cell8(k):
    """the same for the 8-point model: kind k % 7, class (k // 7) % 4; the first 28 records hold one of every cell"""
    k = np.asarray(k)
    return k % len(KINDS8), (k // len(KINDS8)) % len(CLASSES)


def units(n):
    """[n, 3] unit vectors u, z included; from a fixed seed, u_k the same whatever the size of the set"""
    u = np.random.default_rng(_SEED).standard_normal((4096, 3))[:n]
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def _nominal(pkg):
    return pkg.scenarios.NOMINAL_FEET


def displaced(pkg, feet, kind, n20=False):
    """[B, 4, 3] feet of the foothold kinds `kind` [B] from the generator's feet [B, 4, 3] (body or yaw-aligned frame)"""
    nom = _nominal(pkg)
    j = feet - nom[None]
    out = feet.copy()
    side = np.sign(nom)                                      # [4, 3]
    for c, name in enumerate(KINDS):
        m = kind == c
        if not m.any():
            continue
        if name == "bunched":
            out[m] = nom * (0.25, 0.25, 1.0) + 0.2 * j[m]
        elif name == "stretched":
            out[m] = nom * (2.0, 2.0, 1.0) + j[m]
        elif name == "narrow":
            out[m, :, 1] = 0.005 * side[None, :, 1] + 0.1 * j[m, :, 1]
        elif name == "short":
            out[m, :, 0] = 0.005 * side[None, :, 0] + 0.1 * j[m, :, 0]
        elif name == "ahead":
            out[m, :, 0] += AHEAD[n20]
        elif name == "aside":
            out[m, :, 1] += ASIDE[n20]
        elif name == "uneven":
            out[m, :, 2] += np.asarray(UNEVEN)[None]
        elif name == "crossed":
            out[m] = feet[m][:, [1, 0, 2, 3]]
        elif name == "crouched":
            out[m, :, 2] = -0.08 + j[m, :, 2]
        elif name == "tall":
            out[m, :, 2] = -0.60 + j[m, :, 2]
    return out


def with_footholds(pkg, rec, n20=False, kind=None):
    """A copy of Go1 records with foot_pos_body on the foothold kind of record k (or on `kind` [B])"""
    rec = rec.copy()
    B = len(rec)
    kind = cell(np.arange(B))[0] if kind is None else kind
    rec["foot_pos_body"] = displaced(pkg, rec["foot_pos_body"].reshape(B, 4, 3), kind, n20).reshape(B, 12)
    return rec


def with_references(rec, cls):
    """A copy with the field of each record's reference class `cls` [B] moved: pos_ref_body += 0.3 u, vel_ref_body += 3 u,
    acc_ref_body += 5 u (class 0: as drawn)"""
    rec = rec.copy()
    u = units(len(rec))
    for c, (name, scale) in enumerate((("pos_ref_body", 0.3), ("vel_ref_body", 3.0), ("acc_ref_body", 5.0)), start=1):
        rec[name][cls == c] += scale * u[cls == c]
    return rec


def _next_kind(kind, n20):
    """the next kind of the grid (N = 20: of its reduced grid)"""
    nxt = (kind + 1) % len(KINDS)
    if n20:
        nxt = np.where(nxt == KINDS.index("crossed"), (nxt + 1) % len(KINDS), nxt)
    return nxt


def _base(pkg, N):
    return pkg.random_go1_trot_states(8 * GRID, config_id=3 if N == 20 else 2)


def _reduce(rec, N):
    """N = 20: the 288 records of the reduced grid (`crossed` left out)"""
    if N != 20:
        return rec
    return rec[cell(np.arange(len(rec)))[0] != KINDS.index("crossed")]


def quat(pkg, N, footholds=True, references=True):
    """QuatMpc records: 320, eight of every (kind, class) cell; N = 20 from config 3 with its reduced grid (288 records: ahead
    + 0.10, aside + 0.05, crossed left out; the first 36 hold one of every cell), N = 5, 10 from config 2.
    footholds=False / references=False: the same records on the generator's feet / references (what the `really fed` checks
    compare with)."""
    rec = _base(pkg, N)
    if footholds:
        rec = with_footholds(pkg, rec, N == 20)
    if references:
        rec = with_references(rec, cell(np.arange(len(rec)))[1])
    return _reduce(rec, N)


def cells(model, N):
    """(kind [B], class [B]) of the records of quat(pkg, N) (model "quat"), convex(pkg, N) ("convex") or biped8(pkg) ("biped8")"""
    if model == "biped8":
        return cell8(np.arange(8 * GRID8))
    kind, cls = cell(np.arange(8 * GRID))
    if model == "quat" and N == 20:
        keep = kind != KINDS.index("crossed")
        kind, cls = kind[keep], cls[keep]
    return kind, cls


def _rz(yaw, v, inverse=False):
    c, s = np.cos(yaw)[:, None], np.sin(yaw)[:, None] * (-1.0 if inverse else 1.0)
    out = v.copy()
    out[..., 0] = c * v[..., 0] - s * v[..., 1]
    out[..., 1] = s * v[..., 0] + c * v[..., 1]
    return out


def convex(pkg, N, footholds=True, references=True):
    """ConvexMpc records: 320 (config 12 at N = 10, 13 at N = 20), the same kinds applied in the yaw-aligned frame and rotated
    back into foot_pos_abs_com (the full displacements at both horizons: the oracle converges on all of them); classes
    pos_d_world += 0.3 u, lin_vel_d_world += 3 u, yaw_rate_d += 3 u_x."""
    rec = pkg.random_go1_convex_states(8 * GRID, config_id=13 if N == 20 else 12).copy()
    B = len(rec)
    kind, cls = cell(np.arange(B))
    if footholds:
        yaw = rec["euler"][:, 2]
        feet = _rz(yaw, rec["foot_pos_abs_com"].reshape(B, 4, 3), inverse=True)
        rec["foot_pos_abs_com"] = _rz(yaw, displaced(pkg, feet, kind)).reshape(B, 12)
    if references:
        u = units(B)
        rec["pos_d_world"][cls == 1] += 0.3 * u[cls == 1]
        rec["lin_vel_d_world"][cls == 2] += 3.0 * u[cls == 2]
        rec["yaw_rate_d"][cls == 3] += 3.0 * u[cls == 3, 0]
    return rec


def biped8(pkg, N=16, footholds=True, references=True):
    """Records of the 8-point model: 224, eight of every (kind, class) cell of KINDS8 x CLASSES (points 0-3 left foot, 4-7
    right): as drawn; tandem -- both feet on the body's x axis, the left 0.15 m ahead and the right 0.15 m behind; wide -- each
    foot 0.25 m further out; close -- each 4.5 cm inwards (nominal foot edges 1 cm apart); step -- left foot 0.2 m higher;
    ahead + 0.15; aside + 0.10.  The CPU oracle converges on every cell of the product with the reference classes at these
    displacements (tests/test_foothold_sets_cpu.py has the counts), so none was shrunk."""
    rec = pkg.random_biped8_states(8 * GRID8, config_id=5).copy()
    B = len(rec)
    kind, cls = cell8(np.arange(B))
    if footholds:
        f = rec["foot_pos_body"].reshape(B, 8, 3).copy()
        out = np.array([1.0] * 4 + [-1.0] * 4)                          # +y is outwards for the left foot
        m = kind == KINDS8.index("tandem")
        f[m, :, 1] -= 0.1 * out[None]
        f[m, :, 0] += 0.15 * out[None]
        f[kind == KINDS8.index("wide"), :, 1] += 0.25 * out[None]
        f[kind == KINDS8.index("close"), :, 1] -= 0.045 * out[None]
        m = kind == KINDS8.index("step")
        f[m, :4, 2] += 0.2
        f[kind == KINDS8.index("ahead"), :, 0] += 0.15
        f[kind == KINDS8.index("aside"), :, 1] += 0.10
        rec["foot_pos_body"] = f.reshape(B, 24)
    if references:
        rec = with_references(rec, cls)
    return rec


def variants(pkg, p):
    """Per-instance records for quat(pkg, 10): a robot of its own per instance (pkg.random_go1_variants around `p`: mass,
    inertia, friction, force bound, Q and R).  The CPU oracle, solved per record with that record's parameters, converges on
    every one (tests/test_foothold_sets_cpu.py holds that and has the measured iteration counts)."""
    return pkg.random_go1_variants(8 * GRID, seed=29, base=p)


def convex_variants(pkg, p):
    """the same for convex(pkg, 10) (pkg.random_go1_convex_variants)"""
    return pkg.random_go1_convex_variants(8 * GRID, seed=29, base=p)


def warm_pairs(pkg, N):
    """(first tick, second tick) of a warm start: the first tick is quat(pkg, N); the second is the same record one controller
    tick (5 ms) later -- every foot moved by -0.005 lin_vel_body, lin_vel_body + 0.02 -- and on every third record the trot
    diagonals change over (FL <-> FR, RL <-> RR) AND the legs that land take the footholds of the next kind of the grid: a
    landed leg stands somewhere else, and the previous trajectory was solved for another geometry."""
    base = _base(pkg, N)
    n20 = N == 20
    first = quat(pkg, N)
    kind = cell(np.arange(len(base)))[0]
    nxt = _reduce(with_footholds(pkg, base, n20, kind=_next_kind(kind, n20)), N)
    second = first.copy()
    B = len(second)
    second["contacts"][::3] = second["contacts"][::3][:, [1, 0, 3, 2]]
    landed = (second["contacts"] == 1) & (first["contacts"] == 0)
    feet = second["foot_pos_body"].reshape(B, 4, 3).copy()
    feet[landed] = nxt["foot_pos_body"].reshape(B, 4, 3)[landed]
    feet -= 0.005 * first["lin_vel_body"][:, None, :]
    second["foot_pos_body"] = feet.reshape(B, 12)
    second["lin_vel_body"] += 0.02
    return first, second


# the robots of the closed-loop test: displacement of the standing feet in the yaw-aligned frame; two stay nominal.  All feet
# stay on the ground (z = 0), so there is no uneven kind here.
LOOP_KINDS = ("bunched", "stretched", "narrow", "short", "ahead +0.10", "aside +0.05", None, None)
LOOP_YAWS = (0.0, 0.4, -1.0, 2.0, 0.7, -0.3, 0.0, 1.3)


def loop_states(pkg, lib, lp):
    """Eight standing robots of the device closed loop (pkg.loop_states, stand mode, 0.3 m) whose foot_pos_world is displaced to
    LOOP_KINDS (in the yaw-aligned frame about the robot's position, no jitter: the default footholds are the nominal ones);
    attitude, velocities and references at rest."""
    cmds = [[0.0, 0.0, 0.30, 0.0, 0.0, 0.0, 0.0]] * len(LOOP_KINDS)
    st = pkg.loop_states(cmds, lp, height=0.3, yaw=LOOP_YAWS, lib=lib)
    B = len(st)
    yaw = np.asarray(LOOP_YAWS)
    pos = st["pos_world"][:, None, :]
    feet = _rz(yaw, st["foot_pos_world"].reshape(B, 4, 3) - pos, inverse=True)
    kind = np.array([-1 if k is None else KINDS.index(k.split()[0]) for k in LOOP_KINDS])
    feet = displaced(pkg, feet, kind, n20=True)             # (the milder ahead / aside)
    st["foot_pos_world"] = (_rz(yaw, feet) + pos).reshape(B, 12)
    return st


def first_tick_inputs(pkg, st):
    """qmpc_input records of the first tick of standing robots at rest, built in numpy from the loop states alone:
    foot_pos_body = R'(foot_pos_world - pos_world), quat_d = quat, all feet in contact, velocities and references 0"""
    B = len(st)
    rec = np.zeros(B, dtype=pkg.INPUT_DTYPE)
    R = pkg.quat_to_rot(st["quat"]).reshape(B, 3, 3)
    rec["quat"], rec["quat_d"], rec["rot"] = st["quat"], st["quat_d"], R.reshape(B, 9)
    d = st["foot_pos_world"].reshape(B, 4, 3) - st["pos_world"][:, None, :]
    rec["foot_pos_body"] = np.einsum("bji,blj->bli", R, d).reshape(B, 12)
    rec["contacts"] = 1.0
    return rec
