"""quaternion-mpc_amd -- MI355X-native batched quaternion-MPC inner loop.

Python is plumbing only (tests, bench, multi-GPU launch): the product is the
C-ABI shared library ``csrc/libqmpc_hip.so`` declared in ``include/qmpc.h`` and
the C++ host class in ``host/``.  This module mirrors the C records with ctypes
and loads the library.  There is NO CPU fallback: if the HIP library is
missing or no GPU is visible, calls fail loudly.

The directory name contains a hyphen, so load it with
``importlib`` (see ``tests/conftest.py`` / ``__graft_entry__.py``) under the
module name ``quaternion_mpc_amd``.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

PKG_DIR = Path(__file__).resolve().parent
REPO_DIR = PKG_DIR.parent
LIB_PATH = PKG_DIR / "csrc" / "libqmpc_hip.so"

NX, NE, NU, NLEG, NC = 13, 12, 12, 4, 24

# status codes (include/qmpc.h)
OK, MAX_ITER, NO_CONTACT, NAN_INPUT, LINESEARCH_FAIL, NOT_PD, BAD_PARAMS = 0, 1, 2, 3, 4, 5, 6
BAD_ARGUMENT, NO_DEVICE, HIP_ERROR, BATCH_TOO_LARGE, UNSUPPORTED = 16, 17, 18, 19, 20
MODE_CONVERGED, MODE_REFERENCE = 0, 1
MODEL_QUAT, MODEL_CONVEX, MODEL_QUAT8 = 0, 1, 2


class Params(C.Structure):
    """struct qmpc_params (include/qmpc.h)."""

    _fields_ = [
        ("horizon", C.c_int32),
        ("h", C.c_float),
        ("h_ref", C.c_double),
        ("mass", C.c_double),
        ("inertia", C.c_double * 9),
        ("q_weights", C.c_double * 13),
        ("r_weights", C.c_double * 12),
        ("w", C.c_double),
        ("mu", C.c_double),
        ("fz_max", C.c_double),
        ("mode", C.c_int32),
        ("iterations_max", C.c_int32),
        ("penalty_initial", C.c_double),
        ("penalty_scaling", C.c_double),
        ("penalty_max", C.c_double),
        ("tol_stationarity", C.c_double),
        ("tol_feasibility", C.c_double),
        ("tol_cost_intermediate", C.c_double),
        ("tol_step", C.c_double),
        ("ipm_mu0", C.c_double),
        ("ipm_mu_final", C.c_double),
        ("ipm_sigma", C.c_double),
        ("ipm_sigma_fast", C.c_double),
        ("ipm_tau", C.c_double),
        ("linesearch_max", C.c_int32),
        ("drop_ang_vel", C.c_int32),
        ("model", C.c_int32),
    ]

    def copy(self) -> "Params":
        out = Params()
        C.memmove(C.byref(out), C.byref(self), C.sizeof(Params))
        return out


class LegGeometry(C.Structure):
    """struct qmpc_leg_geometry: the reference's rho_fix / rho_opt per leg (BaseInterface.cpp:10-34)."""

    _fields_ = [("rho_fix", (C.c_double * 5) * 4), ("rho_opt", (C.c_double * 3) * 4)]


# struct qmpc_input as a numpy structured dtype: 48 doubles, 384 B
INPUT_DTYPE = np.dtype(
    [
        ("quat", "<f8", (4,)),
        ("rot", "<f8", (9,)),
        ("lin_vel_body", "<f8", (3,)),
        ("ang_vel_body", "<f8", (3,)),
        ("foot_pos_body", "<f8", (12,)),
        ("contacts", "<f8", (4,)),
        ("pos_ref_body", "<f8", (3,)),
        ("vel_ref_body", "<f8", (3,)),
        ("acc_ref_body", "<f8", (3,)),
        ("quat_d", "<f8", (4,)),
    ],
    align=False,
)
assert INPUT_DTYPE.itemsize == 48 * 8

# struct qmpc_input8 (8 contact points, BASELINE config 5): 64 doubles, 512 B
INPUT8_DTYPE = np.dtype(
    [
        ("quat", "<f8", (4,)),
        ("rot", "<f8", (9,)),
        ("lin_vel_body", "<f8", (3,)),
        ("ang_vel_body", "<f8", (3,)),
        ("foot_pos_body", "<f8", (24,)),
        ("contacts", "<f8", (8,)),
        ("pos_ref_body", "<f8", (3,)),
        ("vel_ref_body", "<f8", (3,)),
        ("acc_ref_body", "<f8", (3,)),
        ("quat_d", "<f8", (4,)),
    ],
    align=False,
)
assert INPUT8_DTYPE.itemsize == 64 * 8

# struct qmpc_convex_input (ConvexMpc.cpp:81-198): 48 doubles, 384 B
CONVEX_INPUT_DTYPE = np.dtype(
    [
        ("euler", "<f8", (3,)),
        ("pos_world", "<f8", (3,)),
        ("ang_vel_world", "<f8", (3,)),
        ("lin_vel_world", "<f8", (3,)),
        ("foot_pos_abs_com", "<f8", (12,)),
        ("contacts", "<f8", (4,)),
        ("pos_d_world", "<f8", (3,)),
        ("lin_vel_d_world", "<f8", (3,)),
        ("yaw_rate_d", "<f8"),
        ("reserved", "<f8", (13,)),
    ],
    align=False,
)
assert CONVEX_INPUT_DTYPE.itemsize == 48 * 8

# ---- device-resident closed loop (include/qmpc.h: qmpc_loop_*), 820 doubles per instance ----
LOOP_WINDOW = 100
LOOP_FILTER_DTYPE = np.dtype([("ring", "<f8", (LOOP_WINDOW,)), ("head", "<f8"), ("count", "<f8"), ("sum", "<f8"),
                              ("correction", "<f8")], align=False)
LOOP_LEG_DTYPE = np.dtype([("gait_phase", "<f8"), ("state", "<f8"), ("pattern_index", "<f8"), ("prev_pattern_index", "<f8"),
                           ("start_time", "<f8"), ("end_time", "<f8"), ("not_first_call", "<f8"),
                           ("swing_start", "<f8", (3,)), ("swing_end", "<f8", (3,)), ("swing_extend", "<f8", (3,)),
                           ("fsm_pos", "<f8", (3,)), ("fsm_vel", "<f8", (3,)), ("fsm_acc", "<f8", (3,)),
                           ("terrain_height", "<f8")], align=False)
LOOP_STATE_DTYPE = np.dtype([
    ("pos_world", "<f8", (3,)), ("quat", "<f8", (4,)), ("lin_vel_world", "<f8", (3,)), ("ang_vel_body", "<f8", (3,)),
    ("foot_pos_world", "<f8", (12,)),
    ("joy", "<f8", (6,)), ("movement_mode", "<f8"), ("sin_ang_vel", "<f8"), ("attitude_traj_count", "<f8"),
    ("pos_d_world", "<f8", (3,)), ("pos_d_init", "<f8"), ("quat_d", "<f8", (4,)), ("lin_vel_d_rel", "<f8", (3,)),
    ("vel_filter", LOOP_FILTER_DTYPE, (3,)), ("pos_filter", LOOP_FILTER_DTYPE, (3,)),
    ("leg", LOOP_LEG_DTYPE, (4,)),
    ("contacts", "<f8", (4,)), ("gait_counter", "<f8", (4,)), ("forces_body", "<f8", (12,)), ("grf_world", "<f8", (12,)),
    ("foot_target_world", "<f8", (12,)), ("status", "<f8"), ("iterations", "<f8"), ("tick", "<f8")], align=False)
assert LOOP_STATE_DTYPE.itemsize == 820 * 8


# BaseInterface::tau_ctrl_update records (include/qmpc.h: qmpc_joint_feedback / qmpc_joint_command)
JOINT_FEEDBACK_DTYPE = np.dtype([
    ("joint_pos", "<f8", (12,)), ("joint_vel", "<f8", (12,)), ("torso_pos_world", "<f8", (3,)), ("torso_quat", "<f8", (4,)),
    ("torso_lin_vel_world", "<f8", (3,)), ("foot_pos_target_world", "<f8", (12,)), ("foot_vel_target_world", "<f8", (12,)),
    ("forces_body", "<f8", (12,)), ("plan_contacts", "<f8", (4,)), ("movement_mode", "<f8")])
JOINT_COMMAND_DTYPE = np.dtype([("joint_ang_tgt", "<f8", (12,)), ("joint_vel_tgt", "<f8", (12,)),
                                ("joint_tau_tgt", "<f8", (12,))])
assert JOINT_FEEDBACK_DTYPE.itemsize == 75 * 8 and JOINT_COMMAND_DTYPE.itemsize == 36 * 8


class LoopParams(C.Structure):
    """struct qmpc_loop_params."""

    _fields_ = [("gait_freq", C.c_double), ("default_foot_pos_rel", C.c_double * 12), ("dt", C.c_double),
                ("contact_height", C.c_double), ("warm_start", C.c_double)]


# struct qmpc_instance_params (qmpc_solve_instances*): one instance's robot and cost weights, 38 doubles = 304 B
INSTANCE_PARAMS_DTYPE = np.dtype(
    [
        ("mass", "<f8"),
        ("inertia", "<f8", (9,)),
        ("mu", "<f8"),
        ("fz_max", "<f8"),
        ("q_weights", "<f8", (13,)),
        ("r_weights", "<f8", (12,)),
        ("w", "<f8"),
    ],
    align=False,
)
assert INSTANCE_PARAMS_DTYPE.itemsize == 38 * 8


def instance_params(params: "Params", batch: int = 1) -> np.ndarray:
    """[batch] per-instance records all carrying the seven fields of `params` (edit fields per instance afterwards)."""
    out = np.zeros(int(batch), dtype=INSTANCE_PARAMS_DTYPE)
    out["mass"] = params.mass
    out["inertia"] = np.asarray(params.inertia[:], dtype=np.float64)
    out["mu"] = params.mu
    out["fz_max"] = params.fz_max
    out["q_weights"] = np.asarray(params.q_weights[:], dtype=np.float64)
    out["r_weights"] = np.asarray(params.r_weights[:], dtype=np.float64)
    out["w"] = params.w
    return out


def params_with(params: "Params", rec) -> "Params":
    """A copy of `params` with the seven fields of one per-instance record in place (the handle a plain solve of that
    instance would use)."""
    out = params.copy()
    out.mass = float(rec["mass"])
    out.inertia[:] = [float(x) for x in np.asarray(rec["inertia"]).ravel()]
    out.mu = float(rec["mu"])
    out.fz_max = float(rec["fz_max"])
    out.q_weights[:] = [float(x) for x in rec["q_weights"]]
    out.r_weights[:] = [float(x) for x in rec["r_weights"]]
    out.w = float(rec["w"])
    return out


# struct qmpc_plant_params (qmpc_loop_run_instances*): one robot's TRUE plant, 16 doubles = 128 B
PLANT_PARAMS_DTYPE = np.dtype(
    [
        ("mass", "<f8"),
        ("inertia", "<f8", (9,)),
        ("ext_force_world", "<f8", (3,)),
        ("ext_torque_body", "<f8", (3,)),
    ],
    align=False,
)
assert PLANT_PARAMS_DTYPE.itemsize == 16 * 8


def plant_params(params: "Params", batch: int = 1) -> np.ndarray:
    """[batch] plant records all carrying the mass and inertia of `params`, no disturbance (edit per robot afterwards)."""
    out = np.zeros(int(batch), dtype=PLANT_PARAMS_DTYPE)
    out["mass"] = params.mass
    out["inertia"] = np.asarray(params.inertia[:], dtype=np.float64)
    return out


# struct qmpc_loop_outcome (qmpc_loop_run_outcomes*): one robot's outcome record, 16 doubles = 128 B
LOOP_OUTCOME_DTYPE = np.dtype(
    [
        ("ticks", "<f8"),
        ("down_tick", "<f8"),
        ("min_height", "<f8"),
        ("min_upright", "<f8"),
        ("max_height_err", "<f8"),
        ("max_vel_err", "<f8"),
        ("sum_vel_err_sq", "<f8"),
        ("max_ang_vel", "<f8"),
        ("max_force_z", "<f8"),
        ("not_ok_ticks", "<f8"),
        ("rejected_ticks", "<f8"),
        ("first_rejected_tick", "<f8"),
        ("iterations_sum", "<f8"),
        ("iterations_max", "<f8"),
        ("reserved", "<f8", (2,)),
    ],
    align=False,
)
assert LOOP_OUTCOME_DTYPE.itemsize == 16 * 8


class OutcomeParams(C.Structure):
    """struct qmpc_outcome_params"""
    _fields_ = [("down_height", C.c_double), ("down_upright", C.c_double), ("stop_when_down", C.c_double), ("reserved", C.c_double)]


# struct qmpc_push_params (qmpc_loop_run_pushes*): one push window of one robot, 8 doubles = 64 B
PUSH_PARAMS_DTYPE = np.dtype(
    [
        ("start_tick", "<f8"),
        ("ticks", "<f8"),
        ("force_world", "<f8", (3,)),
        ("torque_body", "<f8", (3,)),
    ],
    align=False,
)
assert PUSH_PARAMS_DTYPE.itemsize == 8 * 8
MAX_PUSHES = 8      # QMPC_MAX_PUSHES


def push_params(batch: int, per_robot: int = 1) -> np.ndarray:
    """[batch][per_robot] push windows, all fields zero: no push (fill start_tick, ticks, force_world, torque_body per robot)."""
    return np.zeros((int(batch), int(per_robot)), dtype=PUSH_PARAMS_DTYPE)


# struct qmpc_ground_params (qmpc_loop_run_ground*): the TRUE ground / actuator under each foot of one robot, 8 doubles = 64 B
GROUND_PARAMS_DTYPE = np.dtype([("mu", "<f8", (4,)), ("fz_max", "<f8", (4,))], align=False)
# struct qmpc_ground_tally: what the ground cut of one robot's commands, 4 doubles = 32 B (in/out: accumulates over calls)
GROUND_TALLY_DTYPE = np.dtype(
    [
        ("clipped_ticks", "<f8"),
        ("first_clipped_tick", "<f8"),
        ("friction_leg_ticks", "<f8"),
        ("normal_leg_ticks", "<f8"),
    ],
    align=False,
)
assert GROUND_PARAMS_DTYPE.itemsize == 8 * 8 and GROUND_TALLY_DTYPE.itemsize == 4 * 8


def ground_params(batch: int) -> np.ndarray:
    """[batch] ground records that limit nothing: every field +inf, the bytes of qmpc_ground_params_init (set mu / fz_max per
    robot and leg)."""
    out = np.zeros(int(batch), dtype=GROUND_PARAMS_DTYPE)
    out["mu"] = np.inf
    out["fz_max"] = np.inf
    return out


def ground_tallies(batch: int) -> np.ndarray:
    """[batch] empty tallies: 0, -1, 0, 0, the bytes of qmpc_ground_tally_init."""
    out = np.zeros(int(batch), dtype=GROUND_TALLY_DTYPE)
    out["first_clipped_tick"] = -1.0
    return out


# struct qmpc_actuation_params (qmpc_loop_run_actuation*): the time between one robot's solve and the force under its feet, 4 doubles
MAX_DELAY = 8
ACTUATION_PARAMS_DTYPE = np.dtype([("delay_ticks", "<f8"), ("alpha", "<f8"), ("reserved", "<f8", (2,))], align=False)
# struct qmpc_actuation_line: the robot's delay line, 112 doubles = 896 B (in/out: carries over calls)
ACTUATION_LINE_DTYPE = np.dtype(
    [("cmd", "<f8", (MAX_DELAY, 12)), ("applied", "<f8", (12,)), ("count", "<f8"), ("reserved", "<f8", (3,))], align=False)
assert ACTUATION_PARAMS_DTYPE.itemsize == 4 * 8 and ACTUATION_LINE_DTYPE.itemsize == 112 * 8


def actuation_params(batch: int, delay_ticks=0, tau=None, dt: float = 0.005) -> np.ndarray:
    """[batch] actuation records: the plant receives the command of delay_ticks ticks ago (an integer in 0 .. MAX_DELAY, or one
    per robot) through a first-order actuator of time constant tau seconds (None or 0: no lag; or one per robot) sampled at
    the loop's tick dt: alpha = 1 - exp(-dt / tau).  The defaults give the bytes of qmpc_actuation_params_init."""
    out = np.zeros(int(batch), dtype=ACTUATION_PARAMS_DTYPE)
    out["delay_ticks"] = delay_ticks
    out["alpha"] = 1.0
    if tau is not None:
        tau = np.broadcast_to(np.asarray(tau, dtype=np.float64), (int(batch),))
        lag = tau > 0.0
        out["alpha"][lag] = -np.expm1(-float(dt) / tau[lag])
    return out


def stand_forces_body(mass: float) -> np.ndarray:
    """[12] the body-frame force of a level robot standing still: m g / 4 on each leg's fz (g = 9.81, the plant's)."""
    f = np.zeros(12)
    f[2::3] = float(mass) * 9.81 / 4.0
    return f


def actuation_lines(batch: int, initial=None) -> np.ndarray:
    """[batch] delay lines before the first command: every ring slot and applied hold `initial` ([12] body-frame forces, e.g.
    stand_forces_body(params.mass), or [batch, 12]; None: zeros), count = 0 -- the bytes of qmpc_actuation_line_init."""
    out = np.zeros(int(batch), dtype=ACTUATION_LINE_DTYPE)
    if initial is not None:
        f = np.broadcast_to(np.asarray(initial, dtype=np.float64), (int(batch), 12))
        out["cmd"] = f[:, None, :]
        out["applied"] = f
    return out


# struct qmpc_sense_params (qmpc_loop_run_sensing*): what one robot's state estimator gets wrong, 32 doubles = 256 B.  Channels
# 0-2 pos_world [m], 3-5 attitude error phi in the body frame [rad], 6-8 lin_vel_world [m/s], 9-11 ang_vel_body [rad/s]
SENSE_PARAMS_DTYPE = np.dtype([("bias", "<f8", (12,)), ("sigma", "<f8", (12,)), ("seed", "<f8"), ("reserved", "<f8", (7,))], align=False)
# struct qmpc_sense_seen: what the controller read in the robot's last tick, 16 doubles = 128 B (in/out: ticks accumulates)
SENSE_SEEN_DTYPE = np.dtype([("meas", "<f8", (13,)), ("ticks", "<f8"), ("reserved", "<f8", (2,))], align=False)
assert SENSE_PARAMS_DTYPE.itemsize == 32 * 8 and SENSE_SEEN_DTYPE.itemsize == 16 * 8
SENSE_GROUPS = {"pos": slice(0, 3), "att": slice(3, 6), "vel": slice(6, 9), "gyro": slice(9, 12)}


def sense_params(batch: int, seed=0, pos_bias=0.0, att_bias=0.0, vel_bias=0.0, gyro_bias=0.0, pos_noise=0.0, att_noise=0.0,
                 vel_noise=0.0, gyro_noise=0.0) -> np.ndarray:
    """[batch] sensing records: the controller reads the true state plus a bias and per-tick noise of standard deviation *_noise
    on position [m], attitude (a rotation vector in the body frame [rad]), world-frame velocity [m/s] and body rate [rad/s] (the
    gyro bias).  Every argument is a scalar, a 3-vector or [batch, 3] (a scalar applies to the three axes); seed an integer in
    0 .. 2^53 - 1 or one per robot -- robots that share a seed draw the same noise.  The defaults give the bytes of
    qmpc_sense_params_init."""
    B = int(batch)
    out = np.zeros(B, dtype=SENSE_PARAMS_DTYPE)
    out["seed"] = seed
    for key, b, n in (("pos", pos_bias, pos_noise), ("att", att_bias, att_noise), ("vel", vel_bias, vel_noise),
                      ("gyro", gyro_bias, gyro_noise)):
        for field, v in (("bias", b), ("sigma", n)):
            out[field][:, SENSE_GROUPS[key]] = np.broadcast_to(np.asarray(v, dtype=np.float64), (B, 3))
    return out


def sense_seen(batch: int) -> np.ndarray:
    """[batch] empty seen records: all zero, the bytes of qmpc_sense_seen_init."""
    return np.zeros(int(batch), dtype=SENSE_SEEN_DTYPE)


# struct qmpc_gait_params (qmpc_loop_run_gaits*): one robot's gait, 16 doubles = 128 B.  Legs in the order FL, FR, RL, RR
GAIT_PARAMS_DTYPE = np.dtype([("gait_freq", "<f8"), ("first_stance", "<f8", (4,)), ("split", "<f8", (4,)), ("phase0", "<f8", (4,)),
                              ("reserved", "<f8", (3,))], align=False)
assert GAIT_PARAMS_DTYPE.itemsize == 16 * 8
# the named gaits: (first_stance, split, phase0) per leg FL, FR, RL, RR.  Every one is valid (no planned flight); trot is the
# reference's set_default_gait_pattern -- at the call's gait_freq it is the identity record
GAITS = {
    "trot": ((1, 0, 0, 1), (0.5,) * 4, (0.0,) * 4),
    "pace": ((1, 0, 1, 0), (0.5,) * 4, (0.0,) * 4),
    "bound": ((1, 1, 0, 0), (0.5,) * 4, (0.0,) * 4),
    "trot_overlap": ((1, 0, 0, 1), (0.625, 0.375, 0.375, 0.625), (0.0, 0.875, 0.875, 0.0)),
    "crawl": ((0, 0, 0, 0), (0.25,) * 4, (0.0, 0.75, 0.5, 0.25)),
    "amble": ((0, 0, 0, 0), (0.375,) * 4, (0.0, 0.5, 0.75, 0.25)),
}


def gait_params(batch: int, gait="trot", gait_freq=None, lp: "LoopParams | None" = None) -> np.ndarray:
    """[batch] gait records: gait a name of GAITS or one per robot, gait_freq [Hz] a scalar or one per robot (None: lp's, the
    library's default loop parameters when lp is None too).  gait_params(B) is the identity record of qmpc_default_gait_params:
    the reference's trot at the call's frequency."""
    B = int(batch)
    out = np.zeros(B, dtype=GAIT_PARAMS_DTYPE)
    if gait_freq is None:
        gait_freq = (lp or default_loop_params()).gait_freq
    out["gait_freq"] = np.broadcast_to(np.asarray(gait_freq, dtype=np.float64), (B,))
    names = [gait] * B if isinstance(gait, str) else list(gait)
    if len(names) != B:
        raise ValueError(f"gait: {len(names)} names for {B} robots")
    for i, n in enumerate(names):
        if n not in GAITS:
            raise ValueError(f"gait: unknown name {n!r} (one of {', '.join(GAITS)})")
        out["first_stance"][i], out["split"][i], out["phase0"][i] = GAITS[n]
    return out


def loop_states_set_gait(states: np.ndarray, gait: np.ndarray, lib: "C.CDLL | None" = None) -> np.ndarray:
    """qmpc_loop_state_set_gait on a copy of `states`: every robot's four legs at their gait's starting phase, in their pattern's
    state, contacts to match -- for robots that walk (movement_mode != 0) from tick 0."""
    lib = lib or load_library()
    st = np.ascontiguousarray(states, dtype=LOOP_STATE_DTYPE).copy()
    g = np.ascontiguousarray(gait, dtype=GAIT_PARAMS_DTYPE)
    if g.shape != st.shape:
        raise ValueError(f"gait: shape {g.shape}, expected {st.shape}")
    for i in range(st.shape[0]):
        lib.qmpc_loop_state_set_gait(C.c_void_p(st[i:i + 1].ctypes.data), C.c_void_p(g[i:i + 1].ctypes.data))
    return st


def constant_schedule(inputs: np.ndarray, N: int) -> np.ndarray:
    """[B, N] uint8 schedule for Solver.solve_schedule: the record's contacts at every knot (bit l: leg l stands).  With it the
    call gives solve_instances' results bit for bit."""
    inputs = np.ascontiguousarray(inputs, dtype=INPUT_DTYPE)
    m = ((inputs["contacts"] != 0.0).astype(np.uint8) << np.arange(4, dtype=np.uint8)).sum(axis=1).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(m[:, None], int(N), axis=1))


def predict_schedule(lp: "LoopParams | None", gait: "np.ndarray | None", states: np.ndarray, h: float, N: int,
                     lib: "C.CDLL | None" = None) -> np.ndarray:
    """qmpc_gait_predict per robot: [B, N] uint8, row b the contact schedule robot b's gait state implies over N knots h apart
    (knot 0: its current contacts).  gait None: the reference's trot at lp.gait_freq for every robot.  `states` is not changed."""
    lib = lib or load_library()
    st = np.ascontiguousarray(states, dtype=LOOP_STATE_DTYPE)
    B = st.shape[0]
    g = None if gait is None else np.ascontiguousarray(gait, dtype=GAIT_PARAMS_DTYPE)
    if g is not None and g.shape != (B,):
        raise ValueError(f"gait: shape {g.shape}, expected ({B},)")
    if g is None and lp is None:
        lp = default_loop_params(lib)
    out = np.zeros((B, int(N)), dtype=np.uint8)
    for i in range(B):
        lib.qmpc_gait_predict(C.byref(lp) if lp is not None else None, C.c_void_p(g[i:i + 1].ctypes.data) if g is not None else None,
                              C.c_void_p(st[i:i + 1].ctypes.data), float(h), int(N), C.c_void_p(out[i:i + 1].ctypes.data))
    return out


SCHEDULE_FAMILIES = ("constant", "trot_four_other", "trot_other", "trot_three")


def schedule_families(inputs: np.ndarray, N: int) -> dict:
    """The four schedule families the schedule tests and tools/instance_params_bench.py --schedule share, for a batch of trot
    records, as {name: [B, N] uint8}.  With m the record's stance set and o the legs it leaves out -- the other diagonal of a
    trot record; for a record whose four legs all stand, the diagonal FL + RR (the robot starts to trot):
      constant         m at every knot
      trot_four_other  m for 3 knots, all four legs for 2, o for the rest      (at N = 10: 3 + 2 + 5)
      trot_other       m for the first 2N/5 knots, o for the rest, no overlap  (4 + 6)
      trot_three       m for the first N/2 knots, then m plus the lowest-numbered other leg  (5 + 5)"""
    N = int(N)
    c = constant_schedule(inputs, N)
    m = c[:, 0]
    o = (np.uint8(15) & ~m).astype(np.uint8)
    o = np.where(o == 0, np.uint8(9), o).astype(np.uint8)
    low = (o & (~o + np.uint8(1))).astype(np.uint8)      # lowest set bit of the other diagonal
    k = np.arange(N)[None, :]
    four = np.where(k < 3, m[:, None], np.where(k < 5, np.uint8(15), o[:, None])).astype(np.uint8)
    other = np.where(k < (2 * N) // 5, m[:, None], o[:, None]).astype(np.uint8)
    three = np.where(k < N // 2, m[:, None], (m | low)[:, None]).astype(np.uint8)
    return {"constant": c, "trot_four_other": np.ascontiguousarray(four), "trot_other": np.ascontiguousarray(other),
            "trot_three": np.ascontiguousarray(three)}


# struct qmpc_motor_params (qmpc_loop_run_motors*): one robot's joint torque limits, 16 doubles = 128 B.  Joints leg-major
# (FL, FR, RL, RR) x (hip, thigh, calf)
MOTOR_PARAMS_DTYPE = np.dtype([("tau_max", "<f8", (12,)), ("reserved", "<f8", (4,))], align=False)
assert MOTOR_PARAMS_DTYPE.itemsize == 16 * 8
# struct qmpc_motor_tally: what the motors of one robot were asked for, 40 doubles = 320 B; in/out, accumulates over calls
MOTOR_TALLY_DTYPE = np.dtype([("joint_pos", "<f8", (12,)), ("peak_tau", "<f8", (12,)), ("sat_ticks", "<f8", (12,)),
                              ("clipped_ticks", "<f8"), ("first_clipped_tick", "<f8"), ("unreachable_leg_ticks", "<f8"),
                              ("reserved", "<f8")], align=False)
assert MOTOR_TALLY_DTYPE.itemsize == 40 * 8
# the Go1's joint torque limits [N m] per joint type (hip, thigh, calf): 23.7 at the motor, the calf through its 1.5 linkage
GO1_TAU_MAX = (23.7, 23.7, 35.55)


def motor_params(batch: int, tau_max=np.inf) -> np.ndarray:
    """[batch] motor records: tau_max [N m] a scalar, three values per joint type (hip, thigh, calf), or the full [batch][12]
    (leg-major).  motor_params(B) is qmpc_default_motor_params: every limit +inf -- nothing binds, the tally still records the
    torque every joint was asked for."""
    B = int(batch)
    out = np.zeros(B, dtype=MOTOR_PARAMS_DTYPE)
    t = np.asarray(tau_max, dtype=np.float64)
    if t.ndim == 1 and t.shape == (3,):
        t = np.tile(t, 4)
    elif t.ndim not in (0, 2) or (t.ndim == 2 and t.shape != (B, 12)):
        raise ValueError(f"tau_max: shape {t.shape}, expected a scalar, (3,) or ({B}, 12)")
    out["tau_max"] = np.broadcast_to(t, (B, 12))
    return out


def motor_tallies(batch: int, lib: "C.CDLL | None" = None) -> np.ndarray:
    """[batch] motor tallies of qmpc_motor_tally_init: joint_pos the stand pose, first_clipped_tick -1, everything else 0."""
    lib = lib or load_library()
    out = np.zeros(int(batch), dtype=MOTOR_TALLY_DTYPE)
    for i in range(out.shape[0]):
        lib.qmpc_motor_tally_init(C.c_void_p(out[i:i + 1].ctypes.data))
    return out


# struct qmpc_info: 2 x int32 + 4 doubles = 40 B
INFO_DTYPE = np.dtype(
    [
        ("status", "<i4"),
        ("iterations", "<i4"),
        ("cost", "<f8"),
        ("max_violation", "<f8"),
        ("last_step", "<f8"),
        ("penalty", "<f8"),
    ],
    align=False,
)
assert INFO_DTYPE.itemsize == 40


# how many arguments each closed-loop call with records takes after trace_contacts (include/qmpc.h), of: op, outcomes, push,
# pushes_per_robot, ground, tally, act, line, sense, seen, gait, geom, motor, motor_tally
_LOOP_RECORD_ARGS = {"instances": 0, "outcomes": 2, "pushes": 4, "ground": 6, "actuation": 8, "sensing": 10, "gaits": 11, "motors": 14}


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class QmpcError(RuntimeError):
    def __init__(self, code: int, what: str):
        super().__init__(f"{what}: qmpc_status {code}")
        self.code = code


def load_library(path: os.PathLike | None = None) -> C.CDLL:
    """dlopen the HIP library.  Raises (never falls back) when it is absent."""
    # QMPC_LIB: a diagnostic build of the same library (tools/.prof/, phase counters compiled in)
    p = Path(path) if path else Path(os.environ.get("QMPC_LIB") or LIB_PATH)
    # torch bundles its own libamdhip64.so.7; whichever HIP runtime is loaded
    # first serves the whole process.  Let torch (our device-memory / stream /
    # RCCL plumbing) load its runtime first so both sides share one.
    try:
        import torch

        if torch.cuda.is_available():
            torch.cuda.init()
    except ImportError:
        pass
    if not p.exists():
        raise FileNotFoundError(
            f"{p} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback."
        )
    lib = C.CDLL(str(p))
    vp, i32 = C.c_void_p, C.c_int32
    lib.qmpc_default_params.argtypes = [C.POINTER(Params), i32, i32]
    lib.qmpc_default_params.restype = None
    lib.qmpc_create.argtypes = [C.POINTER(Params), i32, i32, C.POINTER(vp)]
    lib.qmpc_create.restype = i32
    lib.qmpc_set_params.argtypes = [vp, C.POINTER(Params)]
    lib.qmpc_set_params.restype = i32
    lib.qmpc_destroy.argtypes = [vp]
    lib.qmpc_destroy.restype = None
    lib.qmpc_solve.argtypes = [vp, i32, vp, vp, vp]
    lib.qmpc_solve.restype = i32
    lib.qmpc_solve_traj.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    lib.qmpc_solve_traj.restype = i32
    lib.qmpc_solve_device.argtypes = [vp, i32, vp, vp, vp, vp]
    lib.qmpc_solve_device.restype = i32
    lib.qmpc_wait.argtypes = [vp]
    lib.qmpc_wait.restype = i32
    lib.qmpc_solve_async.argtypes = [vp, i32, vp, vp, vp]
    lib.qmpc_solve_async.restype = i32
    lib.qmpc_host_alloc.argtypes = [C.c_size_t]
    lib.qmpc_host_alloc.restype = vp
    lib.qmpc_host_free.argtypes = [vp]
    lib.qmpc_host_free.restype = None
    lib.qmpc_prepare.argtypes = [vp, i32]
    lib.qmpc_prepare.restype = i32
    lib.qmpc_query.argtypes = [vp, i32, C.c_int64, C.POINTER(C.c_int64)]
    lib.qmpc_query.restype = i32
    lib.qmpc_instance_params_from.argtypes = [C.POINTER(Params), vp]
    lib.qmpc_instance_params_from.restype = None
    lib.qmpc_solve_instances.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    lib.qmpc_solve_instances.restype = i32
    lib.qmpc_solve_instances_device.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    lib.qmpc_solve_instances_device.restype = i32
    lib.qmpc_solve_schedule.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.qmpc_solve_schedule.restype = i32
    lib.qmpc_solve_schedule_device.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.qmpc_solve_schedule_device.restype = i32
    lib.qmpc_gait_predict.argtypes = [vp, vp, vp, C.c_double, i32, vp]
    lib.qmpc_gait_predict.restype = None
    lib.qmpc_convex_solve_instances.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    lib.qmpc_convex_solve_instances.restype = i32
    lib.qmpc_convex_solve_instances_device.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    lib.qmpc_convex_solve_instances_device.restype = i32
    lib.qmpc_prepare_instances.argtypes = [vp]
    lib.qmpc_plant_params_from.argtypes = [C.POINTER(Params), vp]
    lib.qmpc_plant_params_from.restype = None
    lib.qmpc_prepare_instances.restype = i32
    # the closed-loop calls with per-robot records: every entry point takes the arguments of the one before it, then its own
    # (_LOOP_RECORD_ARGS of them in all), the device-buffer form a stream after them
    head = [vp, C.POINTER(LoopParams), i32, vp, i32, vp, vp, vp, vp]
    tail = [C.POINTER(OutcomeParams), vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, C.POINTER(LegGeometry), vp, vp]
    for name, n in _LOOP_RECORD_ARGS.items():
        for fn, args in ((getattr(lib, "qmpc_loop_run_" + name), head + tail[:n]),
                         (getattr(lib, "qmpc_loop_run_" + name + "_device"), head + tail[:n] + [vp])):
            fn.argtypes, fn.restype = args, i32
    lib.qmpc_default_outcome_params.argtypes = [C.POINTER(OutcomeParams)]
    lib.qmpc_default_outcome_params.restype = None
    lib.qmpc_loop_outcome_init.argtypes = [vp, i32]
    lib.qmpc_loop_outcome_init.restype = None
    lib.qmpc_ground_params_init.argtypes = [vp, i32]
    lib.qmpc_ground_params_init.restype = None
    lib.qmpc_ground_tally_init.argtypes = [vp, i32]
    lib.qmpc_ground_tally_init.restype = None
    lib.qmpc_actuation_params_init.argtypes = [vp, i32]
    lib.qmpc_actuation_params_init.restype = None
    lib.qmpc_actuation_line_init.argtypes = [vp, i32, vp]
    lib.qmpc_actuation_line_init.restype = None
    lib.qmpc_sense_params_init.argtypes = [vp, i32]
    lib.qmpc_sense_params_init.restype = None
    lib.qmpc_sense_seen_init.argtypes = [vp, i32]
    lib.qmpc_sense_seen_init.restype = None
    lib.qmpc_default_gait_params.argtypes = [C.POINTER(LoopParams), vp]
    lib.qmpc_default_gait_params.restype = None
    lib.qmpc_loop_state_set_gait.argtypes = [vp, vp]
    lib.qmpc_loop_state_set_gait.restype = None
    lib.qmpc_default_motor_params.argtypes = [vp]
    lib.qmpc_default_motor_params.restype = None
    lib.qmpc_motor_tally_init.argtypes = [vp]
    lib.qmpc_motor_tally_init.restype = None
    lib.qmpc_set_instances_policy.argtypes = [vp, i32]
    lib.qmpc_set_instances_policy.restype = i32
    lib.qmpc_set_loop_warm_records.argtypes = [vp, i32]
    lib.qmpc_set_loop_warm_records.restype = i32
    lib.qmpc_set_convex_records.argtypes = [vp, i32]
    lib.qmpc_set_convex_records.restype = i32
    lib.qmpc_set_convex_lane_records.argtypes = [vp, i32]
    lib.qmpc_set_convex_lane_records.restype = i32
    lib.qmpc_set_convex_warm_records.argtypes = [vp, i32]
    lib.qmpc_set_convex_warm_records.restype = i32
    lib.qmpc_gather.argtypes = [vp, vp, vp, C.c_int64, vp, vp]
    lib.qmpc_gather.restype = i32
    lib.qmpc_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
    lib.qmpc_last_kernel_ms.restype = i32
    lib.qmpc_linearize.argtypes = [vp, i32, vp, vp, vp, vp]
    lib.qmpc_linearize.restype = i32
    lib.qmpc_debug_profile.argtypes = [vp, i32, vp, vp]
    lib.qmpc_debug_profile.restype = i32
    lib.qmpc_selftest_lanes.argtypes = [i32, vp, vp]
    lib.qmpc_selftest_lanes.restype = i32
    lib.qmpc_selftest_mtm.argtypes = [i32, vp, vp, vp]
    lib.qmpc_selftest_mtm.restype = i32
    lib.qmpc_status_string.argtypes = [i32]
    lib.qmpc_status_string.restype = C.c_char_p
    lib.qmpc_version.argtypes = []
    lib.qmpc_version.restype = C.c_char_p
    lib.qmpc_default_convex_params.argtypes = [C.POINTER(Params), i32, i32]
    lib.qmpc_default_convex_params.restype = None
    lib.qmpc_convex_solve.argtypes = [vp, i32, vp, vp, vp]
    lib.qmpc_convex_solve.restype = i32
    lib.qmpc_convex_solve_traj.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    lib.qmpc_convex_solve_traj.restype = i32
    lib.qmpc_convex_solve_device.argtypes = [vp, i32, vp, vp, vp, vp]
    lib.qmpc_convex_solve_device.restype = i32
    lib.qmpc_convex_linearize.argtypes = [vp, i32, vp, vp, vp, vp]
    lib.qmpc_convex_linearize.restype = i32
    lib.qmpc_default_go1_geometry.argtypes = [C.POINTER(LegGeometry)]
    lib.qmpc_default_go1_geometry.restype = None
    lib.qmpc_leg_kinematics.argtypes = [vp, C.POINTER(LegGeometry), i32, vp, vp, vp]
    lib.qmpc_leg_kinematics.restype = i32
    lib.qmpc_torque_map.argtypes = [vp, C.POINTER(LegGeometry), i32, vp, vp, vp, i32, vp]
    lib.qmpc_torque_map.restype = i32
    lib.qmpc_torque_map_device.argtypes = [vp, C.POINTER(LegGeometry), i32, vp, vp, vp, i32, vp, vp]
    lib.qmpc_torque_map_device.restype = i32
    lib.qmpc_leg_inverse_kinematics.argtypes = [vp, C.POINTER(LegGeometry), i32, vp, vp, vp]
    lib.qmpc_leg_inverse_kinematics.restype = i32
    lib.qmpc_joint_commands.argtypes = [vp, C.POINTER(LegGeometry), i32, vp, vp]
    lib.qmpc_joint_commands.restype = i32
    lib.qmpc_joint_commands_device.argtypes = [vp, C.POINTER(LegGeometry), i32, vp, vp, vp]
    lib.qmpc_joint_commands_device.restype = i32
    lib.qmpc_loop_joint_commands_device.argtypes = [vp, C.POINTER(LegGeometry), i32, vp, vp, vp, vp, vp]
    lib.qmpc_loop_joint_commands_device.restype = i32
    lib.qmpc_loop_run_joint_device.argtypes = [vp, C.POINTER(LoopParams), C.POINTER(LegGeometry), i32, vp, vp, i32, vp, vp, vp]
    lib.qmpc_loop_run_joint_device.restype = i32
    lib.qmpc_loop_joint_commands.argtypes = [vp, C.POINTER(LegGeometry), i32, vp, vp, vp, vp]
    lib.qmpc_loop_joint_commands.restype = i32
    lib.qmpc_solve_warm.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    lib.qmpc_solve_warm.restype = i32
    lib.qmpc_solve_warm_device.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    lib.qmpc_solve_warm_device.restype = i32
    lib.qmpc_loop_joint_init.argtypes = [vp, i32]
    lib.qmpc_loop_joint_init.restype = None
    lib.qmpc_default_biped8_params.argtypes = [C.POINTER(Params), i32, i32]
    lib.qmpc_default_biped8_params.restype = None
    lib.qmpc_solve8.argtypes = [vp, i32, vp, vp, vp]
    lib.qmpc_solve8.restype = i32
    lib.qmpc_solve8_traj.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    lib.qmpc_solve8_traj.restype = i32
    lib.qmpc_solve8_device.argtypes = [vp, i32, vp, vp, vp, vp]
    lib.qmpc_solve8_device.restype = i32
    lib.qmpc_default_loop_params.argtypes = [C.POINTER(LoopParams)]
    lib.qmpc_default_loop_params.restype = None
    lib.qmpc_loop_state_init.argtypes = [vp, C.POINTER(LoopParams), vp, C.c_double, C.c_double, C.c_double]
    lib.qmpc_loop_state_init.restype = None
    lib.qmpc_loop_run.argtypes = [vp, C.POINTER(LoopParams), i32, vp, i32, vp, vp]
    lib.qmpc_loop_run.restype = i32
    lib.qmpc_loop_run_device.argtypes = [vp, C.POINTER(LoopParams), i32, vp, i32, vp, vp, vp]
    lib.qmpc_loop_run_device.restype = i32
    for name in ("qmpc_sizeof_input", "qmpc_sizeof_params", "qmpc_sizeof_info", "qmpc_sizeof_convex_input",
                 "qmpc_sizeof_input8", "qmpc_sizeof_loop_state", "qmpc_sizeof_instance_params", "qmpc_sizeof_plant_params",
                 "qmpc_sizeof_loop_outcome", "qmpc_sizeof_push_params", "qmpc_sizeof_ground_params", "qmpc_sizeof_ground_tally",
                 "qmpc_sizeof_actuation_params", "qmpc_sizeof_actuation_line", "qmpc_sizeof_sense_params", "qmpc_sizeof_sense_seen",
                 "qmpc_sizeof_gait_params", "qmpc_sizeof_motor_params", "qmpc_sizeof_motor_tally"):
        getattr(lib, name).argtypes = []
        getattr(lib, name).restype = i32
    if lib.qmpc_sizeof_input() != INPUT_DTYPE.itemsize:
        raise RuntimeError("qmpc_input ABI size mismatch")
    if lib.qmpc_sizeof_convex_input() != CONVEX_INPUT_DTYPE.itemsize:
        raise RuntimeError("qmpc_convex_input ABI size mismatch")
    if lib.qmpc_sizeof_input8() != INPUT8_DTYPE.itemsize:
        raise RuntimeError("qmpc_input8 ABI size mismatch")
    if lib.qmpc_sizeof_params() != C.sizeof(Params):
        raise RuntimeError("qmpc_params ABI size mismatch")
    if lib.qmpc_sizeof_info() != INFO_DTYPE.itemsize:
        raise RuntimeError("qmpc_info ABI size mismatch")
    if lib.qmpc_sizeof_loop_state() != LOOP_STATE_DTYPE.itemsize:
        raise RuntimeError("qmpc_loop_state ABI size mismatch")
    if lib.qmpc_sizeof_instance_params() != INSTANCE_PARAMS_DTYPE.itemsize:
        raise RuntimeError("qmpc_instance_params ABI size mismatch")
    if lib.qmpc_sizeof_plant_params() != PLANT_PARAMS_DTYPE.itemsize:
        raise RuntimeError("qmpc_plant_params ABI size mismatch")
    if lib.qmpc_sizeof_loop_outcome() != LOOP_OUTCOME_DTYPE.itemsize or C.sizeof(OutcomeParams) != 32:
        raise RuntimeError("qmpc_loop_outcome ABI size mismatch")
    if lib.qmpc_sizeof_push_params() != PUSH_PARAMS_DTYPE.itemsize:
        raise RuntimeError("qmpc_push_params ABI size mismatch")
    if lib.qmpc_sizeof_ground_params() != GROUND_PARAMS_DTYPE.itemsize or lib.qmpc_sizeof_ground_tally() != GROUND_TALLY_DTYPE.itemsize:
        raise RuntimeError("qmpc_ground_params / qmpc_ground_tally ABI size mismatch")
    if (lib.qmpc_sizeof_actuation_params() != ACTUATION_PARAMS_DTYPE.itemsize
            or lib.qmpc_sizeof_actuation_line() != ACTUATION_LINE_DTYPE.itemsize):
        raise RuntimeError("qmpc_actuation_params / qmpc_actuation_line ABI size mismatch")
    if lib.qmpc_sizeof_sense_params() != SENSE_PARAMS_DTYPE.itemsize or lib.qmpc_sizeof_sense_seen() != SENSE_SEEN_DTYPE.itemsize:
        raise RuntimeError("qmpc_sense_params / qmpc_sense_seen ABI size mismatch")
    if lib.qmpc_sizeof_gait_params() != GAIT_PARAMS_DTYPE.itemsize:
        raise RuntimeError("qmpc_gait_params ABI size mismatch")
    if lib.qmpc_sizeof_motor_params() != MOTOR_PARAMS_DTYPE.itemsize or lib.qmpc_sizeof_motor_tally() != MOTOR_TALLY_DTYPE.itemsize:
        raise RuntimeError("qmpc_motor_params / qmpc_motor_tally ABI size mismatch")
    return lib


EXPORTED_SYMBOLS = (
    "qmpc_default_params",
    "qmpc_create",
    "qmpc_set_params",
    "qmpc_destroy",
    "qmpc_solve",
    "qmpc_solve_traj",
    "qmpc_solve_device",
    "qmpc_wait",
    "qmpc_solve_async",
    "qmpc_gather",
    "qmpc_last_kernel_ms",
    "qmpc_linearize",
    "qmpc_selftest_mtm",
    "qmpc_selftest_lanes",
    "qmpc_debug_profile",
    "qmpc_status_string",
    "qmpc_version",
    "qmpc_sizeof_input",
    "qmpc_sizeof_params",
    "qmpc_sizeof_info",
    "qmpc_default_convex_params",
    "qmpc_convex_solve",
    "qmpc_convex_solve_traj",
    "qmpc_convex_solve_device",
    "qmpc_convex_linearize",
    "qmpc_sizeof_convex_input",
    "qmpc_default_biped8_params",
    "qmpc_solve8",
    "qmpc_solve8_traj",
    "qmpc_solve8_device",
    "qmpc_sizeof_input8",
    "qmpc_default_go1_geometry",
    "qmpc_leg_kinematics",
    "qmpc_torque_map",
    "qmpc_torque_map_device",
    "qmpc_default_loop_params",
    "qmpc_loop_state_init",
    "qmpc_loop_run",
    "qmpc_loop_run_device",
    "qmpc_sizeof_loop_state",
    "qmpc_leg_inverse_kinematics",
    "qmpc_joint_commands",
    "qmpc_joint_commands_device",
    "qmpc_loop_joint_commands_device",
    "qmpc_loop_joint_init",
    "qmpc_loop_run_joint_device",
    "qmpc_loop_joint_commands",
    "qmpc_solve_warm",
    "qmpc_solve_warm_device",
    "qmpc_host_alloc",
    "qmpc_host_free",
    "qmpc_prepare",
    "qmpc_query",
    "qmpc_instance_params_from",
    "qmpc_sizeof_instance_params",
    "qmpc_solve_instances",
    "qmpc_solve_instances_device",
    "qmpc_convex_solve_instances",
    "qmpc_convex_solve_instances_device",
    "qmpc_set_convex_records",
    "qmpc_set_convex_lane_records",
    "qmpc_set_convex_warm_records",
    "qmpc_prepare_instances",
    "qmpc_plant_params_from",
    "qmpc_sizeof_plant_params",
    "qmpc_loop_run_instances",
    "qmpc_loop_run_instances_device",
    "qmpc_set_instances_policy",
    "qmpc_set_loop_warm_records",
    "qmpc_default_outcome_params",
    "qmpc_loop_outcome_init",
    "qmpc_sizeof_loop_outcome",
    "qmpc_loop_run_outcomes",
    "qmpc_loop_run_outcomes_device",
    "qmpc_sizeof_push_params",
    "qmpc_loop_run_pushes",
    "qmpc_loop_run_pushes_device",
    "qmpc_ground_params_init",
    "qmpc_ground_tally_init",
    "qmpc_sizeof_ground_params",
    "qmpc_sizeof_ground_tally",
    "qmpc_loop_run_ground",
    "qmpc_loop_run_ground_device",
    "qmpc_actuation_params_init",
    "qmpc_actuation_line_init",
    "qmpc_sizeof_actuation_params",
    "qmpc_sizeof_actuation_line",
    "qmpc_loop_run_actuation",
    "qmpc_loop_run_actuation_device",
    "qmpc_sense_params_init",
    "qmpc_sense_seen_init",
    "qmpc_sizeof_sense_params",
    "qmpc_sizeof_sense_seen",
    "qmpc_loop_run_sensing",
    "qmpc_loop_run_sensing_device",
    "qmpc_sizeof_gait_params",
    "qmpc_default_gait_params",
    "qmpc_loop_state_set_gait",
    "qmpc_loop_run_gaits",
    "qmpc_loop_run_gaits_device",
    "qmpc_sizeof_motor_params",
    "qmpc_sizeof_motor_tally",
    "qmpc_default_motor_params",
    "qmpc_motor_tally_init",
    "qmpc_loop_run_motors",
    "qmpc_loop_run_motors_device",
    "qmpc_solve_schedule",
    "qmpc_solve_schedule_device",
    "qmpc_gait_predict",
)

# enum qmpc_query_what / qmpc_kernel_family (include/qmpc.h)
QUERY_HANDOFF_ACTIVE, QUERY_HANDOFF_ALLOC_FAILED, QUERY_KERNEL_FOR_BATCH, QUERY_LAST_KERNEL, QUERY_LANE_CAP, \
    QUERY_DEVICE_BYTES, QUERY_ZERO_COPY, QUERY_KERNEL_FOR_INSTANCES, QUERY_LOOP_INSTANCES_PLAN = 1, 2, 3, 4, 5, 6, 7, 8, 9
QUERY_INSTANCES_POLICY = 10
QUERY_LOOP_WARM_RECORDS = 11
QUERY_KERNEL_FOR_CONVEX_INSTANCES = 12
QUERY_CONVEX_RECORDS = 13
QUERY_CONVEX_LANE_RECORDS = 14
QUERY_CONVEX_WARM_RECORDS = 15
QUERY_KERNEL_FOR_SCHEDULE = 16
# enum qmpc_instances_policy
INSTANCES_WAVE, INSTANCES_AUTO = 0, 1
INSTANCES_POLICY = {"wave": INSTANCES_WAVE, "auto": INSTANCES_AUTO}
KERNEL_FAMILY = {0: "none", 1: "wform_lds", 2: "wform_ws", 3: "dense_lds", 4: "dense_ws", 5: "lane", 6: "lane_handoff"}


def default_params(horizon: int = 10, mode: int = MODE_CONVERGED, lib: C.CDLL | None = None) -> Params:
    lib = lib or load_library()
    p = Params()
    lib.qmpc_default_params(C.byref(p), horizon, mode)
    return p


def default_convex_params(horizon: int = 20, mode: int = MODE_CONVERGED, lib: C.CDLL | None = None) -> Params:
    """ConvexMpc values of gazebo_go1_convex_mpc.yaml (params.model = MODEL_CONVEX)."""
    lib = lib or load_library()
    p = Params()
    lib.qmpc_default_convex_params(C.byref(p), horizon, mode)
    return p


def default_biped8_params(horizon: int = 16, mode: int = MODE_CONVERGED, lib: C.CDLL | None = None) -> Params:
    """Synthetic 8-contact-point biped of BASELINE config 5 (params.model = MODEL_QUAT8)."""
    lib = lib or load_library()
    p = Params()
    lib.qmpc_default_biped8_params(C.byref(p), horizon, mode)
    return p


def default_loop_params(lib: C.CDLL | None = None) -> LoopParams:
    lib = lib or load_library()
    lp = LoopParams()
    lib.qmpc_default_loop_params(C.byref(lp))
    return lp


def default_outcome_params(lib: C.CDLL | None = None, stop_when_down: bool = False) -> OutcomeParams:
    """qmpc_default_outcome_params: down below 0.15 m or beyond 60 degrees of tilt; stop_when_down halts a robot after its down tick."""
    lib = lib or load_library()
    op = OutcomeParams()
    lib.qmpc_default_outcome_params(C.byref(op))
    op.stop_when_down = 1.0 if stop_when_down else 0.0
    return op


def loop_outcomes(B: int, lib: C.CDLL | None = None) -> np.ndarray:
    """[B] empty outcome records (qmpc_loop_outcome_init)."""
    lib = lib or load_library()
    out = np.zeros(int(B), dtype=LOOP_OUTCOME_DTYPE)
    lib.qmpc_loop_outcome_init(_ptr(out), int(B))
    return out


def summarize_outcomes(o: np.ndarray) -> dict:
    """A fleet's outcome records in a few figures (numpy only): robots down and a histogram of their down ticks, worst and
    median tracking figures over the robots that accumulated at least one tick, solve statistics."""
    o = np.ascontiguousarray(o, dtype=LOOP_OUTCOME_DTYPE).ravel()
    seen = o[o["ticks"] > 0]
    down = o["down_tick"] >= 0
    out = {"robots": int(o.size), "evaluated": int(seen.size), "down": int(down.sum()),
           "down_fraction": float(down.mean()) if o.size else 0.0}
    dt = o["down_tick"][down].astype(np.int64)
    if dt.size:
        ticks, counts = np.unique(dt, return_counts=True)
        out["down_tick_histogram"] = {int(t): int(c) for t, c in zip(ticks, counts)}
        out["first_down_tick"], out["median_down_tick"] = int(dt.min()), float(np.median(dt))
    else:
        out["down_tick_histogram"] = {}
    if seen.size:
        rms = np.sqrt(seen["sum_vel_err_sq"] / seen["ticks"])
        out.update(
            min_height=float(seen["min_height"].min()), median_min_height=float(np.median(seen["min_height"])),
            min_upright=float(seen["min_upright"].min()), median_min_upright=float(np.median(seen["min_upright"])),
            worst_height_err=float(seen["max_height_err"].max()), median_height_err=float(np.median(seen["max_height_err"])),
            worst_vel_err=float(seen["max_vel_err"].max()), median_vel_err=float(np.median(seen["max_vel_err"])),
            worst_rms_vel_err=float(rms.max()), median_rms_vel_err=float(np.median(rms)),
            worst_ang_vel=float(seen["max_ang_vel"].max()), worst_force_z=float(seen["max_force_z"].max()),
            not_ok_ticks=int(seen["not_ok_ticks"].sum()), rejected_ticks=int(seen["rejected_ticks"].sum()),
            robots_with_rejected_solves=int((seen["rejected_ticks"] > 0).sum()),
            mean_iterations=float(seen["iterations_sum"].sum() / seen["ticks"].sum()),
            max_iterations=int(seen["iterations_max"].max()))
    return out


def loop_states(commands, lp: LoopParams | None = None, height: float = 0.3, yaw=0.0, lib: C.CDLL | None = None) -> np.ndarray:
    """qmpc_loop_state records of robots standing at `height` over their default footholds.
    commands: [B][7] = joy.{velx, vely, body_height, roll_rate, pitch_rate, yaw_rate}, movement_mode."""
    lib = lib or load_library()
    lp = lp or default_loop_params(lib)
    commands = np.atleast_2d(np.asarray(commands, dtype=np.float64))
    yaws = np.broadcast_to(np.asarray(yaw, dtype=np.float64), (commands.shape[0],))
    out = np.zeros(commands.shape[0], dtype=LOOP_STATE_DTYPE)
    for i, c in enumerate(commands):
        joy = np.ascontiguousarray(c[:6])
        lib.qmpc_loop_state_init(C.c_void_p(out[i:i + 1].ctypes.data), C.byref(lp), _ptr(joy), float(c[6]), float(height),
                                 float(yaws[i]))
    return out


class _PinnedBlock:
    """Owner of one qmpc_host_alloc allocation.  numpy arrays made from it (np.asarray and any view) keep it alive through
    their base chain; the memory is returned (qmpc_host_free) when the last of them is gone -- independent of any Solver."""

    def __init__(self, lib, nbytes: int):
        self._lib = lib
        self.ptr = lib.qmpc_host_alloc(nbytes)
        if not self.ptr:
            raise MemoryError("qmpc_host_alloc")
        self.__array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (int(self.ptr), False), "version": 3}

    def __del__(self):
        try:                      # the library may already be gone at interpreter shutdown
            if self.ptr:
                self._lib.qmpc_host_free(self.ptr)
                self.ptr = None
        except Exception:
            pass


class Solver:
    """Thin RAII wrapper over a qmpc_handle (one per GPU, single caller)."""

    def loop_run(self, states: np.ndarray, ticks: int, lp: LoopParams | None = None, trace: bool = False):
        """`ticks` ticks of the device-resident closed loop (front end + solve + plant per tick, state in HBM).
        Returns the final states (and, with trace, forces [ticks][B][12] and contacts [ticks][B][4])."""
        lp = lp or default_loop_params(self.lib)
        st = np.ascontiguousarray(states, dtype=LOOP_STATE_DTYPE).copy()
        B = st.shape[0]
        tf = np.zeros((ticks, B, 12)) if trace else None
        tc = np.zeros((ticks, B, 4)) if trace else None
        rc = self.lib.qmpc_loop_run(self._h, C.byref(lp), B, _ptr(st), int(ticks), _ptr(tf), _ptr(tc))
        if rc != OK:
            raise QmpcError(rc, "qmpc_loop_run")
        return (st, tf, tc) if trace else st

    def loop_run_device(self, batch: int, d_states: int, ticks: int, lp: LoopParams | None = None, d_trace_forces: int = 0,
                        d_trace_contacts: int = 0, stream: int = 0):
        lp = lp or default_loop_params(self.lib)
        rc = self.lib.qmpc_loop_run_device(self._h, C.byref(lp), int(batch), C.c_void_p(d_states), int(ticks),
                                           C.c_void_p(d_trace_forces) if d_trace_forces else None,
                                           C.c_void_p(d_trace_contacts) if d_trace_contacts else None,
                                           C.c_void_p(stream) if stream else None)
        if rc != OK:
            raise QmpcError(rc, "qmpc_loop_run_device")

    def __init__(self, params: Params, max_batch: int, device: int = 0, lib: C.CDLL | None = None):
        self.lib = lib or load_library()
        self.params = params.copy()
        self.max_batch = int(max_batch)
        self._h = C.c_void_p()
        st = self.lib.qmpc_create(C.byref(self.params), self.max_batch, device, C.byref(self._h))
        if st != OK:
            self._h = C.c_void_p()
            raise QmpcError(st, "qmpc_create")

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._h = None
            self.lib.qmpc_destroy(h)

    def __del__(self):
        try:                      # module globals may already be gone at interpreter shutdown
            self.close()
        except Exception:
            pass

    def set_params(self, params: Params):
        self.params = params.copy()
        st = self.lib.qmpc_set_params(self._h, C.byref(self.params))
        if st != OK:
            raise QmpcError(st, "qmpc_set_params")

    def solve(self, inputs: np.ndarray, want_traj: bool = False):
        """Host buffers in, host buffers out (H2D + kernel + D2H, synchronous)."""
        inputs = np.ascontiguousarray(inputs, dtype=INPUT_DTYPE)
        B, N = inputs.shape[0], self.params.horizon
        forces = np.zeros((B, NU), dtype=np.float64)
        info = np.zeros(B, dtype=INFO_DTYPE)
        if want_traj:
            tu = np.zeros((B, N, NU))
            tx = np.zeros((B, N + 1, NX))
            st = self.lib.qmpc_solve_traj(self._h, B, _ptr(inputs), _ptr(forces), _ptr(info), _ptr(tu), _ptr(tx))
            if st != OK:
                raise QmpcError(st, "qmpc_solve_traj")
            return forces, info, tu, tx
        st = self.lib.qmpc_solve(self._h, B, _ptr(inputs), _ptr(forces), _ptr(info))
        if st != OK:
            raise QmpcError(st, "qmpc_solve")
        return forces, info

    def prepare(self, batch: int | None = None):
        """Allocate now what solves of up to `batch` instances need later (qmpc_prepare)."""
        st = self.lib.qmpc_prepare(self._h, int(self.max_batch if batch is None else batch))
        if st != OK:
            raise QmpcError(st, "qmpc_prepare")

    def query(self, what: int, arg: int = 0) -> int:
        v = C.c_int64()
        st = self.lib.qmpc_query(self._h, int(what), int(arg), C.byref(v))
        if st != OK:
            raise QmpcError(st, "qmpc_query")
        return int(v.value)

    def kernel_for_batch(self, batch: int) -> str:
        return KERNEL_FAMILY[self.query(QUERY_KERNEL_FOR_BATCH, batch)]

    def pinned(self, shape, dtype=np.float64) -> np.ndarray:
        """Array in pinned, device-addressable host memory (qmpc_host_alloc).  The allocation lives as long as the array
        (or any view of it) does -- not as long as the solver: it is freed when the last reference goes away."""
        dt = np.dtype(dtype)
        count = int(np.prod(shape))
        block = _PinnedBlock(self.lib, max(count * dt.itemsize, 1))
        return np.asarray(block)[:count * dt.itemsize].view(dt).reshape(shape)      # base chain -> block

    def _check_out(self, name: str, a: np.ndarray, dtype, rows: int, cols: int | None):
        if not isinstance(a, np.ndarray) or not a.flags.c_contiguous or not a.flags.writeable:
            raise ValueError(f"{name}: a writable C-contiguous numpy array is required")
        if a.dtype != np.dtype(dtype):
            raise ValueError(f"{name}: dtype {a.dtype}, expected {np.dtype(dtype)}")
        need = rows * (cols if cols else 1)
        if a.size < need or (cols and a.ndim == 2 and a.shape[1] != cols):
            raise ValueError(f"{name}: shape {a.shape} cannot hold [{rows}" + (f", {cols}]" if cols else "]"))

    def solve_into(self, inputs: np.ndarray, forces: np.ndarray, info: np.ndarray | None = None):
        """qmpc_solve on caller-owned buffers (no allocation, no conversion): the call a C host makes.  The buffers are
        checked (layout, element type, room for the batch): the kernel writes through raw pointers."""
        if not isinstance(inputs, np.ndarray) or not inputs.flags.c_contiguous:
            raise ValueError("inputs: a C-contiguous numpy array is required")
        B = inputs.shape[0]
        if inputs.nbytes != B * INPUT_DTYPE.itemsize:
            raise ValueError(f"inputs: {inputs.nbytes} bytes for {B} records of {INPUT_DTYPE.itemsize} bytes")
        self._check_out("forces", forces, np.float64, B, NU)
        if info is not None:
            self._check_out("info", info, INFO_DTYPE, B, None)
        st = self.lib.qmpc_solve(self._h, B, _ptr(inputs), _ptr(forces), _ptr(info) if info is not None else None)
        if st != OK:
            raise QmpcError(st, "qmpc_solve")

    def solve_warm(self, inputs: np.ndarray, u_init: np.ndarray | None = None):
        """Warm-started solve: (forces [B,12], info, traj_u [B,N,12]); u_init = a previous traj_u (None: cold)."""
        inputs = np.ascontiguousarray(inputs, dtype=INPUT_DTYPE)
        B, N = inputs.shape[0], self.params.horizon
        forces = np.zeros((B, NU))
        info = np.zeros(B, dtype=INFO_DTYPE)
        tu = np.zeros((B, N, NU))
        ui = None if u_init is None else np.ascontiguousarray(u_init, dtype=np.float64).reshape(B, N, NU)
        st = self.lib.qmpc_solve_warm(self._h, B, _ptr(inputs), _ptr(ui), _ptr(forces), _ptr(info), _ptr(tu))
        if st != OK:
            raise QmpcError(st, "qmpc_solve_warm")
        return forces, info, tu

    def solve_device(self, batch: int, d_in: int, d_forces: int, d_info: int, stream: int = 0):
        """Device pointers (ints), stream-ordered, no synchronisation."""
        st = self.lib.qmpc_solve_device(self._h, int(batch), C.c_void_p(d_in), C.c_void_p(d_forces),
                                        C.c_void_p(d_info) if d_info else None,
                                        C.c_void_p(stream) if stream else None)
        if st != OK:
            raise QmpcError(st, "qmpc_solve_device")

    def solve_instances(self, inputs: np.ndarray, iparams: np.ndarray, want_traj: bool = False):
        """qmpc_solve_instances: instance i solved with the handle's parameters and the seven fields of iparams[i]
        (INSTANCE_PARAMS_DTYPE).  Returns (forces [B,12], info) or, with want_traj, also traj_u [B,N,12] and traj_x [B,N+1,13]."""
        inputs = np.ascontiguousarray(inputs, dtype=INPUT_DTYPE)
        iparams = np.ascontiguousarray(iparams, dtype=INSTANCE_PARAMS_DTYPE)
        B, N = inputs.shape[0], self.params.horizon
        if iparams.shape != (B,):
            raise ValueError(f"iparams: shape {iparams.shape}, expected ({B},)")
        forces = np.zeros((B, NU), dtype=np.float64)
        info = np.zeros(B, dtype=INFO_DTYPE)
        tu = np.zeros((B, N, NU)) if want_traj else None
        tx = np.zeros((B, N + 1, NX)) if want_traj else None
        st = self.lib.qmpc_solve_instances(self._h, B, _ptr(inputs), _ptr(iparams), _ptr(forces), _ptr(info), _ptr(tu), _ptr(tx))
        if st != OK:
            raise QmpcError(st, "qmpc_solve_instances")
        return (forces, info, tu, tx) if want_traj else (forces, info)

    def solve_instances_device(self, batch: int, d_in: int, d_iparams: int, d_forces: int, d_info: int, stream: int = 0):
        """qmpc_solve_instances_device: device pointers (ints), stream-ordered, no synchronisation."""
        st = self.lib.qmpc_solve_instances_device(self._h, int(batch), C.c_void_p(d_in), C.c_void_p(d_iparams), C.c_void_p(d_forces),
                                                  C.c_void_p(d_info) if d_info else None, C.c_void_p(stream) if stream else None)
        if st != OK:
            raise QmpcError(st, "qmpc_solve_instances_device")

    def solve_schedule(self, inputs: np.ndarray, schedule: np.ndarray, iparams: np.ndarray | None = None, want_traj: bool = False):
        """qmpc_solve_schedule: instance i solved with the stance set schedule[i, k] at knot k (uint8, bit l: leg l stands; the
        record's contacts are not read) and, with iparams (INSTANCE_PARAMS_DTYPE), its own robot and cost record -- None: the
        handle's values.  Returns (forces [B,12], info) or, with want_traj, also traj_u [B,N,12] and traj_x [B,N+1,13]."""
        inputs = np.ascontiguousarray(inputs, dtype=INPUT_DTYPE)
        B, N = inputs.shape[0], self.params.horizon
        schedule = np.ascontiguousarray(schedule, dtype=np.uint8)
        if schedule.shape != (B, N):
            raise ValueError(f"schedule: shape {schedule.shape}, expected ({B}, {N})")
        if iparams is not None:
            iparams = np.ascontiguousarray(iparams, dtype=INSTANCE_PARAMS_DTYPE)
            if iparams.shape != (B,):
                raise ValueError(f"iparams: shape {iparams.shape}, expected ({B},)")
        forces = np.zeros((B, NU), dtype=np.float64)
        info = np.zeros(B, dtype=INFO_DTYPE)
        tu = np.zeros((B, N, NU)) if want_traj else None
        tx = np.zeros((B, N + 1, NX)) if want_traj else None
        st = self.lib.qmpc_solve_schedule(self._h, B, _ptr(inputs), _ptr(iparams), _ptr(schedule), _ptr(forces), _ptr(info), _ptr(tu), _ptr(tx))
        if st != OK:
            raise QmpcError(st, "qmpc_solve_schedule")
        return (forces, info, tu, tx) if want_traj else (forces, info)

    def solve_schedule_device(self, batch: int, d_in: int, d_iparams: int, d_schedule: int, d_forces: int, d_info: int = 0,
                              d_traj_u: int = 0, d_traj_x: int = 0, stream: int = 0):
        """qmpc_solve_schedule_device: device pointers (ints; 0 for an optional one), stream-ordered, no synchronisation."""
        opt = lambda a: C.c_void_p(a) if a else None      # noqa: E731
        st = self.lib.qmpc_solve_schedule_device(self._h, int(batch), C.c_void_p(d_in), opt(d_iparams), C.c_void_p(d_schedule),
                                                 C.c_void_p(d_forces), opt(d_info), opt(d_traj_u), opt(d_traj_x), opt(stream))
        if st != OK:
            raise QmpcError(st, "qmpc_solve_schedule_device")

    def kernel_for_schedule(self, batch: int) -> str:
        return KERNEL_FAMILY[self.query(QUERY_KERNEL_FOR_SCHEDULE, batch)]

    def loop_run_instances(self, states: np.ndarray, ticks: int, lp: LoopParams | None = None, ctrl: np.ndarray | None = None,
                           plant: np.ndarray | None = None, trace: bool = False):
        """qmpc_loop_run_instances: `ticks` ticks of the closed loop, robot i with controller ctrl[i] (INSTANCE_PARAMS_DTYPE; None:
        the handle's) and TRUE plant plant[i] (PLANT_PARAMS_DTYPE; None: the controller's robot, no disturbance).  Returns the
        final states (and, with trace, forces [ticks][B][12] and contacts [ticks][B][4]), as loop_run."""
        lp = lp or default_loop_params(self.lib)
        st = np.ascontiguousarray(states, dtype=LOOP_STATE_DTYPE).copy()
        B = st.shape[0]
        if ctrl is not None:
            ctrl = np.ascontiguousarray(ctrl, dtype=INSTANCE_PARAMS_DTYPE)
            if ctrl.shape != (B,):
                raise ValueError(f"ctrl: shape {ctrl.shape}, expected ({B},)")
        if plant is not None:
            plant = np.ascontiguousarray(plant, dtype=PLANT_PARAMS_DTYPE)
            if plant.shape != (B,):
                raise ValueError(f"plant: shape {plant.shape}, expected ({B},)")
        tf = np.zeros((ticks, B, 12)) if trace else None
        tc = np.zeros((ticks, B, 4)) if trace else None
        rc = self.lib.qmpc_loop_run_instances(self._h, C.byref(lp), B, _ptr(st), int(ticks), _ptr(ctrl), _ptr(plant), _ptr(tf), _ptr(tc))
        if rc != OK:
            raise QmpcError(rc, "qmpc_loop_run_instances")
        return (st, tf, tc) if trace else st

    def loop_run_instances_device(self, batch: int, d_states: int, ticks: int, lp: LoopParams | None = None, d_ctrl: int = 0,
                                  d_plant: int = 0, d_trace_forces: int = 0, d_trace_contacts: int = 0, stream: int = 0):
        """qmpc_loop_run_instances_device: device pointers (ints; 0 = NULL), stream-ordered."""
        lp = lp or default_loop_params(self.lib)
        p = lambda v: C.c_void_p(v) if v else None      # noqa: E731
        rc = self.lib.qmpc_loop_run_instances_device(self._h, C.byref(lp), int(batch), p(d_states), int(ticks), p(d_ctrl), p(d_plant),
                                                     p(d_trace_forces), p(d_trace_contacts), p(stream))
        if rc != OK:
            raise QmpcError(rc, "qmpc_loop_run_instances_device")

    def _loop_run_records(self, name, states, ticks, lp, op, trace, ctrl=None, plant=None, outcomes=None, push=None, ground=None,
                          tallies=None, act=None, lines=None, sense=None, seen=None, want_seen=True, gait=None, geom=None,
                          motor=None, mtallies=None, want_motor_tallies=True):
        """The host-buffer call qmpc_loop_run_<name> of loop_run_outcomes .. loop_run_motors: the records coerced and checked for
        shape (B,), the windows as [B][per_robot], the accumulators the entry point takes -- the caller's, copied, or fresh ones
        -- and the traces.  Returns states, (outcomes, tallies, lines, seen, motor_tallies) with None for what the entry point
        does not take, and (forces, contacts) or ()."""
        lp = lp or default_loop_params(self.lib)
        op = op or default_outcome_params(self.lib)
        st = np.ascontiguousarray(states, dtype=LOOP_STATE_DTYPE).copy()
        B = st.shape[0]
        n = _LOOP_RECORD_ARGS[name]

        def records(a, dtype, what, copy=False):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dtype)
            if a.shape != (B,):
                raise ValueError(f"{what}: shape {a.shape}, expected ({B},)")
            return a.copy() if copy else a

        ctrl = records(ctrl, INSTANCE_PARAMS_DTYPE, "ctrl")
        plant = records(plant, PLANT_PARAMS_DTYPE, "plant")
        ground = records(ground, GROUND_PARAMS_DTYPE, "ground")
        act = records(act, ACTUATION_PARAMS_DTYPE, "act")
        sense = records(sense, SENSE_PARAMS_DTYPE, "sense")
        gait = records(gait, GAIT_PARAMS_DTYPE, "gait")
        motor = records(motor, MOTOR_PARAMS_DTYPE, "motor")
        per_robot = 0
        if push is not None:
            push = np.ascontiguousarray(push, dtype=PUSH_PARAMS_DTYPE)
            if push.ndim == 1:
                push = push.reshape(-1, 1)
            if push.ndim != 2 or push.shape[0] != B:
                raise ValueError(f"push: shape {push.shape}, expected ({B}, per_robot)")
            per_robot = push.shape[1]      # 0 or above QMPC_MAX_PUSHES: the library refuses (QMPC_BAD_ARGUMENT)
            if per_robot == 0:
                push = np.zeros((B, 1), dtype=PUSH_PARAMS_DTYPE)      # a non-NULL pointer for the library to refuse
        oc = loop_outcomes(B, self.lib) if outcomes is None else records(outcomes, LOOP_OUTCOME_DTYPE, "outcomes", copy=True)
        ta = li = sn = mt = None
        if n >= 6:
            ta = ground_tallies(B) if tallies is None else records(tallies, GROUND_TALLY_DTYPE, "tallies", copy=True)
        if n >= 8:
            li = actuation_lines(B) if lines is None else records(lines, ACTUATION_LINE_DTYPE, "lines", copy=True)
        if n >= 10:
            sn = sense_seen(B) if seen is None else records(seen, SENSE_SEEN_DTYPE, "seen", copy=True)
        if n >= 14:
            mt = motor_tallies(B, self.lib) if mtallies is None else records(mtallies, MOTOR_TALLY_DTYPE, "mtallies", copy=True)
        tf = np.zeros((ticks, B, 12)) if trace else None
        tc = np.zeros((ticks, B, 4)) if trace else None
        tail = (C.byref(op), _ptr(oc), _ptr(push), int(per_robot), _ptr(ground), _ptr(ta), _ptr(act), _ptr(li), _ptr(sense),
                _ptr(sn) if want_seen else None, _ptr(gait), C.byref(geom) if geom is not None else None, _ptr(motor),
                _ptr(mt) if want_motor_tallies else None)
        fn = "qmpc_loop_run_" + name
        rc = getattr(self.lib, fn)(self._h, C.byref(lp), B, _ptr(st), int(ticks), _ptr(ctrl), _ptr(plant), _ptr(tf), _ptr(tc), *tail[:n])
        if rc != OK:
            raise QmpcError(rc, fn)
        return st, (oc, ta, li, sn, mt), ((tf, tc) if trace else ())

    def _loop_run_records_device(self, name, batch, d_states, ticks, lp, op, d_ctrl, d_plant, d_trace_forces, d_trace_contacts, stream,
                                 d_outcomes, d_push=0, pushes_per_robot=0, d_ground=0, d_tally=0, d_act=0, d_line=0, d_sense=0,
                                 d_seen=0, d_gait=0, geom=None, d_motor=0, d_motor_tally=0):
        """The device-buffer call qmpc_loop_run_<name>_device of loop_run_outcomes_device .. loop_run_motors_device: device
        pointers (ints; 0 = NULL), of which the entry point gets those it takes."""
        lp = lp or default_loop_params(self.lib)
        op = op or default_outcome_params(self.lib)
        p = lambda v: C.c_void_p(v) if v else None      # noqa: E731
        tail = (C.byref(op), p(d_outcomes), p(d_push), int(pushes_per_robot), p(d_ground), p(d_tally), p(d_act), p(d_line), p(d_sense),
                p(d_seen), p(d_gait), C.byref(geom) if geom is not None else None, p(d_motor), p(d_motor_tally))
        fn = "qmpc_loop_run_" + name + "_device"
        rc = getattr(self.lib, fn)(self._h, C.byref(lp), int(batch), p(d_states), int(ticks), p(d_ctrl), p(d_plant), p(d_trace_forces),
                                   p(d_trace_contacts), *tail[:_LOOP_RECORD_ARGS[name]], p(stream))
        if rc != OK:
            raise QmpcError(rc, fn)

    def loop_run_outcomes(self, states: np.ndarray, ticks: int, lp: LoopParams | None = None, ctrl: np.ndarray | None = None,
                          plant: np.ndarray | None = None, op: OutcomeParams | None = None, outcomes: np.ndarray | None = None,
                          trace: bool = False):
        """qmpc_loop_run_outcomes: loop_run_instances that also accumulates one outcome record per robot (LOOP_OUTCOME_DTYPE) on
        the device.  outcomes: the records to go on accumulating into (None: empty ones); op: default_outcome_params().  Returns
        (states, outcomes[, forces, contacts]); the arguments are not modified."""
        st, acc, tr = self._loop_run_records(
            "outcomes", states, ticks, lp, op, trace, ctrl=ctrl, plant=plant, outcomes=outcomes)
        return (st, *acc[:1], *tr)

    def loop_run_outcomes_device(self, batch: int, d_states: int, ticks: int, d_outcomes: int, lp: LoopParams | None = None,
                                 op: OutcomeParams | None = None, d_ctrl: int = 0, d_plant: int = 0, d_trace_forces: int = 0,
                                 d_trace_contacts: int = 0, stream: int = 0):
        """qmpc_loop_run_outcomes_device: device pointers (ints; 0 = NULL), stream-ordered."""
        self._loop_run_records_device(
            "outcomes", batch, d_states, ticks, lp, op, d_ctrl, d_plant, d_trace_forces, d_trace_contacts, stream, d_outcomes)

    def loop_run_pushes(self, states: np.ndarray, ticks: int, push: np.ndarray | None, lp: LoopParams | None = None,
                        ctrl: np.ndarray | None = None, plant: np.ndarray | None = None, op: OutcomeParams | None = None,
                        outcomes: np.ndarray | None = None, trace: bool = False):
        """qmpc_loop_run_pushes: loop_run_outcomes whose plant integrates under timed push windows per robot.  push:
        [B][per_robot] (or [B]: one window each) PUSH_PARAMS_DTYPE records, push_params(); None: exactly loop_run_outcomes.
        Returns what loop_run_outcomes returns; the arguments are not modified."""
        st, acc, tr = self._loop_run_records(
            "pushes", states, ticks, lp, op, trace, ctrl=ctrl, plant=plant, outcomes=outcomes, push=push)
        return (st, *acc[:1], *tr)

    def loop_run_pushes_device(self, batch: int, d_states: int, ticks: int, d_outcomes: int, d_push: int, pushes_per_robot: int,
                               lp: LoopParams | None = None, op: OutcomeParams | None = None, d_ctrl: int = 0, d_plant: int = 0,
                               d_trace_forces: int = 0, d_trace_contacts: int = 0, stream: int = 0):
        """qmpc_loop_run_pushes_device: device pointers (ints; 0 = NULL), stream-ordered; d_push is read in place."""
        self._loop_run_records_device(
            "pushes", batch, d_states, ticks, lp, op, d_ctrl, d_plant, d_trace_forces, d_trace_contacts, stream, d_outcomes,
            d_push=d_push, pushes_per_robot=pushes_per_robot)

    def loop_run_ground(self, states: np.ndarray, ticks: int, ground: np.ndarray | None, push: np.ndarray | None = None,
                        lp: LoopParams | None = None, ctrl: np.ndarray | None = None, plant: np.ndarray | None = None,
                        op: OutcomeParams | None = None, outcomes: np.ndarray | None = None, tallies: np.ndarray | None = None,
                        trace: bool = False):
        """qmpc_loop_run_ground: loop_run_pushes whose plant integrates under the force the robot's TRUE ground delivers.
        ground: [B] GROUND_PARAMS_DTYPE records, ground_params(); None: exactly loop_run_pushes (the tallies come back as given).
        tallies: the GROUND_TALLY_DTYPE records to go on accumulating into (None: empty ones).  Returns (states, outcomes,
        tallies[, forces, contacts]); the arguments are not modified."""
        st, acc, tr = self._loop_run_records(
            "ground", states, ticks, lp, op, trace, ctrl=ctrl, plant=plant, outcomes=outcomes, push=push, ground=ground,
            tallies=tallies)
        return (st, *acc[:2], *tr)

    def loop_run_ground_device(self, batch: int, d_states: int, ticks: int, d_outcomes: int, d_ground: int, d_tally: int = 0,
                               d_push: int = 0, pushes_per_robot: int = 0, lp: LoopParams | None = None,
                               op: OutcomeParams | None = None, d_ctrl: int = 0, d_plant: int = 0, d_trace_forces: int = 0,
                               d_trace_contacts: int = 0, stream: int = 0):
        """qmpc_loop_run_ground_device: device pointers (ints; 0 = NULL), stream-ordered; d_ground and d_push are read in place,
        d_tally (or 0) is read and written."""
        self._loop_run_records_device(
            "ground", batch, d_states, ticks, lp, op, d_ctrl, d_plant, d_trace_forces, d_trace_contacts, stream, d_outcomes,
            d_push=d_push, pushes_per_robot=pushes_per_robot, d_ground=d_ground, d_tally=d_tally)

    def loop_run_actuation(self, states: np.ndarray, ticks: int, act: np.ndarray | None, lines: np.ndarray | None = None,
                           ground: np.ndarray | None = None, push: np.ndarray | None = None, lp: LoopParams | None = None,
                           ctrl: np.ndarray | None = None, plant: np.ndarray | None = None, op: OutcomeParams | None = None,
                           outcomes: np.ndarray | None = None, tallies: np.ndarray | None = None, trace: bool = False):
        """qmpc_loop_run_actuation: loop_run_ground whose plant receives each robot's command of delay_ticks ticks ago through
        its first-order actuator.  act: [B] ACTUATION_PARAMS_DTYPE records, actuation_params(); None: exactly loop_run_ground
        (the lines come back as given).  lines: the ACTUATION_LINE_DTYPE records to go on from (None: actuation_lines(B), zeros).
        ground may be None (no clamp).  Returns (states, outcomes, tallies, lines[, forces, contacts]); the arguments are not
        modified."""
        st, acc, tr = self._loop_run_records(
            "actuation", states, ticks, lp, op, trace, ctrl=ctrl, plant=plant, outcomes=outcomes, push=push, ground=ground,
            tallies=tallies, act=act, lines=lines)
        return (st, *acc[:3], *tr)

    def loop_run_actuation_device(self, batch: int, d_states: int, ticks: int, d_outcomes: int, d_act: int, d_line: int,
                                  d_ground: int = 0, d_tally: int = 0, d_push: int = 0, pushes_per_robot: int = 0,
                                  lp: LoopParams | None = None, op: OutcomeParams | None = None, d_ctrl: int = 0, d_plant: int = 0,
                                  d_trace_forces: int = 0, d_trace_contacts: int = 0, stream: int = 0):
        """qmpc_loop_run_actuation_device: device pointers (ints; 0 = NULL), stream-ordered; d_act, d_ground and d_push are read in
        place, d_line and d_tally (or 0) are read and written."""
        self._loop_run_records_device(
            "actuation", batch, d_states, ticks, lp, op, d_ctrl, d_plant, d_trace_forces, d_trace_contacts, stream, d_outcomes,
            d_push=d_push, pushes_per_robot=pushes_per_robot, d_ground=d_ground, d_tally=d_tally, d_act=d_act, d_line=d_line)

    def loop_run_sensing(self, states: np.ndarray, ticks: int, sense: np.ndarray | None, seen: np.ndarray | None = None,
                         act: np.ndarray | None = None, lines: np.ndarray | None = None, ground: np.ndarray | None = None,
                         push: np.ndarray | None = None, lp: LoopParams | None = None, ctrl: np.ndarray | None = None,
                         plant: np.ndarray | None = None, op: OutcomeParams | None = None, outcomes: np.ndarray | None = None,
                         tallies: np.ndarray | None = None, trace: bool = False, want_seen: bool = True):
        """qmpc_loop_run_sensing: loop_run_actuation whose controller reads each robot's MEASURED state -- the true one plus the
        record's bias and reproducible bounded noise -- while plant, outcome record, pushes, ground and actuation work on the
        truth.  sense: [B] SENSE_PARAMS_DTYPE records, sense_params(); None: exactly loop_run_actuation (seen comes back as
        given).  seen: the SENSE_SEEN_DTYPE records to go on from (None: sense_seen(B)); want_seen=False passes NULL.  act may be
        None (every command acts in its own tick; the lines come back as given), ground may be None (no clamp).  Returns (states,
        outcomes, tallies, lines, seen[, forces, contacts]); the arguments are not modified."""
        st, acc, tr = self._loop_run_records(
            "sensing", states, ticks, lp, op, trace, ctrl=ctrl, plant=plant, outcomes=outcomes, push=push, ground=ground,
            tallies=tallies, act=act, lines=lines, sense=sense, seen=seen, want_seen=want_seen)
        return (st, *acc[:4], *tr)

    def loop_run_sensing_device(self, batch: int, d_states: int, ticks: int, d_outcomes: int, d_sense: int, d_seen: int = 0,
                                d_act: int = 0, d_line: int = 0, d_ground: int = 0, d_tally: int = 0, d_push: int = 0,
                                pushes_per_robot: int = 0, lp: LoopParams | None = None, op: OutcomeParams | None = None,
                                d_ctrl: int = 0, d_plant: int = 0, d_trace_forces: int = 0, d_trace_contacts: int = 0, stream: int = 0):
        """qmpc_loop_run_sensing_device: device pointers (ints; 0 = NULL), stream-ordered; d_sense, d_act, d_ground and d_push are
        read in place, d_seen (or 0), d_line and d_tally (or 0) are read and written."""
        self._loop_run_records_device(
            "sensing", batch, d_states, ticks, lp, op, d_ctrl, d_plant, d_trace_forces, d_trace_contacts, stream, d_outcomes,
            d_push=d_push, pushes_per_robot=pushes_per_robot, d_ground=d_ground, d_tally=d_tally, d_act=d_act, d_line=d_line,
            d_sense=d_sense, d_seen=d_seen)

    def loop_run_gaits(self, states: np.ndarray, ticks: int, gait: np.ndarray | None, sense: np.ndarray | None = None,
                       seen: np.ndarray | None = None, act: np.ndarray | None = None, lines: np.ndarray | None = None,
                       ground: np.ndarray | None = None, push: np.ndarray | None = None, lp: LoopParams | None = None,
                       ctrl: np.ndarray | None = None, plant: np.ndarray | None = None, op: OutcomeParams | None = None,
                       outcomes: np.ndarray | None = None, tallies: np.ndarray | None = None, trace: bool = False,
                       want_seen: bool = True):
        """qmpc_loop_run_gaits: loop_run_sensing in which every robot walks its own gait -- frequency, contact pattern, split and
        starting phase per leg.  gait: [B] GAIT_PARAMS_DTYPE records, gait_params(); None: exactly loop_run_sensing.  Every other
        record may be None as there.  The schedule lives in the states (leg, contacts, gait_counter): there is no record to carry
        over calls, and a record changed between calls takes effect at each leg's next transition (phase0 at the next reset).
        Returns (states, outcomes, tallies, lines, seen[, forces, contacts]); the arguments are not modified."""
        st, acc, tr = self._loop_run_records(
            "gaits", states, ticks, lp, op, trace, ctrl=ctrl, plant=plant, outcomes=outcomes, push=push, ground=ground,
            tallies=tallies, act=act, lines=lines, sense=sense, seen=seen, want_seen=want_seen, gait=gait)
        return (st, *acc[:4], *tr)

    def loop_run_gaits_device(self, batch: int, d_states: int, ticks: int, d_outcomes: int, d_gait: int, d_sense: int = 0,
                              d_seen: int = 0, d_act: int = 0, d_line: int = 0, d_ground: int = 0, d_tally: int = 0, d_push: int = 0,
                              pushes_per_robot: int = 0, lp: LoopParams | None = None, op: OutcomeParams | None = None,
                              d_ctrl: int = 0, d_plant: int = 0, d_trace_forces: int = 0, d_trace_contacts: int = 0, stream: int = 0):
        """qmpc_loop_run_gaits_device: device pointers (ints; 0 = NULL), stream-ordered; d_gait, d_sense, d_act, d_ground and
        d_push are read in place, d_seen (or 0), d_line and d_tally (or 0) are read and written."""
        self._loop_run_records_device(
            "gaits", batch, d_states, ticks, lp, op, d_ctrl, d_plant, d_trace_forces, d_trace_contacts, stream, d_outcomes,
            d_push=d_push, pushes_per_robot=pushes_per_robot, d_ground=d_ground, d_tally=d_tally, d_act=d_act, d_line=d_line,
            d_sense=d_sense, d_seen=d_seen, d_gait=d_gait)

    def loop_run_motors(self, states: np.ndarray, ticks: int, motor: np.ndarray | None, mtallies: np.ndarray | None = None,
                        geom: "LegGeometry | None" = None, gait: np.ndarray | None = None, sense: np.ndarray | None = None,
                        seen: np.ndarray | None = None, act: np.ndarray | None = None, lines: np.ndarray | None = None,
                        ground: np.ndarray | None = None, push: np.ndarray | None = None, lp: LoopParams | None = None,
                        ctrl: np.ndarray | None = None, plant: np.ndarray | None = None, op: OutcomeParams | None = None,
                        outcomes: np.ndarray | None = None, tallies: np.ndarray | None = None, trace: bool = False,
                        want_seen: bool = True, want_motor_tallies: bool = True):
        """qmpc_loop_run_motors: loop_run_gaits in which the foot force a stance leg delivers respects the joint torque limits of
        the robot's motors, and which records the torque every joint was asked for.  motor: [B] MOTOR_PARAMS_DTYPE records,
        motor_params(); None: exactly loop_run_gaits.  mtallies: [B] MOTOR_TALLY_DTYPE, carried over calls (None: fresh ones
        of module-level motor_tallies()); geom: one LegGeometry for all robots (None: the Go1's).  Every other record may be None
        as there.  Returns (states, outcomes, tallies, lines, seen, motor_tallies[, forces, contacts]); the arguments are not
        modified."""
        st, acc, tr = self._loop_run_records(
            "motors", states, ticks, lp, op, trace, ctrl=ctrl, plant=plant, outcomes=outcomes, push=push, ground=ground,
            tallies=tallies, act=act, lines=lines, sense=sense, seen=seen, want_seen=want_seen, gait=gait, geom=geom,
            motor=motor, mtallies=mtallies, want_motor_tallies=want_motor_tallies)
        return (st, *acc[:5], *tr)

    def loop_run_motors_device(self, batch: int, d_states: int, ticks: int, d_outcomes: int, d_motor: int, d_motor_tally: int,
                               geom: "LegGeometry | None" = None, d_gait: int = 0, d_sense: int = 0, d_seen: int = 0, d_act: int = 0,
                               d_line: int = 0, d_ground: int = 0, d_tally: int = 0, d_push: int = 0, pushes_per_robot: int = 0,
                               lp: LoopParams | None = None, op: OutcomeParams | None = None, d_ctrl: int = 0, d_plant: int = 0,
                               d_trace_forces: int = 0, d_trace_contacts: int = 0, stream: int = 0):
        """qmpc_loop_run_motors_device: device pointers (ints; 0 = NULL), stream-ordered; geom is a host record (None: the Go1's);
        d_motor, d_gait, d_sense, d_act, d_ground and d_push are read in place, d_motor_tally, d_seen (or 0), d_line and d_tally
        (or 0) are read and written."""
        self._loop_run_records_device(
            "motors", batch, d_states, ticks, lp, op, d_ctrl, d_plant, d_trace_forces, d_trace_contacts, stream, d_outcomes,
            d_push=d_push, pushes_per_robot=pushes_per_robot, d_ground=d_ground, d_tally=d_tally, d_act=d_act, d_line=d_line,
            d_sense=d_sense, d_seen=d_seen, d_gait=d_gait, geom=geom, d_motor=d_motor, d_motor_tally=d_motor_tally)

    def loop_instances_plan(self, batch: int, ctrl: bool = False, warm: bool = False):
        """The launch qmpc_loop_run_instances* takes for `batch` robots: (form, family) -- form "persistent" / "per_tick", family
        as KERNEL_FAMILY -- or None where the call is refused (QMPC_QUERY_LOOP_INSTANCES_PLAN).  Answers under the handle's
        instances policy: with ctrl under "auto" the per-tick form is ("per_tick", "lane_handoff" / "lane") from the switch-over on.
        ctrl and warm together answer under set_loop_warm_records (default off: None; a ConvexMpc
        handle: under set_convex_warm_records)."""
        v = self.query(QUERY_LOOP_INSTANCES_PLAN, int(batch) | (int(bool(ctrl)) << 32) | (int(bool(warm)) << 33))
        if v == 0:
            return None
        return ({1: "persistent", 2: "per_tick"}[v // 16], KERNEL_FAMILY[v % 16])

    def kernel_for_instances(self, batch: int) -> str:
        return KERNEL_FAMILY[self.query(QUERY_KERNEL_FOR_INSTANCES, batch)]

    def set_instances_policy(self, policy: str | int):
        """Which kernel family solve_instances* and the ticks of loop_run_instances* / loop_run_outcomes* with controller records
        may take on this handle (qmpc_set_instances_policy): "wave" (default: the wave wrench-form kernels at every size) or
        "auto" (lane per instance with the straggler hand-off from the switch-over on).  prepare() allocates for the policy set."""
        value = INSTANCES_POLICY[policy] if isinstance(policy, str) else int(policy)
        st = self.lib.qmpc_set_instances_policy(self._h, value)
        if st != OK:
            raise QmpcError(st, "qmpc_set_instances_policy")

    def set_loop_warm_records(self, on: bool = True):
        """Let the loops with controller records (loop_run_instances* / loop_run_outcomes* / loop_run_pushes* with ctrl) accept
        lp.warm_start on this handle (qmpc_set_loop_warm_records; default off: they refuse it).  Holds until it is changed."""
        st = self.lib.qmpc_set_loop_warm_records(self._h, int(on))
        if st != OK:
            raise QmpcError(st, "qmpc_set_loop_warm_records")

    def loop_warm_records(self) -> bool:
        return bool(self.query(QUERY_LOOP_WARM_RECORDS))

    def set_convex_records(self, on: bool = True):
        """Let loop_run_instances* / loop_run_outcomes* / loop_run_pushes* accept this ConvexMpc handle (converged mode) with
        per-robot controller and plant records, outcome records and push windows (qmpc_set_convex_records; default off: they
        refuse it).  Holds until it is changed; does nothing on a handle of another model."""
        st = self.lib.qmpc_set_convex_records(self._h, int(on))
        if st != OK:
            raise QmpcError(st, "qmpc_set_convex_records")

    def convex_records(self) -> bool:
        return bool(self.query(QUERY_CONVEX_RECORDS))

    def set_convex_lane_records(self, on: bool = True):
        """Let ConvexMpc's calls with per-instance records (convex_solve_instances*, and with set_convex_records the ticks of the
        record loops with ctrl) take the lane-per-instance kernel with per-lane parameters from the switch-over on, under
        set_instances_policy(INSTANCES_AUTO) (qmpc_set_convex_lane_records; default off: the wave kernels at every size).  It
        does nothing on a handle of another model."""
        st = self.lib.qmpc_set_convex_lane_records(self._h, int(on))
        if st != OK:
            raise QmpcError(st, "qmpc_set_convex_lane_records")

    def convex_lane_records(self) -> bool:
        return bool(self.query(QUERY_CONVEX_LANE_RECORDS))

    def set_convex_warm_records(self, on: bool = True):
        """Let the loops with controller records accept lp.warm_start on this ConvexMpc handle (qmpc_set_convex_warm_records;
        default off: they refuse it).  Takes effect only together with set_convex_records; set_loop_warm_records keeps having
        no effect on ConvexMpc, and this setting does nothing on a handle of another model."""
        st = self.lib.qmpc_set_convex_warm_records(self._h, int(on))
        if st != OK:
            raise QmpcError(st, "qmpc_set_convex_warm_records")

    def convex_warm_records(self) -> bool:
        return bool(self.query(QUERY_CONVEX_WARM_RECORDS))

    def instances_policy(self) -> str:
        return {v: k for k, v in INSTANCES_POLICY.items()}[self.query(QUERY_INSTANCES_POLICY)]

    def prepare_instances(self):
        """Allocate the per-instance buffers now (qmpc_prepare_instances)."""
        st = self.lib.qmpc_prepare_instances(self._h)
        if st != OK:
            raise QmpcError(st, "qmpc_prepare_instances")

    def solve_async(self, inputs: np.ndarray, forces: np.ndarray, info: np.ndarray = None):
        """Host buffers, non-blocking (qmpc_solve_async); the arrays must stay alive until wait()."""
        assert inputs.dtype == INPUT_DTYPE and inputs.flags.c_contiguous and forces.flags.c_contiguous
        st = self.lib.qmpc_solve_async(self._h, inputs.shape[0], _ptr(inputs), _ptr(forces),
                                       _ptr(info) if info is not None else None)
        if st != OK:
            raise QmpcError(st, "qmpc_solve_async")

    def gather(self, nccl_comm: int, d_local: int, count: int, d_all: int, stream: int = 0):
        """ncclAllGather of `count` doubles per rank (qmpc_gather); nccl_comm is the caller's ncclComm_t."""
        st = self.lib.qmpc_gather(self._h, C.c_void_p(nccl_comm), C.c_void_p(d_local), int(count),
                                  C.c_void_p(d_all), C.c_void_p(stream) if stream else None)
        if st != OK:
            raise QmpcError(st, "qmpc_gather")

    def wait(self):
        st = self.lib.qmpc_wait(self._h)
        if st != OK:
            raise QmpcError(st, "qmpc_wait")

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        st = self.lib.qmpc_last_kernel_ms(self._h, C.byref(ms))
        if st != OK:
            raise QmpcError(st, "qmpc_last_kernel_ms")
        return float(ms.value)

    # ---- 8 contact points (handle created with params.model = MODEL_QUAT8) ----
    def solve8(self, inputs: np.ndarray, want_traj: bool = False):
        inputs = np.ascontiguousarray(inputs, dtype=INPUT8_DTYPE)
        B, N = inputs.shape[0], self.params.horizon
        forces = np.zeros((B, 24), dtype=np.float64)
        info = np.zeros(B, dtype=INFO_DTYPE)
        if want_traj:
            tu = np.zeros((B, N, 24))
            tx = np.zeros((B, N + 1, NX))
            st = self.lib.qmpc_solve8_traj(self._h, B, _ptr(inputs), _ptr(forces), _ptr(info), _ptr(tu), _ptr(tx))
            if st != OK:
                raise QmpcError(st, "qmpc_solve8_traj")
            return forces, info, tu, tx
        st = self.lib.qmpc_solve8(self._h, B, _ptr(inputs), _ptr(forces), _ptr(info))
        if st != OK:
            raise QmpcError(st, "qmpc_solve8")
        return forces, info

    def solve8_device(self, batch: int, d_in: int, d_forces: int, d_info: int, stream: int = 0):
        st = self.lib.qmpc_solve8_device(self._h, int(batch), C.c_void_p(d_in), C.c_void_p(d_forces),
                                         C.c_void_p(d_info) if d_info else None,
                                         C.c_void_p(stream) if stream else None)
        if st != OK:
            raise QmpcError(st, "qmpc_solve8_device")

    # ---- ConvexMpc model (handle created with params.model = MODEL_CONVEX) ----
    def convex_solve(self, inputs: np.ndarray, want_traj: bool = False):
        """World-frame forces of legged::ConvexMpc::grf_update's problem, host buffers."""
        inputs = np.ascontiguousarray(inputs, dtype=CONVEX_INPUT_DTYPE)
        B, N = inputs.shape[0], self.params.horizon
        forces = np.zeros((B, NU), dtype=np.float64)
        info = np.zeros(B, dtype=INFO_DTYPE)
        if want_traj:
            tu = np.zeros((B, N, NU))
            tx = np.zeros((B, N + 1, 12))
            st = self.lib.qmpc_convex_solve_traj(self._h, B, _ptr(inputs), _ptr(forces), _ptr(info), _ptr(tu), _ptr(tx))
            if st != OK:
                raise QmpcError(st, "qmpc_convex_solve_traj")
            return forces, info, tu, tx
        st = self.lib.qmpc_convex_solve(self._h, B, _ptr(inputs), _ptr(forces), _ptr(info))
        if st != OK:
            raise QmpcError(st, "qmpc_convex_solve")
        return forces, info

    def convex_solve_device(self, batch: int, d_in: int, d_forces: int, d_info: int, stream: int = 0):
        st = self.lib.qmpc_convex_solve_device(self._h, int(batch), C.c_void_p(d_in), C.c_void_p(d_forces),
                                               C.c_void_p(d_info) if d_info else None,
                                               C.c_void_p(stream) if stream else None)
        if st != OK:
            raise QmpcError(st, "qmpc_convex_solve_device")

    def convex_solve_instances(self, inputs: np.ndarray, iparams: np.ndarray, want_traj: bool = False):
        """qmpc_convex_solve_instances: ConvexMpc's problem, instance i solved with the handle's parameters and the fields of
        iparams[i] (INSTANCE_PARAMS_DTYPE; q_weights[12] and w are validated but unused).  Returns (forces_world [B,12], info) or,
        with want_traj, also traj_u [B,N,12] and traj_x [B,N+1,12]."""
        inputs = np.ascontiguousarray(inputs, dtype=CONVEX_INPUT_DTYPE)
        iparams = np.ascontiguousarray(iparams, dtype=INSTANCE_PARAMS_DTYPE)
        B, N = inputs.shape[0], self.params.horizon
        if iparams.shape != (B,):
            raise ValueError(f"iparams: shape {iparams.shape}, expected ({B},)")
        forces = np.zeros((B, NU), dtype=np.float64)
        info = np.zeros(B, dtype=INFO_DTYPE)
        tu = np.zeros((B, N, NU)) if want_traj else None
        tx = np.zeros((B, N + 1, 12)) if want_traj else None
        st = self.lib.qmpc_convex_solve_instances(self._h, B, _ptr(inputs), _ptr(iparams), _ptr(forces), _ptr(info), _ptr(tu), _ptr(tx))
        if st != OK:
            raise QmpcError(st, "qmpc_convex_solve_instances")
        return (forces, info, tu, tx) if want_traj else (forces, info)

    def convex_solve_instances_device(self, batch: int, d_in: int, d_iparams: int, d_forces: int, d_info: int, stream: int = 0):
        """qmpc_convex_solve_instances_device: device pointers (ints), stream-ordered, no synchronisation."""
        st = self.lib.qmpc_convex_solve_instances_device(self._h, int(batch), C.c_void_p(d_in), C.c_void_p(d_iparams),
                                                         C.c_void_p(d_forces), C.c_void_p(d_info) if d_info else None,
                                                         C.c_void_p(stream) if stream else None)
        if st != OK:
            raise QmpcError(st, "qmpc_convex_solve_instances_device")

    def kernel_for_convex_instances(self, batch: int) -> str:
        """The kernel family convex_solve_instances* launches for a batch size ("none": the handle refuses the call)."""
        return KERNEL_FAMILY[self.query(QUERY_KERNEL_FOR_CONVEX_INSTANCES, batch)]

    def convex_linearize(self, inputs: np.ndarray):
        inputs = np.ascontiguousarray(inputs, dtype=CONVEX_INPUT_DTYPE)
        B, N = inputs.shape[0], self.params.horizon
        A = np.zeros((B, N, 12, 12))
        Bm = np.zeros((B, N, 12, 12))
        X = np.zeros((B, N + 1, 12))
        st = self.lib.qmpc_convex_linearize(self._h, B, _ptr(inputs), _ptr(A), _ptr(Bm), _ptr(X))
        if st != OK:
            raise QmpcError(st, "qmpc_convex_linearize")
        return A, Bm, X

    # ---- force -> joint torque consumer (BaseInterface::tau_ctrl_update) ----
    def default_go1_geometry(self) -> LegGeometry:
        g = LegGeometry()
        self.lib.qmpc_default_go1_geometry(C.byref(g))
        return g

    def leg_kinematics(self, geom: LegGeometry, joint_pos: np.ndarray):
        q = np.ascontiguousarray(joint_pos, dtype=np.float64).reshape(-1, 12)
        p = np.zeros((len(q), 12))
        J = np.zeros((len(q), 4, 9))
        st = self.lib.qmpc_leg_kinematics(self._h, C.byref(geom), len(q), _ptr(q), _ptr(p), _ptr(J))
        if st != OK:
            raise QmpcError(st, "qmpc_leg_kinematics")
        return p, J

    def torque_map(self, geom: LegGeometry, joint_pos, forces_body, contacts=None, walking: bool = True):
        q = np.ascontiguousarray(joint_pos, dtype=np.float64).reshape(-1, 12)
        f = np.ascontiguousarray(forces_body, dtype=np.float64).reshape(-1, 12)
        c = None if contacts is None else np.ascontiguousarray(contacts, dtype=np.float64).reshape(-1, 4)
        tau = np.zeros((len(q), 12))
        st = self.lib.qmpc_torque_map(self._h, C.byref(geom), len(q), _ptr(q), _ptr(f), _ptr(c), int(bool(walking)), _ptr(tau))
        if st != OK:
            raise QmpcError(st, "qmpc_torque_map")
        return tau

    def torque_map_device(self, geom: LegGeometry, batch: int, d_joint_pos: int, d_forces: int, d_contacts: int,
                          walking: bool, d_tau: int, stream: int = 0):
        st = self.lib.qmpc_torque_map_device(self._h, C.byref(geom), int(batch), C.c_void_p(d_joint_pos),
                                             C.c_void_p(d_forces), C.c_void_p(d_contacts) if d_contacts else None,
                                             int(bool(walking)), C.c_void_p(d_tau),
                                             C.c_void_p(stream) if stream else None)
        if st != OK:
            raise QmpcError(st, "qmpc_torque_map_device")

    def leg_inverse_kinematics(self, geom: LegGeometry, foot_pos_body, cur_joint_pos):
        """A1Kinematics::inv_kin for every (instance, leg); NaN where the foot is out of reach."""
        p = np.ascontiguousarray(foot_pos_body, dtype=np.float64).reshape(-1, 12)
        c = np.ascontiguousarray(cur_joint_pos, dtype=np.float64).reshape(-1, 12)
        q = np.zeros((len(p), 12))
        st = self.lib.qmpc_leg_inverse_kinematics(self._h, C.byref(geom), len(p), _ptr(p), _ptr(c), _ptr(q))
        if st != OK:
            raise QmpcError(st, "qmpc_leg_inverse_kinematics")
        return q

    def joint_commands(self, geom: LegGeometry, feedback: np.ndarray) -> np.ndarray:
        """BaseInterface::tau_ctrl_update for a batch of JOINT_FEEDBACK_DTYPE records -> JOINT_COMMAND_DTYPE."""
        fb = np.ascontiguousarray(feedback, dtype=JOINT_FEEDBACK_DTYPE)
        cmd = np.zeros(len(fb), dtype=JOINT_COMMAND_DTYPE)
        st = self.lib.qmpc_joint_commands(self._h, C.byref(geom), len(fb), _ptr(fb), _ptr(cmd))
        if st != OK:
            raise QmpcError(st, "qmpc_joint_commands")
        return cmd

    def joint_commands_device(self, geom: LegGeometry, batch: int, d_fb: int, d_cmd: int, stream: int = 0):
        st = self.lib.qmpc_joint_commands_device(self._h, C.byref(geom), int(batch), C.c_void_p(d_fb), C.c_void_p(d_cmd),
                                                 C.c_void_p(stream) if stream else None)
        if st != OK:
            raise QmpcError(st, "qmpc_joint_commands_device")

    def loop_joint_commands_device(self, geom: LegGeometry, batch: int, d_states: int, d_joint_pos: int, d_fb: int,
                                   d_cmd: int, stream: int = 0):
        """Joint-level feedback (d_fb may be 0) and commands of the robots of a closed loop, from their states."""
        st = self.lib.qmpc_loop_joint_commands_device(self._h, C.byref(geom), int(batch), C.c_void_p(d_states),
                                                      C.c_void_p(d_joint_pos), C.c_void_p(d_fb) if d_fb else None,
                                                      C.c_void_p(d_cmd), C.c_void_p(stream) if stream else None)
        if st != OK:
            raise QmpcError(st, "qmpc_loop_joint_commands_device")

    def loop_joint_commands(self, geom: LegGeometry, states: np.ndarray, joint_pos: np.ndarray | None = None):
        """Host-buffer form: (joint_pos [B][12] updated, feedback records, command records) of the robots' states."""
        st = np.ascontiguousarray(states, dtype=LOOP_STATE_DTYPE)
        B = len(st)
        jp = np.zeros((B, 12))
        if joint_pos is None:
            self.lib.qmpc_loop_joint_init(_ptr(jp), B)
        else:
            jp[:] = np.asarray(joint_pos, dtype=np.float64).reshape(B, 12)
        fb = np.zeros(B, dtype=JOINT_FEEDBACK_DTYPE)
        cmd = np.zeros(B, dtype=JOINT_COMMAND_DTYPE)
        rc = self.lib.qmpc_loop_joint_commands(self._h, C.byref(geom), B, _ptr(st), _ptr(jp), _ptr(fb), _ptr(cmd))
        if rc != OK:
            raise QmpcError(rc, "qmpc_loop_joint_commands")
        return jp, fb, cmd

    def loop_run_joint_device(self, geom: LegGeometry, batch: int, d_states: int, d_joint_pos: int, ticks: int,
                              lp: LoopParams | None = None, d_cmd: int = 0, d_trace_cmd: int = 0, stream: int = 0):
        """`ticks` ticks of the device-resident loop, each closed by the joint-level kernel (inside the captured graph)."""
        lp = lp or default_loop_params(self.lib)
        st = self.lib.qmpc_loop_run_joint_device(self._h, C.byref(lp), C.byref(geom), int(batch), C.c_void_p(d_states),
                                                 C.c_void_p(d_joint_pos), int(ticks), C.c_void_p(d_cmd) if d_cmd else None,
                                                 C.c_void_p(d_trace_cmd) if d_trace_cmd else None,
                                                 C.c_void_p(stream) if stream else None)
        if st != OK:
            raise QmpcError(st, "qmpc_loop_run_joint_device")

    def phase_profile(self, inputs: np.ndarray) -> np.ndarray:
        inputs = np.ascontiguousarray(inputs, dtype=INPUT_DTYPE)
        out = np.zeros((inputs.shape[0], 16), dtype=np.int64)
        st = self.lib.qmpc_debug_profile(self._h, inputs.shape[0], _ptr(inputs), _ptr(out))
        if st != OK:
            raise QmpcError(st, "qmpc_debug_profile")
        return out

    def linearize(self, inputs: np.ndarray):
        inputs = np.ascontiguousarray(inputs, dtype=INPUT_DTYPE)
        B, N = inputs.shape[0], self.params.horizon
        A = np.zeros((B, N, NE, NE))
        Bm = np.zeros((B, N, NE, NU))
        X = np.zeros((B, N + 1, NX))
        st = self.lib.qmpc_linearize(self._h, B, _ptr(inputs), _ptr(A), _ptr(Bm), _ptr(X))
        if st != OK:
            raise QmpcError(st, "qmpc_linearize")
        return A, Bm, X


from .scenarios import (go1_stand_input, quat_to_rot, random_go1_trot_states,  # noqa: E402,F401
                        random_go1_convex_states, random_biped8_states, random_go1_variants, random_go1_convex_variants, random_go1_plants,
                        random_go1_pushes, random_go1_grounds, random_go1_actuations, random_go1_senses, random_go1_gaits,
                        random_go1_motors)
from .sharding import StepPipeline, gather_forces, shard_range, solve_sharded  # noqa: E402,F401
