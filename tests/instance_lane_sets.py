"""Input sets of the per-instance lane path's tests (tests/test_instance_lane_cpu.py, tests/test_gpu_instance_lane.py):
states, per-instance records and the handle's parameters of S1 .. S4, and the sampling rule.  Not a test module."""
import numpy as np

SETS = {"S1": (10, 32768), "S2": (10, 65536), "S3": (20, 65536), "S4": (10, 32768)}


def sample(B, n):
    return np.unique(np.linspace(0, B - 1, n).astype(int))


def input_set(pkg, lib, name):
    """(params of the handle, states [B], records [B])"""
    N, B = SETS[name]
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    if name == "S1":
        return p, pkg.random_go1_trot_states(B, config_id=2), pkg.random_go1_variants(B, seed=13, base=p)
    if name == "S2":
        return p, pkg.random_go1_trot_states(B, config_id=2), pkg.random_go1_variants(B, seed=23, base=p)
    if name == "S3":
        return p, pkg.random_go1_trot_states(B, config_id=3), pkg.random_go1_variants(B, seed=29, base=p)
    # S4: the friction-cone stress set of test_each_instance_keeps_its_own_friction_cone (tests/test_gpu_instance_params.py)
    p.mu = 0.9
    rng = np.random.default_rng(3)
    ip = pkg.instance_params(p, B)
    ip["mu"] = rng.uniform(0.3, 0.5, B)
    ip["fz_max"] = rng.uniform(60.0, 120.0, B)
    rec = pkg.random_go1_trot_states(B, config_id=4, tilt_max=0.5)
    rec["lin_vel_body"] = 0.0
    rec["vel_ref_body"][:, 0] = rng.choice([-2.0, 2.0], B)
    rec["vel_ref_body"][:, 1] = rng.uniform(-1.0, 1.0, B)
    return p, rec, ip


# the ten invalid records of test_bad_records_are_flagged_alone (tests/test_gpu_instance_params.py): index -> (field, value)
BAD_RECORDS = {3: ("mass", np.nan), 10: ("mass", 0.0), 17: ("inertia", 0.0), 24: ("inertia", np.inf), 30: ("r_weights", 0.0),
               41: ("q_weights", -1.0), 50: ("w", -1.0), 60: ("mu", 0.0), 70: ("fz_max", -5.0), 80: ("fz_max", np.nan)}


def plant_bad(records, plant=BAD_RECORDS):
    bad = records.copy()
    for i, (field, v) in plant.items():
        if field in ("r_weights", "q_weights"):
            bad[field][i, 2] = v
        else:
            bad[field][i] = v
    return bad


def cone_violation(rec, ip, f):
    """Largest friction-pyramid and force-bound excess [N] per instance over its stance legs (<= 0: inside)."""
    B = len(rec)
    R = rec["rot"].reshape(B, 3, 3)
    fw = np.einsum("bij,blj->bli", R, f.reshape(B, 4, 3))
    stance = rec["contacts"] > 0
    mu = ip["mu"][:, None]
    fric = np.maximum.reduce([fw[..., 0] - mu * fw[..., 2], -fw[..., 0] - mu * fw[..., 2],
                              fw[..., 1] - mu * fw[..., 2], -fw[..., 1] - mu * fw[..., 2]])
    bound = fw[..., 2] - ip["fz_max"][:, None]
    return np.where(stance, fric, -np.inf).max(axis=1), np.where(stance, bound, -np.inf).max(axis=1)
