"""Input sets of the stance-set tests (tests/test_stance_sets_cpu.py, tests/test_gpu_stance_sets.py,
tests/golden/make_stance_fixtures.py): every non-empty stance set of the four legs, a spread of the 255 of the 8-point model,
and both signs of the two quaternions -- where the state generators draw three trot sets and w > 0 only.  Not a test module.

The CPU suite and the GPU suite build their records here, so both see the same ones."""
import gzip
import itertools
from pathlib import Path

import numpy as np

# the 15 non-empty stance sets of four legs, (FL, FR, RL, RR), in the order of itertools.product: 0001, 0010, ... 1111
MASKS4 = tuple(m for m in itertools.product((0, 1), repeat=4) if any(m))
# 16 of the 255 of the 8-point model (points 0-3 left foot, 4-7 right foot): one point, two, odd counts, a point of each foot,
# half of each foot, all but one, one foot, both
MASKS8 = ((1, 0, 0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0, 1, 0), (1, 1, 0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 1, 0, 1),
          (1, 1, 1, 0, 0, 0, 0, 0), (1, 0, 0, 1, 0, 0, 0, 0), (1, 1, 1, 1, 1, 0, 0, 0), (0, 1, 0, 0, 1, 1, 1, 1),
          (1, 1, 0, 0, 1, 1, 0, 0), (1, 0, 1, 0, 0, 1, 0, 1), (1, 1, 1, 0, 1, 1, 1, 0), (1, 1, 1, 1, 1, 1, 1, 0),
          (0, 1, 1, 1, 1, 1, 1, 1), (1, 1, 1, 1, 0, 0, 0, 0), (0, 0, 0, 0, 1, 1, 1, 1), (1, 1, 1, 1, 1, 1, 1, 1))
# QuatMpc at N = 20: the sets on which the converged mode converges with room to spare (at most 48 of 120 iterations, CPU
# oracle).  On the four one-leg sets and on 0101, 1010 it ends 13 ... 30 of 32 instances OK and rounding decides which.
ENVELOPE_N20 = ((0, 0, 1, 1), (0, 1, 1, 0), (0, 1, 1, 1), (1, 0, 0, 1), (1, 0, 1, 1), (1, 1, 0, 0), (1, 1, 0, 1), (1, 1, 1, 0),
                (1, 1, 1, 1))


def _masked(rec, masks):
    rec["contacts"] = np.array(masks, dtype=np.float64)[np.arange(len(rec)) % len(masks)]
    return rec


def flip(rec, quat=False, quat_d=False):
    """A copy with q -> -q (the same attitude; `rot` stays) on every record"""
    rec = rec.copy()
    if quat:
        rec["quat"] *= -1.0
    if quat_d:
        rec["quat_d"] *= -1.0
    return rec


def quat(pkg, N, flipped=True):
    """480 QuatMpc records, instance k on MASKS4[k % 15]; -quat on every second and -quat_d on every third record.  Every set
    meets both signs of quat; 3 divides 15, so -quat_d falls on MASKS4[0, 3, 6, 9, 12] always and on the other sets never.
    N > 12: the 288 records on ENVELOPE_N20.
    flipped=False: the same records as the generator draws them, both quaternions with w > 0 -- with flip() below, all four
    sign combinations on every set."""
    rec = _masked(pkg.random_go1_trot_states(480, config_id=3 if N == 20 else 2), MASKS4)
    if flipped:
        rec["quat"][::2] *= -1.0
        rec["quat_d"][::3] *= -1.0
    if N > 12:
        rec = rec[[tuple(int(c) for c in m) in ENVELOPE_N20 for m in rec["contacts"]]]
    return rec


def convex(pkg):
    """480 ConvexMpc records, instance k on MASKS4[k % 15]"""
    return _masked(pkg.random_go1_convex_states(480, config_id=12), MASKS4)


def biped8(pkg):
    """256 records of the 8-point model, instance k on MASKS8[k % 16]"""
    return _masked(pkg.random_biped8_states(256, config_id=5), MASKS8)


def warm_pairs(pkg):
    """(first tick [450], second tick [450]): the first tick on MASKS4[k % 15]; the second with slightly different velocities on
    MASKS4[(k // 15) % 15] -- every ordered pair of sets twice, so every leg lands, lifts off, stays down and stays up next to
    every combination of the other three."""
    first = _masked(pkg.random_go1_trot_states(450, config_id=2), MASKS4)
    second = first.copy()
    second["lin_vel_body"] += 0.02
    second["contacts"] = np.array(MASKS4, dtype=np.float64)[(np.arange(450) // 15) % 15]
    return first, second


def tiled(rec, at_least):
    """Whole copies of rec, as few as reach `at_least` records: for kernel forms that exist beyond a batch size only.  The
    unique records stay the CPU-verified ones; every copy must return the first one's bits."""
    return np.tile(rec, -(-int(at_least) // len(rec)))


def copies_identical(a, n):
    """every copy of the first n rows of a tiled result equals the first, bit for bit"""
    a = np.ascontiguousarray(a)
    return all(a[k:k + n].tobytes() == a[:n].tobytes() for k in range(n, len(a), n))


def swing_rows(rec, nl=4):
    """[B, 3 nl] mask of the force components of the points not in stance"""
    return np.repeat(rec["contacts"][:, :nl] == 0, 3, axis=1)


def plain_plan(model, N, mode="converged", knobs="default", kind="plain"):
    """[(smallest batch, family, variant)] of a plain solve (kind="warm": of a warm-started one), from the planner's enumeration tests/golden/kernel_plans.txt.gz
    (tests/test_plan_cpu.py holds qmpc_plan.h to it).  The family query of a handle does not tell the two workspace forms
    of the wave kernels apart (variant 5: gains in the workspace, 6: slack arrays too); the table does."""
    text = gzip.decompress((Path(__file__).parent / "golden" / "kernel_plans.txt.gz").read_bytes()).decode()
    out, on = [], False
    for line in text.splitlines():
        if line.startswith("# "):
            on = line == f"# {model} {mode} N={N} {knobs}"
        elif on and line.startswith(kind + " "):
            w = line.split()
            out.append((int(w[1]), int(w[2]), int(w[3])))
    assert out, (model, N, mode, knobs)
    return out
