"""GPU suite (-m gpu): every quaternion solve path at attitude errors up to and beyond pi (tests/attitude_sets.py).

The state generators keep quat_d within about 0.55 rad of quat; the sign-flip runs of tests/test_gpu_stance_sets.py reach
q_ref'q < 0 only as a relabelling of the same attitude.  The cost w (1 - |q_ref'q|) is written out four times (expand_knot and
expand_knot_part in qmpc_device.h, twice in qmpc_lane_core.h) and every wave form, the dense family, the reference-mode bodies,
the per-instance kernels, the hand-off records and the loop ticks consume those expansions: here its sign branch is taken by
geometry (3.5 rad), its attitude Hessian w |q_ref'q| falls to 0.02 w (3.1 rad), its gradient is of order w, every stance leg is
asked for tangential force and the solves run 20 to 30 iterations -- across the lane kernel's hand-off cap.  The records carry
errors of 0.5 ... 3.5 rad about the body's z, x and y and a random axis in both senses (QuatMpc N = 5, 10; N = 20 up to 1.5 rad;
the 8-point model up to 1.5 rad and, a set of its own, at 2.0 rad); the CPU suite (tests/test_attitude_sets_cpu.py) certifies the
oracle on the same records and keeps them inside the solver's envelope.

Rules, unless a test says otherwise (the project's own for the converged mode, those of tests/test_gpu_stance_sets.py, whose
handle, knob and comparison helpers this module takes): status words equal to the oracle's and all 0; forces within 1e-6 N
(8-point model: corner forces 1e-5, foot wrench 1e-7); swing forces exactly 0; iteration counts equal on >= 97 %; first-knot
forces within 1e-6 (1e-5) of the stored certified points (tests/golden/attitude_fixtures.npz).  On the 8-point set at 2.0 rad
the share of equal iteration counts is printed and not held: there the solver's last steps sit on its step tolerance (the
docstring of tests/test_attitude_sets_cpu.py::test_lane_core_matches_oracle_on_every_attitude_set).  No instance is left out
of a comparison.  Every test reads back the kernel family that ran.  Each prints a line `attitude-sets | ...` with the family,
the worst force difference per angle and the share of equal iteration counts (profiles/r19_attitude_sets.txt is made of them)."""
import ctypes as C
import hashlib
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import attitude_sets as A
from test_gpu_stance_sets import LANE_HANDLES, _bits_differ, _first_batch_beyond, _handle, _last, _same, _wrench8
from test_gpu_stance_sets import lib  # noqa: F401  (the fixture: raises if the HIP extension is missing, no fallback)

pytestmark = pytest.mark.gpu

# name: (records, default params, Solver call, oracle call, horizon, force components, model name of the planner's table,
#        angles of the set, iteration counts held)
SETS = {
    "quat_n5": (lambda pkg: A.quat(pkg, 5), "default_params", "solve", "solve", 5, 12, "quat", A.ANGLES, True),
    "quat_n10": (lambda pkg: A.quat(pkg, 10), "default_params", "solve", "solve", 10, 12, "quat", A.ANGLES, True),
    "quat_n20": (lambda pkg: A.quat(pkg, 20), "default_params", "solve", "solve", 20, 12, "quat", A.ANGLES_N20, True),
    "biped8_n16": (lambda pkg: A.biped8(pkg, 16), "default_biped8_params", "solve8", "solve8", 16, 24, "quat8",
                   A.ANGLES_BIPED8_COUNTS, True),
    "biped8_n16_far": (lambda pkg: A.biped8(pkg, 16, far=True), "default_biped8_params", "solve8", "solve8", 16, 24, "quat8",
                       A.ANGLES_BIPED8[3:], False),
}
_cache = {}


@pytest.fixture(scope="module")
def fix():
    return np.load(Path(__file__).parent / "golden" / "attitude_fixtures.npz")


def _params(pkg, lib, name, mode=None):  # noqa: F811
    return getattr(pkg, SETS[name][1])(SETS[name][4], pkg.MODE_CONVERGED if mode is None else mode, lib)


def _records(pkg, name):
    if ("rec", name) not in _cache:
        _cache["rec", name] = SETS[name][0](pkg)
    return _cache["rec", name]


def _oracle(pkg, oracle, name, mode=0):
    """(forces, info) of the oracle on the set, computed once per module run"""
    if ("oracle", name, mode) not in _cache:
        p = getattr(oracle, SETS[name][1])(SETS[name][4], mode)
        _cache["oracle", name, mode] = getattr(oracle, SETS[name][3])(p, _records(pkg, name), threads=8)
    return _cache["oracle", name, mode]


def _run(pkg, lib, name, cap=None, rec=None, mode=None, family=None, **knobs):  # noqa: F811
    """One solve of the set (or of `rec`) on a fresh handle; asserts the family that ran.  (forces, info)"""
    rec = _records(pkg, name) if rec is None else rec
    with _handle(pkg, lib, _params(pkg, lib, name, mode), cap or len(rec), **knobs) as s:
        planned = s.kernel_for_batch(len(rec))
        f, info = getattr(s, SETS[name][2])(rec)
        ran = _last(pkg, s)
    assert ran == planned and (family is None or ran == family), (name, knobs, planned, ran, family)
    return f, info


def _per_angle(rec, d, angles=A.ANGLES):
    """'0.5: 1.2e-11, 1.0: ...': the largest of d [B] or [B, k] over the records of each error angle"""
    ang = A.grid_angle(rec, angles)
    d = np.asarray(d).reshape(len(rec), -1).max(axis=1)
    return ", ".join(f"{a}: {d[ang == a].max():.1e}" for a in angles if (ang == a).any())


def _converged_rules(pkg, oracle, fix, name, f, info, tag, family):
    """The converged mode's rules of this module on the unique records of a set; prints the record line"""
    rec = _records(pkg, name)
    nu, angles, counts = SETS[name][5], SETS[name][7], SETS[name][8]
    fo, io = _oracle(pkg, oracle, name)
    d = float(np.abs(f - fo).max())
    share = float((info["iterations"] == io["iterations"]).mean())
    dw = float(np.abs(_wrench8(rec, f) - _wrench8(rec, fo)).max()) if nu == 24 else None
    U = fix[name + "_U"] if name + "_U" in fix.files else None
    dc = float(np.abs(f[:len(U)] - U[:, 0, :]).max()) if U is not None else None
    print(f"attitude-sets | {tag} | {name} | family {family} | worst |f - f_oracle| {d:.2e} N, per angle [rad] {{{_per_angle(rec, np.abs(f - fo), angles)}}}"
          + (f" (foot wrench {dw:.2e})" if dw is not None else "") + f" | iteration counts equal on {100 * share:.2f} %"
          + ("" if counts else " (printed, not held)")
          + (f" | certified points within {dc:.2e} N" if dc is not None else "")
          + f" | status counts {np.bincount(info['status'], minlength=6).tolist()}")
    assert np.array_equal(info["status"], io["status"]) and (info["status"] == 0).all(), tag
    assert d < (1e-5 if nu == 24 else 1e-6), (tag, d)
    if nu == 24:
        assert dw < 1e-7, (tag, dw)
    assert np.abs(f[A.swing_rows(rec, nu // 3)]).max() == 0.0, tag
    if counts:
        assert share >= 0.97, (tag, share)
    if U is not None:
        assert dc < (1e-5 if nu == 24 else 1e-6), (tag, dc)


def _wave_lds(pkg, lib, name):  # noqa: F811
    """The set on the all-LDS wave kernel (default planner, the set's own size): what the workspace forms are compared with"""
    if ("lds", name) not in _cache:
        _cache["lds", name] = _run(pkg, lib, name, family="wform_lds")
    return _cache["lds", name]


def _lane(pkg, lib, name="quat_n10"):  # noqa: F811
    if ("lane", name) not in _cache:
        _cache["lane", name] = _run(pkg, lib, name, family="lane", QMPC_VARIANT=4)
    return _cache["lane", name]


# ---- 1. wave kernels, everything in LDS ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SETS))
def test_wave_kernels_in_lds(pkg, lib, oracle, fix, name):  # noqa: F811
    """Default planner at the set's own size (384 / 192 / 96 instances): the wrench-form kernel with everything in LDS.
    Measured, worst force difference to the oracle (share of equal iteration counts where not 100 %): QuatMpc N=5 3.5e-11, N=10
    1.4e-9 (99.48 %), N=20 5.2e-9 N (99.48 %); 8-point corner forces 3.6e-9, foot wrench 3.6e-9; at 2.0 rad 2.8e-9 / 4.7e-9 (85.42 %,
    printed).  Per angle the difference grows from 1e-11 N at 0.5 rad to 1e-9 N from 2.5 rad on (profiles/r19_attitude_sets.txt)."""
    f, info = _wave_lds(pkg, lib, name)
    _converged_rules(pkg, oracle, fix, name, f, info, "wave, all LDS", "wform_lds")


# ---- 2. wave kernels, workspace forms -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["quat_n5", "quat_n10", "quat_n20", "biped8_n16"])
def test_wave_kernels_workspace_forms(pkg, lib, oracle, fix, name):  # noqa: F811
    """The set tiled to just beyond the batch at which the planner leaves the all-LDS form (asked of the handle), and -- where
    the planner's table (tests/golden/kernel_plans.txt.gz) has a second workspace form for the horizon: the slack arrays out as
    well -- to just beyond that batch too: QuatMpc N=10 / 5 take the gains-in-workspace form, QuatMpc N=20 and the 8-point model
    both.  Against the all-LDS form on the unique records: forces within 1e-7 N (8-point 1e-5) and identical iteration counts
    (the forms differ in where their arrays live); every copy returns the first one's bits; and the oracle's rules.
    Measured: every workspace form returns the all-LDS form's BITS on every set (0.0 N), so the figures of test_wave_kernels_in_lds."""
    rec, (model, N, nu) = _records(pkg, name), (SETS[name][6], SETS[name][4], SETS[name][5])
    n = len(rec)
    fl, il = _wave_lds(pkg, lib, name)
    with _handle(pkg, lib, _params(pkg, lib, name), 4096) as s:
        b1 = _first_batch_beyond(s, "wform_lds", 4096)
        assert b1 > n and s.kernel_for_batch(b1) == "wform_ws"
        steps = [(b1, 5, None)]
        if N != 5:          # (the table enumerates N = 4, 10, ...: the N = 5 handle is asked alone)
            plan = A.plain_plan(model, N)
            ws = [(b, var, plan[i + 1][0] if i + 1 < len(plan) else None) for i, (b, fam, var) in enumerate(plan) if fam == 2]
            assert ws[0][0] == b1 and [v for _, v, _ in ws] == ([5] if N == 10 else [5, 6]), (ws, b1)
            steps = ws
        for b, var, end in steps:
            t = A.tiled(rec, b)
            assert end is None or len(t) < end, (name, b, len(t), end)
            assert s.kernel_for_batch(len(t)) == "wform_ws"
            f, info = getattr(s, SETS[name][2])(t)
            assert _last(pkg, s) == "wform_ws"
            tag = f"wave, workspace form {var} at {len(t)}"
            assert A.copies_identical(f, n) and A.copies_identical(info["status"], n) and A.copies_identical(info["iterations"], n), tag
            d = float(np.abs(f[:n] - fl).max())
            print(f"attitude-sets | {tag} | {name} | against the all-LDS form: {d:.2e} N, iteration counts equal "
                  f"{np.array_equal(info['iterations'][:n], il['iterations'])}")
            assert d < (1e-5 if nu == 24 else 1e-7), (tag, d)
            assert np.array_equal(info["iterations"][:n], il["iterations"]), tag
            _converged_rules(pkg, oracle, fix, name, f[:n], info[:n], tag, "wform_ws")


# ---- 3. round-1 family --------------------------------------------------------------------------------------------------------
def test_round_1_family(pkg, lib, oracle, fix):  # noqa: F811
    """QMPC_WFORM=0: the dense kernels -- the only consumer of expand_knot -- everything in LDS at 384 instances and, tiled
    beyond the batch the handle names, with the gains in the workspace.  Measured: 2.6e-9 N (all LDS) and 2.7e-9 N (workspace form) from the oracle,
    iteration counts equal on 98.96 / 99.22 %; the two forms within 1.2e-9 N of each other, iteration counts equal on 98.70 %."""
    name = "quat_n10"
    rec = _records(pkg, name)
    n = len(rec)
    with _handle(pkg, lib, _params(pkg, lib, name), 4096, QMPC_WFORM=0) as s:
        assert s.kernel_for_batch(n) == "dense_lds"
        f, info = s.solve(rec)
        assert _last(pkg, s) == "dense_lds"
        _converged_rules(pkg, oracle, fix, name, f, info, "round-1 family, all LDS", "dense_lds")
        t = A.tiled(rec, _first_batch_beyond(s, "dense_lds", 4096))
        assert s.kernel_for_batch(len(t)) == "dense_ws"
        ft, it_ = s.solve(t)
        assert _last(pkg, s) == "dense_ws"
    assert A.copies_identical(ft, n) and A.copies_identical(it_["status"], n) and A.copies_identical(it_["iterations"], n)
    _converged_rules(pkg, oracle, fix, name, ft[:n], it_[:n], f"round-1 family, workspace form at {len(t)}", "dense_ws")
    # the two dense forms are two rounding families (on the stance sets they differ by 1e-11 N), and from 2.5 rad on the last
    # steps of a solve sit on the step tolerance (tests/test_attitude_sets_cpu.py), so between them the rule is the one this
    # project has for two rounding families, test_straggler_hand_off's: status equal, forces within 1e-7 N, iteration counts
    # equal on >= 97 % -- not identical iteration words, which only the wave workspace forms (the all-LDS form's bits) can give
    d, share = float(np.abs(ft[:n] - f).max()), float((it_["iterations"][:n] == info["iterations"]).mean())
    print(f"attitude-sets | round-1 family | workspace form against all LDS: {d:.2e} N, per angle [rad] {{{_per_angle(rec, np.abs(ft[:n] - f))}}}, "
          f"iteration counts equal on {100 * share:.2f} %")
    assert np.array_equal(it_["status"][:n], info["status"]) and d < 1e-7 and share >= 0.97, (d, share)


# ---- 4. reference mode --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,knobs,family", [("quat_n10", {}, "wform_lds"), ("biped8_n16", {}, "wform_lds"),
                                               ("quat_n10", {"QMPC_WFORM": 0}, "dense_lds")])
def test_reference_mode_on_the_wave_kernels(pkg, lib, oracle, name, knobs, family):  # noqa: F811
    """MODE_REFERENCE (truncated AL-iLQR iterates) under the rule of test_reference_mode_on_device_matches_oracle_reference_mode:
    >= 99 % of the instances agree with the oracle to 1e-6 N with identical status and iteration words; swing forces exactly 0.
    Measured: QuatMpc 384 of 384 identical (worst 2.0e-8 N; status counts 47 OK / 317 MAX_ITER / 20 LINESEARCH_FAIL), with
    QMPC_WFORM=0 384 of 384 (4.2e-9 N); 8-point 192 of 192 (7.6e-11 N)."""
    rec = _records(pkg, name)
    f, info = _run(pkg, lib, name, mode=pkg.MODE_REFERENCE, family=family, **knobs)
    fo, io = _oracle(pkg, oracle, name, 1)
    d = np.abs(f - fo).max(axis=1)
    same = (d < 1e-6) & (info["status"] == io["status"]) & (info["iterations"] == io["iterations"])
    print(f"attitude-sets | reference mode, wave kernels {knobs or ''} | {name} | family {family} | {int(same.sum())}/{len(rec)} identical "
          f"(1e-6 N, status, iterations) | worst {d.max():.2e} N, per angle [rad] {{{_per_angle(rec, d, SETS[name][7])}}} | "
          f"status counts {np.bincount(info['status'], minlength=6).tolist()}")
    assert same.mean() >= 0.99
    assert np.abs(f[A.swing_rows(rec, SETS[name][5] // 3)]).max() == 0.0 and np.isfinite(f).all()


@pytest.mark.parametrize("name", ["quat_n10", "quat_n20", "biped8_n16"])
def test_lane_kernel_reference_mode(pkg, lib, oracle, name):  # noqa: F811
    """The rule of tests/test_gpu_lane.py::test_lane_kernel_reference_mode: status and iteration words identical to the oracle's
    on every instance, forces within 1e-6 N on >= 95 % (truncated iterates); swing forces exactly 0.
    Measured: within 1e-6 N on 100 % everywhere; worst 1.3e-10 (QuatMpc N=10), 3.1e-10 (N=20), 7.6e-11 N (8-point)."""
    rec = _records(pkg, name)
    f, info = _run(pkg, lib, name, mode=pkg.MODE_REFERENCE, family="lane", QMPC_VARIANT=4)
    fo, io = _oracle(pkg, oracle, name, 1)
    d = np.abs(f - fo).max(axis=1)
    print(f"attitude-sets | reference mode, lane kernel | {name} | family lane | within 1e-6 N on {100 * (d < 1e-6).mean():.2f} % | "
          f"worst {d.max():.2e} N, per angle [rad] {{{_per_angle(rec, d, SETS[name][7])}}} | status counts {np.bincount(info['status'], minlength=6).tolist()}")
    assert np.array_equal(info["status"], io["status"]) and np.array_equal(info["iterations"], io["iterations"])
    assert (d < 1e-6).mean() >= 0.95
    assert np.abs(f[A.swing_rows(rec, SETS[name][5] // 3)]).max() == 0.0 and np.isfinite(f).all()


# ---- 5. lane kernel -----------------------------------------------------------------------------------------------------------
def _lane_handles(pkg, lib):  # noqa: F811
    """quat(10) on the four handles of QMPC_VARIANT=4: lane pairs on the sorted batch (default), QMPC_LANE_PAIR=0, QMPC_LANE_SORT=0, both"""
    if "lane4" not in _cache:
        _cache["lane4"] = {tag: (_lane(pkg, lib) if not knobs else _run(pkg, lib, "quat_n10", family="lane", QMPC_VARIANT=4, **knobs))
                           for tag, knobs in LANE_HANDLES.items()}
    return _cache["lane4"]


def test_lane_kernel_at_every_attitude_error(pkg, lib, oracle, fix):  # noqa: F811
    """QMPC_VARIANT=4 on quat(10), four handles: lane pairs or the plain form with half the lanes masked, on the batch sorted by
    stance set or in its own order (a wavefront then holds all eight angles, and the lanes at 3 rad run twice as long as those
    at 0.5 rad).  Each handle against the oracle; the order of the batch does not change a bit of either form, and the pair
    form returns the plain form's bits (the contract of tests/test_gpu_lane.py::test_lane_pairs_return_the_plain_forms_bits).
    Measured: 2.2e-9 N from the oracle on all four handles, iteration counts equal on 98.96 %; 0 instances differ between any two."""
    runs = _lane_handles(pkg, lib)
    for tag, (f, info) in runs.items():
        _converged_rules(pkg, oracle, fix, "quat_n10", f, info, f"lane kernel ({tag})", "lane")
    for form in ("pairs", "plain"):
        n, d, st, it_ = _bits_differ(runs[form + ", sorted"], runs[form + ", unsorted"])
        print(f"attitude-sets | lane kernel ({form}) | sorted against unsorted batch: {n} instances differ, largest difference {d:.2e} N")
        assert n == 0 and st and it_, (form, n, d)
    base = runs["pairs, sorted"]
    for tag in list(LANE_HANDLES)[1:]:
        n, d, st, it_ = _bits_differ(runs[tag], base)
        print(f"attitude-sets | lane kernel ({tag}) | against the default handle (pairs, sorted): {n} instances differ, largest difference "
              f"{d:.2e} N, status words equal {st}, iteration words equal {it_}")
        assert st and it_, tag
        assert n == 0, (tag, n, d)


@pytest.mark.parametrize("name", [n for n in SETS if n != "quat_n10"])
def test_lane_kernel_other_sets(pkg, lib, oracle, fix, name):  # noqa: F811
    """The other sets on the default handle of QMPC_VARIANT=4.  Measured: QuatMpc N=5 9.8e-11 N, N=20 5.1e-9 N (98.96 %); 8-point
    3.1e-9 (foot wrench 3.1e-9; 98.96 %); at 2.0 rad 4.3e-9 (8.5e-9), iteration counts equal on 84.38 % (printed)."""
    f, info = _lane(pkg, lib, name)
    _converged_rules(pkg, oracle, fix, name, f, info, "lane kernel (pairs, sorted)", "lane")


def test_lane_kernel_full_wavefronts(pkg, lib, oracle, fix):  # noqa: F811
    """The plain 64-lane form launches only when twice the batch exceeds the resident lanes (a handle of 70000, more than 32768
    instances): quat(10) tiled to 33024.  Every copy returns the first one's bits; the unique records follow the oracle and
    return the bits of the 384-instance launches, plain form and lane pairs.  Measured: 0 instances differ from either; 2.2e-9 N from the oracle."""
    rec = _records(pkg, "quat_n10")
    n = len(rec)
    runs = _lane_handles(pkg, lib)
    t = A.tiled(rec, 32769)
    f, info = _run(pkg, lib, "quat_n10", cap=70000, rec=t, family="lane", QMPC_VARIANT=4)
    assert A.copies_identical(f, n) and A.copies_identical(info["status"], n) and A.copies_identical(info["iterations"], n)
    _converged_rules(pkg, oracle, fix, "quat_n10", f[:n], info[:n], f"lane kernel, full wavefronts at {len(t)}", "lane")
    first = (f[:n], info[:n])
    for tag in ("plain, sorted", "pairs, sorted"):
        k, d, st, it_ = _bits_differ(first, runs[tag])
        print(f"attitude-sets | lane kernel, full wavefronts at {len(t)} | against the {n}-instance launch ({tag}): {k} instances differ, "
              f"largest difference {d:.2e} N, status words equal {st}, iteration words equal {it_}")
        assert st and it_, tag
        assert k == 0, (tag, k, d)


# ---- 6. warm start ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knobs,family", [({}, "wform_lds"), ({"QMPC_VARIANT": 4}, "lane")], ids=["wave", "lane"])
def test_warm_start_between_attitude_errors(pkg, lib, oracle, knobs, family):  # noqa: F811
    """qmpc_solve_warm at N=10 with the closed loop's low initial barrier (ipm_mu0 = 1e-6) on warm_pairs(10) up to 2.5 rad (the
    envelope of that barrier, tests/test_attitude_sets_cpu.py): a cold call, then the next tick from its trajectory with the
    reference attitude at the neighbouring angle of the grid and, on every third record, the trot diagonals changed over.  The
    rules of test_warm_start_between_every_pair_of_stance_sets against oracle.solve_warm: status equal and all 0, forces within
    1e-6 N, iteration counts equal on >= 90 % and within one on >= 95 %; swing forces of the new set exactly 0; trajectories
    within 1e-5 N.  Measured: wave kernel cold 3.0e-9, warm 5.3e-10 N, iteration counts equal on 100 %;
    lane kernel cold 1.6e-9, warm 2.3e-9 N, equal on 98.96 %, within one on 100 %."""
    first, second = A.warm_pairs(pkg, 10, A.WARM_LOW_BARRIER_MAX)
    B, N = len(first), 10
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    p.ipm_mu0 = 1e-6
    # (qmpc_solve_warm does not record its launch for QUERY_LAST_KERNEL: the family is the planner's for a warm-started call of
    # this size under these knobs -- its table -- which shares the plain solve's choice, asked of the handle)
    table = A.plain_plan("quat", N, knobs="QMPC_VARIANT=4" if knobs else "default", kind="warm")
    assert pkg.KERNEL_FAMILY[[fam for b, fam, _ in table if b <= B][-1]] == family
    with _handle(pkg, lib, p, B, **knobs) as s:
        assert s.kernel_for_batch(B) == family
        f0, i0, tu0 = s.solve_warm(first, None)
        f1, i1, tu1 = s.solve_warm(second, tu0)
    po = oracle.default_params(N, 0)
    po.ipm_mu0 = 1e-6
    if "warm0" not in _cache:
        _cache["warm0"] = oracle.solve_warm(po, first, None, threads=8)
    fo0, io0, _ = _cache["warm0"]
    fo1, io1, tuo1 = oracle.solve_warm(po, second, tu0, threads=8)
    di = np.abs(i1["iterations"].astype(int) - io1["iterations"].astype(int))
    print(f"attitude-sets | warm start | family {family} | cold {np.abs(f0 - fo0).max():.2e} N, warm {np.abs(f1 - fo1).max():.2e} N, "
          f"per angle of the second tick [rad] {{{_per_angle(second, np.abs(f1 - fo1))}}} | "
          f"iteration counts equal on {100 * (di == 0).mean():.2f} %, within one on {100 * (di <= 1).mean():.2f} % | "
          f"warm iterations {i1['iterations'].mean():.2f} (cold {i0['iterations'].mean():.2f})")
    assert np.array_equal(i0["status"], io0["status"]) and (i0["status"] == 0).all() and np.abs(f0 - fo0).max() < 1e-6
    assert np.array_equal(i1["status"], io1["status"]) and (i1["status"] == 0).all()
    assert np.abs(f1 - fo1).max() < 1e-6
    assert (di == 0).mean() >= 0.9 and (di <= 1).mean() >= 0.95, np.bincount(di)
    assert np.abs(f1[A.swing_rows(second)]).max() == 0.0
    assert np.abs(tu1.reshape(B, N, 12)[np.repeat(A.swing_rows(second)[:, None, :], N, axis=1)]).max() == 0.0
    assert np.abs(tu1.reshape(B, -1) - tuo1.reshape(B, -1)).max() < 1e-5


# ---- 7. hand-off --------------------------------------------------------------------------------------------------------------
def test_straggler_hand_off(pkg, lib, oracle, fix):  # noqa: F811
    """QMPC_LANE_MIN=64, QMPC_LANE_CAP=12 on quat(10): the lane kernel stops at 12 iterations and the wave kernel continues what
    is left from the hand-off's records -- at these errors at least half of the batch (asserted from the oracle's counts).
    Against the same handle with QMPC_LANE_CAP=0 (the pure lane kernel) under the rules of
    tests/test_gpu_stance_sets.py::test_straggler_hand_off: status equal, forces within 1e-7 N, iteration counts equal on
    >= 97 %; a second call returns the same bits; the same with QMPC_HANDOFF_RESTART=1.
    Measured: 93.8 % of the batch beyond the cap; 2.2e-9 N from the oracle and 2.2e-10 N from the pure lane kernel with iteration
    counts equal on 100 %; with the restart 1.4e-9 N from the oracle (the wave kernel's figures) and 2.5e-9 N from the pure lane
    kernel, equal on 99.48 %."""
    name = "quat_n10"
    rec = _records(pkg, name)
    fo, io = _oracle(pkg, oracle, name)
    handed = float((io["iterations"] > 12).mean())
    assert handed >= 0.5, handed
    fp, ip = _run(pkg, lib, name, family="lane", QMPC_LANE_MIN=64, QMPC_LANE_CAP=0)
    _converged_rules(pkg, oracle, fix, name, fp, ip, "lane kernel below QMPC_LANE_MIN=64, no hand-off", "lane")
    for knobs in ({}, {"QMPC_HANDOFF_RESTART": 1}):
        with _handle(pkg, lib, _params(pkg, lib, name), len(rec), QMPC_LANE_MIN=64, QMPC_LANE_CAP=12, **knobs) as s:
            assert s.kernel_for_batch(len(rec)) == "lane_handoff" and s.query(pkg.QUERY_LANE_CAP, 1) == 12
            f, info = s.solve(rec)
            assert _last(pkg, s) == "lane_handoff"
            f2, info2 = s.solve(rec)
        tag = f"hand-off at 12 iterations {knobs or ''}"
        assert _same(f, f2) and _same(info, info2), tag
        _converged_rules(pkg, oracle, fix, name, f, info, tag, "lane_handoff")
        share = float((info["iterations"] == ip["iterations"]).mean())
        d = float(np.abs(f - fp).max())
        print(f"attitude-sets | {tag} | {100 * handed:.1f} % of the batch beyond the cap | against the pure lane kernel: {d:.2e} N, "
              f"per angle [rad] {{{_per_angle(rec, np.abs(f - fp))}}}, iteration counts equal on {100 * share:.2f} %")
        assert np.array_equal(info["status"], ip["status"]) and d < 1e-7 and share >= 0.97, (tag, d, share)


# ---- 8. per-instance parameter paths ------------------------------------------------------------------------------------------
def test_per_instance_paths_with_uniform_records(pkg, lib, oracle, fix):  # noqa: F811
    """Records that carry the handle's own values return the plain solve's bytes: qmpc_solve_instances on the wave kernel
    (default policy) and on the lane kernel (QMPC_INSTANCES_AUTO, QMPC_LANE_INST_MIN=64; the plain solve on the lane kernel too:
    QMPC_LANE_MIN=64).  Measured: bytes equal in both; 1.4e-9 N (wave) and 2.2e-9 N (lane_handoff) from the oracle."""
    rec = _records(pkg, "quat_n10")
    p = _params(pkg, lib, "quat_n10")
    n = len(rec)
    with _handle(pkg, lib, p, n) as s:
        assert s.kernel_for_instances(n) == s.kernel_for_batch(n) == "wform_lds"
        fi, ii = s.solve_instances(rec, pkg.instance_params(p, n))
        assert _last(pkg, s) == "wform_lds"
        fp, ip = s.solve(rec)
    assert _same(fi, fp) and _same(ii, ip)
    _converged_rules(pkg, oracle, fix, "quat_n10", fi, ii, "solve_instances, default policy", "wform_lds")
    with _handle(pkg, lib, p, n, QMPC_LANE_INST_MIN=64, QMPC_LANE_MIN=64) as s:
        s.set_instances_policy("auto")
        fam = s.kernel_for_instances(n)
        assert fam in ("lane", "lane_handoff") and fam == s.kernel_for_batch(n)
        fi, ii = s.solve_instances(rec, pkg.instance_params(p, n))
        assert _last(pkg, s) == fam
        fp, ip = s.solve(rec)
        assert _last(pkg, s) == fam
    assert _same(fi, fp) and _same(ii, ip)
    _converged_rules(pkg, oracle, fix, "quat_n10", fi, ii, "solve_instances, auto policy", fam)


@pytest.mark.parametrize("policy", ["wave", "auto"])
def test_random_variants_at_every_attitude_error(pkg, lib, oracle, policy):  # noqa: F811
    """quat(10) with a robot of its own per instance (attitude_sets.variants: pkg.random_go1_variants' mass, inertia, friction,
    force bound, Q and R, and the attitude weight w, the factor of the cost under test, scaled by U(0.5, 1.25) per instance:
    the range on which the reference alone converges) on the wave kernel (default policy) and on the lane kernel (auto,
    QMPC_LANE_INST_MIN=64), against the oracle solved per instance with that instance's parameters, the way and under the
    tolerances of tests/test_gpu_instance_params.py::test_random_variants_against_the_oracle: more than 95 % converge, every
    status word is the oracle's, and where that is 0 the forces are within 1e-6 N -- here on all 384 instances.
    Measured: 1.9e-8 N (wave kernel) and 1.2e-8 N (lane_handoff) from the oracle, both at 3.5 rad; every status 0 on both sides;
    iteration counts equal on 99.22 / 98.96 %.  (With the weight scaled up to 2 w the kernels ended 3 / 1 records MAX_ITER where the
    oracle ended one NOT_PD and another after 63 iterations: outside the reference's envelope, attitude_sets.variants.)"""
    rec = _records(pkg, "quat_n10")
    n = len(rec)
    p = _params(pkg, lib, "quat_n10")
    ip = A.variants(pkg, p)
    knobs = {"QMPC_LANE_INST_MIN": 64} if policy == "auto" else {}
    with _handle(pkg, lib, p, n, **knobs) as s:
        s.set_instances_policy(policy)
        fam = s.kernel_for_instances(n)
        assert fam in (("lane", "lane_handoff") if policy == "auto" else ("wform_lds",)), fam
        f, info = s.solve_instances(rec, ip)
        assert _last(pkg, s) == fam
    if "variants" not in _cache:
        _cache["variants"] = [oracle.solve(pkg.params_with(p, ip[i]), rec[i:i + 1]) for i in range(n)]
    fo = np.concatenate([o[0] for o in _cache["variants"]])
    so = np.array([int(o[1]["status"][0]) for o in _cache["variants"]])
    ito = np.array([int(o[1]["iterations"][0]) for o in _cache["variants"]])
    ok = so == 0
    d = np.where(ok[:, None], np.abs(f - fo), 0.0)
    print(f"attitude-sets | solve_instances, random variants with per-instance w, {policy} policy | quat_n10 | family {fam} | "
          f"worst |f - f_oracle| {d.max():.2e} N, per angle [rad] {{{_per_angle(rec, d)}}} | iteration counts equal on "
          f"{100 * (info['iterations'] == ito).mean():.2f} % | status counts {np.bincount(info['status'], minlength=6).tolist()} "
          f"(oracle {np.bincount(so, minlength=6).tolist()})")
    assert (info["status"] == 0).mean() > 0.95
    assert np.array_equal(info["status"], so)
    assert d.max() <= 1e-6


# ---- 9. device closed loop ----------------------------------------------------------------------------------------------------
def test_device_closed_loop_from_large_attitude_errors(pkg, lib):  # noqa: F811
    """Eight standing robots (attitude_sets.loop_states) that start 1.0, 2.0, 3.0 and 3.5 rad of yaw and 1.0 and 2.0 rad about a
    random axis away from their attitude reference, two where it is; 40 ticks in stand mode at N = 10.  Both sides carry quat_d
    as state: the device tick (qmpc_loop_math.h) and the host classes (host/QuatMpcHip.h, pack_input) integrate it with the
    commanded body rates -- zero here -- and neither rebuilds it from the measured yaw, so the error is what the solves see
    at every tick until the body has turned.  The device loop against the same ticks built from the host classes, with the
    harness and bounds of tests/test_gpu_parity.py::test_device_closed_loop_matches_host_classes_tick_for_tick: contact flags
    exact, forces <= 1e-6 N at every tick, final states <= 1e-8; the persistent kernel and the per-tick form return the same
    bytes (test_persistent_loop_kernel_equals_the_per_tick_sequence); and the attitude error shrinks on every rotated robot.
    Measured: forces and states equal to the host classes' to the last bit (the host tick launches the same kernel for one robot);
    the two launch forms the same bytes; attitude error after 40 ticks (0.2 s) 1.0 -> 0.22, 2.0 -> 0.73, 3.0 -> 1.17 and 3.5 (2.78
    the short way round, which the controller takes) -> 2.43 rad of yaw, 1.0 -> 0.17 and 2.0 -> 0.15 rad about the random axes;
    17 ... 23 iterations at the last tick against 10 on the unrotated robots."""
    import __graft_entry__ as g

    host = C.CDLL(str(g.build_host()))
    vp = C.c_void_p
    host.qh_loop_create.argtypes = [C.c_char_p, C.c_int, vp, vp]; host.qh_loop_create.restype = vp
    for fn in ("qh_loop_tick", "qh_loop_destroy", "qh_loop_device_status"):
        getattr(host, fn).argtypes = [vp]
    host.qh_loop_export.argtypes = [vp, vp]
    T, N = 40, 10
    lp = pkg.default_loop_params(lib)
    st_init = A.loop_states(pkg, lib, lp)
    B = len(st_init)
    dot = (st_init["quat"] * st_init["quat_d"]).sum(axis=1)
    assert np.allclose(A.attitude_distance(st_init), [a if a < np.pi else 2 * np.pi - a for _, a in A.LOOP_ERRORS], rtol=0, atol=1e-7)
    assert np.array_equal(dot < 0, np.array([a > np.pi for _, a in A.LOOP_ERRORS]))
    s = pkg.Solver(pkg.default_params(N, pkg.MODE_CONVERGED, lib), B, device=0, lib=lib)
    st, tf, tc = s.loop_run(st_init, T, lp, trace=True)
    s.close()
    assert (st["tick"] == T).all() and (st["status"] == 0).all(), st["status"]
    worst_f = worst_x = 0.0
    for i in range(B):
        h = host.qh_loop_create(str(pkg.LIB_PATH).encode(), N, C.addressof(lp), st_init[i:i + 1].ctypes.data)
        assert h and host.qh_loop_device_status(h) == 0
        e = np.zeros(1, dtype=pkg.LOOP_STATE_DTYPE)
        for t in range(T):
            assert host.qh_loop_tick(h) == 1, (i, t)
            host.qh_loop_export(h, e.ctypes.data)
            assert np.array_equal(e[0]["contacts"], tc[t, i]), (i, t, e[0]["contacts"], tc[t, i])     # exact
            worst_f = max(worst_f, float(np.abs(e[0]["forces_body"] - tf[t, i]).max()))
        host.qh_loop_destroy(h)
        d, r = st[i], e[0]
        for k in ("pos_world", "quat", "lin_vel_world", "ang_vel_body", "foot_pos_world", "pos_d_world", "quat_d", "grf_world",
                  "foot_target_world"):
            worst_x = max(worst_x, float(np.abs(d[k] - r[k]).max()))
    before, after = A.attitude_distance(st_init), A.attitude_distance(st)
    sha = hashlib.sha256(st.tobytes() + tf.tobytes() + tc.tobytes()).hexdigest()
    print(f"attitude-sets | device closed loop, {B} robots x {T} ticks in stand mode | worst force difference to the host classes "
          f"{worst_f:.2e} N, worst state difference {worst_x:.2e} | attitude error [rad] " +
          ", ".join(f"{k or 'none'} {a}: {b:.3f} -> {c:.3f}" for (k, a), b, c in zip(A.LOOP_ERRORS, before, after)) +
          f" | iterations of the last tick {st['iterations'].astype(int).tolist()}")
    assert worst_f <= 1e-6 and worst_x <= 1e-8
    # carried, never rebuilt: no rate is commanded, so 40 normalisations are all that happens to it
    assert np.abs(st["quat_d"] - st_init["quat_d"]).max() < 1e-13
    rotated = np.array([k is not None for k, _ in A.LOOP_ERRORS])
    assert (after[rotated] < before[rotated]).all(), (before, after)
    worker = Path(__file__).resolve().parent / "_loop_attitude_worker.py"
    out = {}
    for fused in ("0", "1"):
        r = subprocess.run([sys.executable, str(worker), str(T), str(N)], env=dict(os.environ, QMPC_LOOP_FUSED=fused),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        out[fused] = [l for l in r.stdout.splitlines() if l.startswith("SHA")][0].split()[1]
    print(f"attitude-sets | device closed loop | per-tick form and persistent kernel: the same bytes {out['0'] == out['1']}")
    assert out["0"] == out["1"] and sha in out.values()
