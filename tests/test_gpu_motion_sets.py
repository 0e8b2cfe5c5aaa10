"""GPU suite (-m gpu): every quaternion solve path at body rates up to 12 rad/s and speeds up to 3 m/s, the rate fed to the
problem (tests/motion_sets.py; drop_ang_vel = 0 on every handle).

The default parameters drop the measured angular velocity (the reference's x_init) and the state generators draw it at
sigma = 0.5 rad/s; the stance sets, the attitude sets, the per-instance, hand-off, reference-mode and 8-point tests all run with
the rate dropped.  The product runs with it fed.  It enters through the quaternion kinematics -- Omega(w) in qmpc_device.h, the
attitude blocks of the wrench-form linearisation (qmpc_wform.h), the knot expansions of qmpc_lane_core.h, the trial rollouts --
and with w0 = 0 those blocks are near zero over the whole horizon: a wrong sign, a transposed block or a stale operand in any one
copy passes.  The records carry rates of 1 ... 12 rad/s about the body's z, x and y and a random axis in both senses at the
generator's speed, 1 and 3 m/s (QuatMpc N = 5, 10, 20; the 8-point model at N = 16); the CPU suite
(tests/test_motion_sets_cpu.py) certifies the oracle on the same records, keeps them inside the solver's envelope and shows
that dropping the rate moves the forces by tens of newtons.

Rules, unless a test says otherwise (the project's own for the converged mode, those of tests/test_gpu_stance_sets.py, whose
handle, knob and comparison helpers this module takes): status words equal to the oracle's and all 0; forces within 1e-6 N
(8-point model: corner forces 1e-5, foot wrench 1e-7); swing forces exactly 0; iteration counts equal on >= 97 %; first-knot
forces within 1e-6 (1e-5) of the stored certified points (tests/golden/motion_fixtures.npz).  No instance is left out of a
comparison.  Every test reads back the kernel family that ran.  Each prints a line `motion-sets | ...` with the family, the
worst force difference per rate and the share of equal iteration counts (profiles/r20_motion_sets.txt is made of them)."""
import ctypes as C
import hashlib
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import motion_sets as M
from test_gpu_stance_sets import LANE_HANDLES, _bits_differ, _first_batch_beyond, _handle, _last, _same, _wrench8
from test_gpu_stance_sets import lib  # noqa: F401  (the fixture: raises if the HIP extension is missing, no fallback)

pytestmark = pytest.mark.gpu

# name: (records, default params, Solver call, oracle call, horizon, force components, model name of the planner's table)
SETS = {
    "quat_n5": (lambda pkg: M.quat(pkg, 5), "default_params", "solve", "solve", 5, 12, "quat"),
    "quat_n10": (lambda pkg: M.quat(pkg, 10), "default_params", "solve", "solve", 10, 12, "quat"),
    "quat_n20": (lambda pkg: M.quat(pkg, 20), "default_params", "solve", "solve", 20, 12, "quat"),
    "biped8_n16": (lambda pkg: M.biped8(pkg, 16), "default_biped8_params", "solve8", "solve8", 16, 24, "quat8"),
}
_cache = {}


@pytest.fixture(scope="module")
def fix():
    return np.load(Path(__file__).parent / "golden" / "motion_fixtures.npz")


def _params(pkg, lib, name, mode=None):  # noqa: F811
    return M.params(pkg, SETS[name][1], SETS[name][4], pkg.MODE_CONVERGED if mode is None else mode, lib)


def _records(pkg, name):
    if ("rec", name) not in _cache:
        _cache["rec", name] = SETS[name][0](pkg)
    return _cache["rec", name]


def _oracle(pkg, oracle, name, mode=0):
    """(forces, info) of the oracle on the set, computed once per module run"""
    if ("oracle", name, mode) not in _cache:
        p = M.params(oracle, SETS[name][1], SETS[name][4], mode)
        _cache["oracle", name, mode] = getattr(oracle, SETS[name][3])(p, _records(pkg, name), threads=8)
    return _cache["oracle", name, mode]


def _run(pkg, lib, name, cap=None, rec=None, mode=None, family=None, **knobs):  # noqa: F811
    """One solve of the set (or of `rec`) on a fresh handle; asserts the family that ran.  (forces, info)"""
    rec = _records(pkg, name) if rec is None else rec
    p = _params(pkg, lib, name, mode)
    assert p.drop_ang_vel == 0
    with _handle(pkg, lib, p, cap or len(rec), **knobs) as s:
        planned = s.kernel_for_batch(len(rec))
        f, info = getattr(s, SETS[name][2])(rec)
        ran = _last(pkg, s)
    assert ran == planned and (family is None or ran == family), (name, knobs, planned, ran, family)
    return f, info


def _per_rate(rec, d):
    """'1.0: 1.2e-11, 2.0: ...': the largest of d [B] or [B, k] over the records of each body rate"""
    r = M.grid_rate(rec)
    d = np.asarray(d).reshape(len(rec), -1).max(axis=1)
    return ", ".join(f"{a}: {d[r == a].max():.1e}" for a in M.RATES if (r == a).any())


def _converged_rules(pkg, oracle, fix, name, f, info, tag, family):
    """The converged mode's rules of this module on the unique records of a set; prints the record line"""
    rec = _records(pkg, name)
    nu = SETS[name][5]
    fo, io = _oracle(pkg, oracle, name)
    d = float(np.abs(f - fo).max())
    share = float((info["iterations"] == io["iterations"]).mean())
    dw = float(np.abs(_wrench8(rec, f) - _wrench8(rec, fo)).max()) if nu == 24 else None
    U = fix[name + "_U"] if name + "_U" in fix.files else None
    dc = float(np.abs(f[:len(U)] - U[:, 0, :]).max()) if U is not None else None
    print(f"motion-sets | {tag} | {name} | family {family} | worst |f - f_oracle| {d:.2e} N, per rate [rad/s] {{{_per_rate(rec, np.abs(f - fo))}}}"
          + (f" (foot wrench {dw:.2e})" if dw is not None else "") + f" | iteration counts equal on {100 * share:.2f} %"
          + (f" | certified points within {dc:.2e} N" if dc is not None else "")
          + f" | status counts {np.bincount(info['status'], minlength=6).tolist()}")
    assert np.array_equal(info["status"], io["status"]) and (info["status"] == 0).all(), tag
    assert d < (1e-5 if nu == 24 else 1e-6), (tag, d)
    if nu == 24:
        assert dw < 1e-7, (tag, dw)
    assert np.abs(f[M.swing_rows(rec, nu // 3)]).max() == 0.0, tag
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
    """Default planner at the set's own size (360 / 240 instances): the wrench-form kernel with everything in LDS.
    Measured, worst force difference to the oracle: QuatMpc N=5 4.4e-11, N=10 5.9e-11, N=20 7.7e-11 N; 8-point corner forces and
    foot wrench 1.9e-10 N; iteration counts equal on 100 % everywhere.  Per rate the difference grows from 3e-12 N at 1 rad/s to
    6e-11 N at 12 rad/s (profiles/r20_motion_sets.txt)."""
    f, info = _wave_lds(pkg, lib, name)
    _converged_rules(pkg, oracle, fix, name, f, info, "wave, all LDS", "wform_lds")


# ---- 2. wave kernels, workspace forms -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SETS))
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
            plan = M.plain_plan(model, N)
            ws = [(b, var, plan[i + 1][0] if i + 1 < len(plan) else None) for i, (b, fam, var) in enumerate(plan) if fam == 2]
            assert ws[0][0] == b1 and [v for _, v, _ in ws] == ([5] if N == 10 else [5, 6]), (ws, b1)
            steps = ws
        for b, var, end in steps:
            t = M.tiled(rec, b)
            assert end is None or len(t) < end, (name, b, len(t), end)
            assert s.kernel_for_batch(len(t)) == "wform_ws"
            f, info = getattr(s, SETS[name][2])(t)
            assert _last(pkg, s) == "wform_ws"
            tag = f"wave, workspace form {var} at {len(t)}"
            assert M.copies_identical(f, n) and M.copies_identical(info["status"], n) and M.copies_identical(info["iterations"], n), tag
            d = float(np.abs(f[:n] - fl).max())
            print(f"motion-sets | {tag} | {name} | against the all-LDS form: {d:.2e} N, iteration counts equal "
                  f"{np.array_equal(info['iterations'][:n], il['iterations'])}")
            assert d < (1e-5 if nu == 24 else 1e-7), (tag, d)
            assert np.array_equal(info["iterations"][:n], il["iterations"]), tag
            _converged_rules(pkg, oracle, fix, name, f[:n], info[:n], tag, "wform_ws")


# ---- 3. round-1 family --------------------------------------------------------------------------------------------------------
def test_round_1_family(pkg, lib, oracle, fix):  # noqa: F811
    """QMPC_WFORM=0: the dense kernels -- the only consumer of expand_knot and of Omega(w) in qmpc_device.h -- everything in LDS
    at 360 instances and, tiled beyond the batch the handle names, with the gains in the workspace.  Between the two forms the
    rule of tests/test_gpu_attitude_sets.py::test_round_1_family: two rounding families, so status equal, forces within 1e-7 N
    and iteration counts equal on >= 97 %.  Measured: 5.6e-12 N (all LDS) and 1.8e-11 N (workspace form) from the oracle, iteration
    counts equal on 100 %; the two forms within 1.6e-11 N of each other, iteration counts equal on 100 %."""
    name = "quat_n10"
    rec = _records(pkg, name)
    n = len(rec)
    with _handle(pkg, lib, _params(pkg, lib, name), 4096, QMPC_WFORM=0) as s:
        assert s.kernel_for_batch(n) == "dense_lds"
        f, info = s.solve(rec)
        assert _last(pkg, s) == "dense_lds"
        _converged_rules(pkg, oracle, fix, name, f, info, "round-1 family, all LDS", "dense_lds")
        t = M.tiled(rec, _first_batch_beyond(s, "dense_lds", 4096))
        assert s.kernel_for_batch(len(t)) == "dense_ws"
        ft, it_ = s.solve(t)
        assert _last(pkg, s) == "dense_ws"
    assert M.copies_identical(ft, n) and M.copies_identical(it_["status"], n) and M.copies_identical(it_["iterations"], n)
    _converged_rules(pkg, oracle, fix, name, ft[:n], it_[:n], f"round-1 family, workspace form at {len(t)}", "dense_ws")
    d, share = float(np.abs(ft[:n] - f).max()), float((it_["iterations"][:n] == info["iterations"]).mean())
    print(f"motion-sets | round-1 family | workspace form against all LDS: {d:.2e} N, per rate [rad/s] {{{_per_rate(rec, np.abs(ft[:n] - f))}}}, "
          f"iteration counts equal on {100 * share:.2f} %")
    assert np.array_equal(it_["status"][:n], info["status"]) and d < 1e-7 and share >= 0.97, (d, share)


@pytest.mark.parametrize("name", ["quat_n10", "quat_n20"])
def test_linearisation_at_high_body_rates(pkg, lib, oracle, name):  # noqa: F811
    """qmpc_linearize on the set with the rate fed and with it dropped: A, B and the reference states X against the oracle at
    the 1e-12 of tests/test_gpu_parity.py::test_linearisation_matches_oracle; and the rate really reaches the attitude blocks:
    A with the rate fed differs from A with it dropped.  Measured: A within 6.7e-16 (N=10) and 1.1e-15 (N=20), B within 4.9e-19,
    X within 3.6e-14, the same with the rate fed and dropped."""
    rec = _records(pkg, name)
    p = _params(pkg, lib, name)
    out = {}
    with _handle(pkg, lib, p, len(rec)) as s:
        for drop in (0, 1):
            p.drop_ang_vel = drop
            s.set_params(p)
            A, B, X = s.linearize(rec)
            Ao, Bo, Xo = oracle.linearize(p, rec)
            out[drop] = A
            dA = np.abs(A - Ao).reshape(len(rec), -1).max(axis=1)
            print(f"motion-sets | qmpc_linearize, drop_ang_vel = {drop} | {name} | worst |A - A_oracle| {dA.max():.2e}, per rate [rad/s] "
                  f"{{{_per_rate(rec, dA)}}} | |B - B_oracle| {np.abs(B - Bo).max():.2e} | |X - X_oracle| {np.abs(X - Xo).max():.2e}")
            assert np.abs(X - Xo).max() < 1e-12
            assert np.abs(A - Ao).max() < 1e-12
            assert np.abs(B - Bo).max() < 1e-12
    assert np.abs(out[0] - out[1]).reshape(len(rec), -1).max(axis=1).min() > 1e-3


# ---- 4. reference mode --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,knobs,family", [("quat_n10", {}, "wform_lds"), ("biped8_n16", {}, "wform_lds"),
                                               ("quat_n10", {"QMPC_WFORM": 0}, "dense_lds")])
def test_reference_mode_on_the_wave_kernels(pkg, lib, oracle, name, knobs, family):  # noqa: F811
    """MODE_REFERENCE (truncated AL-iLQR iterates) under the rule of test_reference_mode_on_device_matches_oracle_reference_mode:
    >= 99 % of the instances agree with the oracle to 1e-6 N with identical status and iteration words; swing forces exactly 0.
    (The oracle's reference mode ends most of these records at its 10-iteration cap and a few with LINESEARCH_FAIL: the words
    must agree.)  Measured: QuatMpc 360 of 360 identical (worst 1.4e-8 N; status counts 38 OK / 287 MAX_ITER / 35 LINESEARCH_FAIL),
    with QMPC_WFORM=0 360 of 360 (2.6e-9 N); 8-point 240 of 240 (3.5e-10 N; 21 / 199 / 20)."""
    rec = _records(pkg, name)
    f, info = _run(pkg, lib, name, mode=pkg.MODE_REFERENCE, family=family, **knobs)
    fo, io = _oracle(pkg, oracle, name, 1)
    d = np.abs(f - fo).max(axis=1)
    same = (d < 1e-6) & (info["status"] == io["status"]) & (info["iterations"] == io["iterations"])
    print(f"motion-sets | reference mode, wave kernels {knobs or ''} | {name} | family {family} | {int(same.sum())}/{len(rec)} identical "
          f"(1e-6 N, status, iterations) | worst {d.max():.2e} N, per rate [rad/s] {{{_per_rate(rec, d)}}} | "
          f"status counts {np.bincount(info['status'], minlength=6).tolist()}")
    assert same.mean() >= 0.99
    assert np.abs(f[M.swing_rows(rec, SETS[name][5] // 3)]).max() == 0.0 and np.isfinite(f).all()


@pytest.mark.parametrize("name", ["quat_n10", "quat_n20", "biped8_n16"])
def test_lane_kernel_reference_mode(pkg, lib, oracle, name):  # noqa: F811
    """The rule of tests/test_gpu_lane.py::test_lane_kernel_reference_mode: status and iteration words identical to the oracle's
    on every instance, forces within 1e-6 N on >= 95 % (truncated iterates); swing forces exactly 0.
    Measured: within 1e-6 N on 100 % everywhere; worst 1.9e-10 (QuatMpc N=10), 1.4e-10 (N=20), 3.5e-10 N (8-point)."""
    rec = _records(pkg, name)
    f, info = _run(pkg, lib, name, mode=pkg.MODE_REFERENCE, family="lane", QMPC_VARIANT=4)
    fo, io = _oracle(pkg, oracle, name, 1)
    d = np.abs(f - fo).max(axis=1)
    print(f"motion-sets | reference mode, lane kernel | {name} | family lane | within 1e-6 N on {100 * (d < 1e-6).mean():.2f} % | "
          f"worst {d.max():.2e} N, per rate [rad/s] {{{_per_rate(rec, d)}}} | status counts {np.bincount(info['status'], minlength=6).tolist()}")
    assert np.array_equal(info["status"], io["status"]) and np.array_equal(info["iterations"], io["iterations"])
    assert (d < 1e-6).mean() >= 0.95
    assert np.abs(f[M.swing_rows(rec, SETS[name][5] // 3)]).max() == 0.0 and np.isfinite(f).all()


# ---- 5. lane kernel -----------------------------------------------------------------------------------------------------------
def _lane_handles(pkg, lib):  # noqa: F811
    """quat(10) on the four handles of QMPC_VARIANT=4: lane pairs on the sorted batch (default), QMPC_LANE_PAIR=0, QMPC_LANE_SORT=0, both"""
    if "lane4" not in _cache:
        _cache["lane4"] = {tag: (_lane(pkg, lib) if not knobs else _run(pkg, lib, "quat_n10", family="lane", QMPC_VARIANT=4, **knobs))
                           for tag, knobs in LANE_HANDLES.items()}
    return _cache["lane4"]


def test_lane_kernel_at_every_body_rate(pkg, lib, oracle, fix):  # noqa: F811
    """QMPC_VARIANT=4 on quat(10), four handles: lane pairs or the plain form with half the lanes masked, on the batch sorted by
    stance set or in its own order.  Each handle against the oracle; the order of the batch does not change a bit of either
    form, and the pair form returns the plain form's bits (the contract of
    tests/test_gpu_lane.py::test_lane_pairs_return_the_plain_forms_bits).
    Measured: 1.8e-10 N from the oracle on all four handles, iteration counts equal on 100 %; 0 instances differ between any two.
    (A library whose lane unit negates the rate where qmpc_lane_core.h builds x_init fails this test by 197 N and
    test_lane_kernel_other_sets by 197 N and, on the 8-point model, 495 N.)"""
    runs = _lane_handles(pkg, lib)
    for tag, (f, info) in runs.items():
        _converged_rules(pkg, oracle, fix, "quat_n10", f, info, f"lane kernel ({tag})", "lane")
    for form in ("pairs", "plain"):
        n, d, st, it_ = _bits_differ(runs[form + ", sorted"], runs[form + ", unsorted"])
        print(f"motion-sets | lane kernel ({form}) | sorted against unsorted batch: {n} instances differ, largest difference {d:.2e} N")
        assert n == 0 and st and it_, (form, n, d)
    base = runs["pairs, sorted"]
    for tag in list(LANE_HANDLES)[1:]:
        n, d, st, it_ = _bits_differ(runs[tag], base)
        print(f"motion-sets | lane kernel ({tag}) | against the default handle (pairs, sorted): {n} instances differ, largest difference "
              f"{d:.2e} N, status words equal {st}, iteration words equal {it_}")
        assert st and it_, tag
        assert n == 0, (tag, n, d)


@pytest.mark.parametrize("name", [n for n in SETS if n != "quat_n10"])
def test_lane_kernel_other_sets(pkg, lib, oracle, fix, name):  # noqa: F811
    """The other sets on the default handle of QMPC_VARIANT=4.  Measured: QuatMpc N=5 2.1e-10 N, N=20 1.4e-10 N; 8-point 2.2e-10
    (foot wrench 2.2e-10); iteration counts equal on 100 %."""
    f, info = _lane(pkg, lib, name)
    _converged_rules(pkg, oracle, fix, name, f, info, "lane kernel (pairs, sorted)", "lane")


def test_lane_kernel_full_wavefronts(pkg, lib, oracle, fix):  # noqa: F811
    """The plain 64-lane form launches only when twice the batch exceeds the resident lanes (a handle of 70000, more than 32768
    instances): quat(10) tiled to 33120.  Every copy returns the first one's bits; the unique records follow the oracle and
    return the bits of the 360-instance launches, plain form and lane pairs.  Measured: 0 instances differ from either; 1.8e-10 N
    from the oracle."""
    rec = _records(pkg, "quat_n10")
    n = len(rec)
    runs = _lane_handles(pkg, lib)
    t = M.tiled(rec, 32769)
    f, info = _run(pkg, lib, "quat_n10", cap=70000, rec=t, family="lane", QMPC_VARIANT=4)
    assert M.copies_identical(f, n) and M.copies_identical(info["status"], n) and M.copies_identical(info["iterations"], n)
    _converged_rules(pkg, oracle, fix, "quat_n10", f[:n], info[:n], f"lane kernel, full wavefronts at {len(t)}", "lane")
    first = (f[:n], info[:n])
    for tag in ("plain, sorted", "pairs, sorted"):
        k, d, st, it_ = _bits_differ(first, runs[tag])
        print(f"motion-sets | lane kernel, full wavefronts at {len(t)} | against the {n}-instance launch ({tag}): {k} instances differ, "
              f"largest difference {d:.2e} N, status words equal {st}, iteration words equal {it_}")
        assert st and it_, tag
        assert k == 0, (tag, k, d)


# ---- 6. warm start ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mu0", [0.0, 1e-6])
@pytest.mark.parametrize("knobs,family", [({}, "wform_lds"), ({"QMPC_VARIANT": 4}, "lane")], ids=["wave", "lane"])
def test_warm_start_between_body_rates(pkg, lib, oracle, knobs, family, mu0):  # noqa: F811
    """qmpc_solve_warm at N=10 with the default initial barrier and with the closed loop's low one (ipm_mu0 = 1e-6) on
    warm_pairs(10): a cold call, then the next tick from its trajectory with the body rate at the neighbouring rate of the
    grid, the velocity 0.02 m/s up and, on every third record, the trot diagonals changed over.  The rules of
    test_warm_start_between_every_pair_of_stance_sets against oracle.solve_warm: status equal and all 0, forces within 1e-6 N,
    iteration counts equal on >= 90 % and within one on >= 95 %; swing forces of the new set exactly 0; trajectories within
    1e-5 N.  Measured, warm tick: wave kernel 5.7e-11 N (mu0 = 0) and 5.9e-11 N (1e-6), iteration counts equal on 100 %; lane
    kernel 1.5e-10 and 1.2e-10 N, equal on 100 and 99.72 %, within one on 100 %; 16.7 (21.4) iterations warm against 16.2 (24.4) cold."""
    first, second = M.warm_pairs(pkg, 10)
    B, N = len(first), 10
    p = M.params(pkg, "default_params", N, pkg.MODE_CONVERGED, lib)
    po = M.params(oracle, "default_params", N, 0)
    if mu0:
        p.ipm_mu0 = po.ipm_mu0 = mu0
    # (qmpc_solve_warm does not record its launch for QUERY_LAST_KERNEL: the family is the planner's for a warm-started call of
    # this size under these knobs -- its table -- which shares the plain solve's choice, asked of the handle)
    table = M.plain_plan("quat", N, knobs="QMPC_VARIANT=4" if knobs else "default", kind="warm")
    assert pkg.KERNEL_FAMILY[[fam for b, fam, _ in table if b <= B][-1]] == family
    with _handle(pkg, lib, p, B, **knobs) as s:
        assert s.kernel_for_batch(B) == family
        f0, i0, tu0 = s.solve_warm(first, None)
        f1, i1, tu1 = s.solve_warm(second, tu0)
    if ("warm0", mu0) not in _cache:
        _cache["warm0", mu0] = oracle.solve_warm(po, first, None, threads=8)
    fo0, io0, _ = _cache["warm0", mu0]
    fo1, io1, tuo1 = oracle.solve_warm(po, second, tu0, threads=8)
    di = np.abs(i1["iterations"].astype(int) - io1["iterations"].astype(int))
    print(f"motion-sets | warm start, ipm_mu0 = {mu0} | quat_n10 | family {family} | cold {np.abs(f0 - fo0).max():.2e} N, warm {np.abs(f1 - fo1).max():.2e} N, "
          f"per rate of the second tick [rad/s] {{{_per_rate(second, np.abs(f1 - fo1))}}} | "
          f"iteration counts equal on {100 * (di == 0).mean():.2f} %, within one on {100 * (di <= 1).mean():.2f} % | "
          f"warm iterations {i1['iterations'].mean():.2f} (cold {i0['iterations'].mean():.2f}) | "
          f"status counts {np.bincount(i1['status'], minlength=6).tolist()}")
    assert np.array_equal(i0["status"], io0["status"]) and (i0["status"] == 0).all() and np.abs(f0 - fo0).max() < 1e-6
    assert np.array_equal(i1["status"], io1["status"]) and (i1["status"] == 0).all()
    assert np.abs(f1 - fo1).max() < 1e-6
    assert (di == 0).mean() >= 0.9 and (di <= 1).mean() >= 0.95, np.bincount(di)
    assert np.abs(f1[M.swing_rows(second)]).max() == 0.0
    assert np.abs(tu1.reshape(B, N, 12)[np.repeat(M.swing_rows(second)[:, None, :], N, axis=1)]).max() == 0.0
    assert np.abs(tu1.reshape(B, -1) - tuo1.reshape(B, -1)).max() < 1e-5


# ---- 7. hand-off --------------------------------------------------------------------------------------------------------------
def test_straggler_hand_off(pkg, lib, oracle, fix):  # noqa: F811
    """quat(10) tiled to just beyond the batch from which the default planner takes the lane kernel with the straggler hand-off
    (its table: 14336 at N = 10): the lane kernel stops at its cap and the wave kernel continues what is left from the hand-off's
    records -- the records at 8 and 12 rad/s run across the cap (asserted from the oracle's counts).  Against the same batch on
    the pure lane kernel (QMPC_LANE_CAP=0) under the rules of tests/test_gpu_stance_sets.py::test_straggler_hand_off: status
    equal, forces within 1e-7 N, iteration counts equal on >= 97 %; a second call returns the same bits; every copy the first
    one's bits; the same with QMPC_HANDOFF_RESTART=1.  Measured at 14400 instances, cap 16: 40.6 % of the batch beyond the cap;
    1.8e-10 N from the oracle and 1.4e-10 N from the pure lane kernel, iteration counts equal on 100 %, with and without the restart."""
    name = "quat_n10"
    rec = _records(pkg, name)
    n = len(rec)
    fo, io = _oracle(pkg, oracle, name)
    b = [b for b, fam, _ in M.plain_plan("quat", 10) if fam == 6][0]
    t = M.tiled(rec, b)
    fp, ip = _run(pkg, lib, name, rec=t, family="lane", QMPC_LANE_CAP=0)
    assert M.copies_identical(fp, n) and M.copies_identical(ip["status"], n) and M.copies_identical(ip["iterations"], n)
    fp, ip = fp[:n], ip[:n]
    _converged_rules(pkg, oracle, fix, name, fp, ip, f"lane kernel at {len(t)}, no hand-off", "lane")
    for knobs in ({}, {"QMPC_HANDOFF_RESTART": 1}):
        with _handle(pkg, lib, _params(pkg, lib, name), len(t), **knobs) as s:
            assert s.kernel_for_batch(b) == s.kernel_for_batch(len(t)) == "lane_handoff" and s.kernel_for_batch(b - 1) != "lane_handoff"
            cap = s.query(pkg.QUERY_LANE_CAP, 1)
            handed = float((io["iterations"] > cap).mean())
            assert cap > 0 and handed >= 0.05, (cap, handed)
            f, info = s.solve(t)
            assert _last(pkg, s) == "lane_handoff"
            f2, info2 = s.solve(t)
        tag = f"hand-off at {cap} iterations at {len(t)} {knobs or ''}"
        assert _same(f, f2) and _same(info, info2), tag
        assert M.copies_identical(f, n) and M.copies_identical(info["status"], n) and M.copies_identical(info["iterations"], n), tag
        f, info = f[:n], info[:n]
        _converged_rules(pkg, oracle, fix, name, f, info, tag, "lane_handoff")
        share = float((info["iterations"] == ip["iterations"]).mean())
        d = float(np.abs(f - fp).max())
        print(f"motion-sets | {tag} | {100 * handed:.1f} % of the batch beyond the cap | against the pure lane kernel: {d:.2e} N, "
              f"per rate [rad/s] {{{_per_rate(rec, np.abs(f - fp))}}}, iteration counts equal on {100 * share:.2f} %")
        assert np.array_equal(info["status"], ip["status"]) and d < 1e-7 and share >= 0.97, (tag, d, share)


# ---- 8. per-instance parameter paths ------------------------------------------------------------------------------------------
def test_per_instance_paths_with_uniform_records(pkg, lib, oracle, fix):  # noqa: F811
    """Records that carry the handle's own values return the plain solve's bytes: qmpc_solve_instances on the wave kernel
    (default policy) and on the lane kernel (QMPC_INSTANCES_AUTO, QMPC_LANE_INST_MIN=64; the plain solve on the lane kernel too:
    QMPC_LANE_MIN=64).  drop_ang_vel is the handle's on these paths, not the record's: the per-instance kernels must take it
    from there.  Measured: bytes equal in both; 5.9e-11 N (wave) and 1.8e-10 N (lane_handoff) from the oracle."""
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
def test_random_variants_at_every_body_rate(pkg, lib, oracle, policy):  # noqa: F811
    """quat(10) with a robot of its own per instance (motion_sets.variants: pkg.random_go1_variants' mass, inertia, friction,
    force bound, Q and R) on the wave kernel (default policy) and on the lane kernel (auto, QMPC_LANE_INST_MIN=64), against the
    oracle solved per instance with that instance's parameters and the rate fed, the way and under the tolerances of
    tests/test_gpu_instance_params.py::test_random_variants_against_the_oracle: more than 95 % converge, every status word is
    the oracle's, and where that is 0 the forces are within 1e-6 N -- here on all 360 instances (the CPU suite holds the
    oracle to status 0 on every one).  Measured: 1.7e-10 N (wave kernel, at 12 rad/s) and 2.9e-10 N (lane_handoff) from the oracle;
    every status 0 on both sides; iteration counts equal on 99.72 / 100 %."""
    rec = _records(pkg, "quat_n10")
    n = len(rec)
    p = _params(pkg, lib, "quat_n10")
    ip = M.variants(pkg, p)
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
    d = np.abs(f - fo)
    print(f"motion-sets | solve_instances, random variants, {policy} policy | quat_n10 | family {fam} | "
          f"worst |f - f_oracle| {d.max():.2e} N, per rate [rad/s] {{{_per_rate(rec, d)}}} | iteration counts equal on "
          f"{100 * (info['iterations'] == ito).mean():.2f} % | status counts {np.bincount(info['status'], minlength=6).tolist()} "
          f"(oracle {np.bincount(so, minlength=6).tolist()})")
    assert (so == 0).all()
    assert np.array_equal(info["status"], so)
    assert d.max() <= 1e-6


# ---- 9. device closed loop ----------------------------------------------------------------------------------------------------
def test_device_closed_loop_from_high_body_rates(pkg, lib):  # noqa: F811
    """Eight standing robots (motion_sets.loop_states) that start with body rates of 2, 4 and 8 rad/s about yaw and about a
    random body axis, two at rest; 40 ticks in stand mode at N = 10 with drop_ang_vel = 0.  The device loop against the same
    ticks built from the host classes, with the harness and bounds of
    tests/test_gpu_parity.py::test_device_closed_loop_matches_host_classes_tick_for_tick: contact flags exact, forces <= 1e-6 N
    at every tick, final states <= 1e-8; the persistent kernel and the per-tick form return the same bytes
    (test_persistent_loop_kernel_equals_the_per_tick_sequence); every spinning robot is slower after the 40 ticks than at the
    start; and the loop tick hands the rate to the solve: the first tick's forces differ by more than 1 N from those of the
    same loop with drop_ang_vel = 1 on every spinning robot, and by nothing on the two at rest.
    Measured: forces and states equal to the host classes' to the last bit (the host tick launches the same kernel for one robot);
    the two launch forms the same bytes; |ang_vel_body| after 40 ticks (0.2 s) 2 -> 0.06, 4 -> 0.08, 8 -> 0.13 rad/s about yaw and
    2 -> 0.07, 4 -> 0.08, 8 -> 0.12 rad/s about the random axes (0.05 rad/s on the two that start at rest); first tick's forces 15, 38,
    88, 12, 19 and 70 N from those of the loop with the rate dropped, 0 N on the two at rest."""
    import __graft_entry__ as g

    host = C.CDLL(str(g.build_host()))
    vp = C.c_void_p
    host.qh_loop_create_opts.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, vp, vp]; host.qh_loop_create_opts.restype = vp
    for fn in ("qh_loop_tick", "qh_loop_destroy", "qh_loop_device_status"):
        getattr(host, fn).argtypes = [vp]
    host.qh_loop_export.argtypes = [vp, vp]
    T, N = 40, 10
    lp = pkg.default_loop_params(lib)
    st_init = M.loop_states(pkg, lib, lp)
    B = len(st_init)
    before = np.linalg.norm(st_init["ang_vel_body"], axis=1)
    assert np.allclose(before, [r for _, r in M.LOOP_RATES], rtol=0, atol=1e-14)
    out = {}
    for drop in (0, 1):
        p = M.params(pkg, "default_params", N, pkg.MODE_CONVERGED, lib)
        p.drop_ang_vel = drop
        s = pkg.Solver(p, B, device=0, lib=lib)
        out[drop] = s.loop_run(st_init, T if drop == 0 else 1, lp, trace=True)
        s.close()
    st, tf, tc = out[0]
    assert (st["tick"] == T).all() and (st["status"] == 0).all(), st["status"]
    worst_f = worst_x = 0.0
    for i in range(B):
        h = host.qh_loop_create_opts(str(pkg.LIB_PATH).encode(), N, pkg.MODE_CONVERGED, 0, C.addressof(lp), st_init[i:i + 1].ctypes.data)
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
    after = np.linalg.norm(st["ang_vel_body"], axis=1)
    fed = np.abs(tf[0] - out[1][1][0]).max(axis=1)
    sha = hashlib.sha256(st.tobytes() + tf.tobytes() + tc.tobytes()).hexdigest()
    print(f"motion-sets | device closed loop, {B} robots x {T} ticks in stand mode | worst force difference to the host classes "
          f"{worst_f:.2e} N, worst state difference {worst_x:.2e} | |ang_vel_body| [rad/s] " +
          ", ".join(f"{k or 'none'} {a}: {b:.3f} -> {c:.3f}" for (k, a), b, c in zip(M.LOOP_RATES, before, after)) +
          f" | first tick's forces against drop_ang_vel = 1 [N] {fed.round(2).tolist()}"
          f" | iterations of the last tick {st['iterations'].astype(int).tolist()}")
    assert worst_f <= 1e-6 and worst_x <= 1e-8
    spinning = np.array([k is not None for k, _ in M.LOOP_RATES])
    assert (after[spinning] < before[spinning]).all(), (before, after)
    assert (fed[spinning] > 1.0).all() and (fed[~spinning] == 0.0).all(), fed
    worker = Path(__file__).resolve().parent / "_loop_motion_worker.py"
    sums = {}
    for fused in ("0", "1"):
        r = subprocess.run([sys.executable, str(worker), str(T), str(N)], env=dict(os.environ, QMPC_LOOP_FUSED=fused),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        sums[fused] = [l for l in r.stdout.splitlines() if l.startswith("SHA")][0].split()[1]
    print(f"motion-sets | device closed loop | per-tick form and persistent kernel: the same bytes {sums['0'] == sums['1']}")
    assert sums["0"] == sums["1"] and sha in sums.values()
