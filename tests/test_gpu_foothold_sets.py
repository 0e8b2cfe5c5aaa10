"""GPU suite (-m gpu): every solve path on footholds and references far from nominal (tests/foothold_sets.py).

The state generators place every foot within 5 cm of the nominal 40 x 28 cm rectangle at z = -0.30 m (the 8-point model within
3 cm of two fixed foot centres), draw pos_ref_body at sigma = 2 cm and vel_ref_body within 0.5 / 0.1 m/s with z = 0, and leave
acc_ref_body at 0; the stance, attitude and motion suites keep those.  The foot positions are the operand of the wrench map
Wr = [c I ; Bw0], of G = sum V D^-1 V', of the two 6 x 6 Cholesky factorisations per knot, of the B blocks of qmpc_linearize and of
the gravity-torque and lever-arm terms of every rollout, in every copy (qmpc_wform.h, qmpc_wform_body.inc, qmpc_lane_core.h,
the round-1 family in qmpc_device.h, the per-instance and warm instances, the ConvexMpc and 8-point policies): with all feet
near one rectangle a lever arm taken from the wrong leg's z, a constant standing in for a foot coordinate or a block that is
right only for feet symmetric about the centre of mass passes.  The references enter the cost gradient of every knot, and with
acc_ref = 0 the quadratic term of the reference trajectory is dead code.  The records carry ten foothold kinds -- a 10 x 7 cm
rectangle, one of 80 x 56 cm, feet on the body's x or y axis, the whole polygon 0.3 m ahead or 0.25 m aside of the centre of
mass, 24 cm of height difference, crossed front legs, 8 and 60 cm of body height -- crossed with pos_ref + 0.3 m, vel_ref +
3 m/s and acc_ref + 5 m/s^2 along a random direction, z included (QuatMpc N = 5, 10, 20; ConvexMpc N = 10, 20; seven kinds of the
8-point model at N = 16); the CPU suite (tests/test_foothold_sets_cpu.py) certifies the oracle on the same records, keeps them
inside the solver's envelope and shows that footholds and references move the forces.

Rules, unless a test says otherwise (the project's own for the converged mode, those of tests/test_gpu_stance_sets.py, whose
handle, knob and comparison helpers this module takes): status words equal to the oracle's and all 0; forces within 1e-6 N
(8-point model: corner forces 1e-5, foot wrench 1e-7); swing forces exactly 0; iteration counts equal on >= 97 %; first-knot
forces within 1e-6 (1e-5) of the stored certified points (tests/golden/foothold_fixtures.npz).  No instance is left out of a
comparison.  Every test reads back the kernel family that ran.  Each prints a line `foothold-sets | ...` with the family, the
worst force difference per foothold kind and per reference class and the share of equal iteration counts
(profiles/r21_foothold_sets.txt is made of them)."""
import contextlib
import ctypes as C
import hashlib
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import foothold_sets as F
import motion_sets as M
from test_gpu_stance_sets import LANE_HANDLES, _bits_differ, _first_batch_beyond, _handle, _last, _same, _wrench8
from test_gpu_stance_sets import lib  # noqa: F401  (the fixture: raises if the HIP extension is missing, no fallback)

pytestmark = pytest.mark.gpu

# name: (records, default params, Solver call, oracle call, horizon, force components, model name of the planner's table, model)
SETS = {
    "quat_n5": (lambda pkg, **kw: F.quat(pkg, 5, **kw), "default_params", "solve", "solve", 5, 12, "quat", "quat"),
    "quat_n10": (lambda pkg, **kw: F.quat(pkg, 10, **kw), "default_params", "solve", "solve", 10, 12, "quat", "quat"),
    "quat_n20": (lambda pkg, **kw: F.quat(pkg, 20, **kw), "default_params", "solve", "solve", 20, 12, "quat", "quat"),
    "convex_n10": (lambda pkg, **kw: F.convex(pkg, 10, **kw), "default_convex_params", "convex_solve", "convex_solve", 10, 12, "convex", "convex"),
    "convex_n20": (lambda pkg, **kw: F.convex(pkg, 20, **kw), "default_convex_params", "convex_solve", "convex_solve", 20, 12, "convex", "convex"),
    "biped8_n16": (lambda pkg, **kw: F.biped8(pkg, 16, **kw), "default_biped8_params", "solve8", "solve8", 16, 24, "quat8", "biped8"),
}
_cache = {}


@pytest.fixture(scope="module")
def fix():
    return np.load(Path(__file__).parent / "golden" / "foothold_fixtures.npz")


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


def _lane_knobs(name):
    """the lane kernel for a plain solve of the set: QuatMpc and the 8-point model by QMPC_VARIANT=4; ConvexMpc's lane form
    under its own knob, the way tests/test_gpu_convex_instance_lane.py brings it down to small batches"""
    return {"QMPC_LANE_MIN": 1} if SETS[name][7] == "convex" else {"QMPC_VARIANT": 4}


def _run(pkg, lib, name, cap=None, rec=None, mode=None, family=None, **knobs):  # noqa: F811
    """One solve of the set (or of `rec`) on a fresh handle; asserts the family that ran.  (forces, info)"""
    rec = _records(pkg, name) if rec is None else rec
    with _handle(pkg, lib, _params(pkg, lib, name, mode), cap or len(rec), **knobs) as s:
        planned = s.kernel_for_batch(len(rec))
        f, info = getattr(s, SETS[name][2])(rec)
        ran = _last(pkg, s)
    assert ran == planned and (family is None or ran == family), (name, knobs, planned, ran, family)
    return f, info


def _per(name, d, what="kind", second=None):
    """'bunched: 1.2e-11, ...': the largest of d [B] or [B, k] over the records of each foothold kind (what="class": of each
    reference class) of the set; `second`: of these (kind, class) arrays instead of the set's own"""
    model, N = SETS[name][7], SETS[name][4]
    kind, cls = second if second is not None else F.cells(model, N)
    idx, names = (kind, F.KINDS8 if model == "biped8" else F.KINDS) if what == "kind" else (cls, F.CLASSES)
    d = np.asarray(d).reshape(len(idx), -1).max(axis=1)
    return ", ".join(f"{names[c]}: {d[idx == c].max():.1e}" for c in range(len(names)) if (idx == c).any())


def _both(name, d):
    return f"per kind {{{_per(name, d)}}}, per reference class {{{_per(name, d, 'class')}}}"


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
    print(f"foothold-sets | {tag} | {name} | family {family} | worst |f - f_oracle| {d:.2e} N, {_both(name, np.abs(f - fo))}"
          + (f" (foot wrench {dw:.2e})" if dw is not None else "") + f" | iteration counts equal on {100 * share:.2f} %"
          + (f" | certified points within {dc:.2e} N" if dc is not None else "")
          + f" | status counts {np.bincount(info['status'], minlength=6).tolist()}")
    assert np.array_equal(info["status"], io["status"]) and (info["status"] == 0).all(), tag
    assert d < (1e-5 if nu == 24 else 1e-6), (tag, d)
    if nu == 24:
        assert dw < 1e-7, (tag, dw)
    assert np.abs(f[F.swing_rows(rec, nu // 3)]).max() == 0.0, tag
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
        _cache["lane", name] = _run(pkg, lib, name, family="lane", **_lane_knobs(name))
    return _cache["lane", name]


# ---- 1. wave kernels, everything in LDS ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SETS))
def test_wave_kernels_in_lds(pkg, lib, oracle, fix, name):  # noqa: F811
    """Default planner at the set's own size (320 / 288 / 224 instances): the wrench-form kernel with everything in LDS;
    ConvexMpc through convex_solve.  Measured, worst force difference to the oracle (share of equal iteration counts where
    not 100 %): QuatMpc N=5 1.5e-11, N=10 4.5e-11, N=20 1.6e-10 N (99.31 %: 286 of 288); ConvexMpc N=10 4.5e-11, N=20 1.7e-10 N (98.75 %);
    8-point corner forces 5.3e-11, foot wrench 6.2e-11 N; certified points within 1.9e-11 N."""
    f, info = _wave_lds(pkg, lib, name)
    _converged_rules(pkg, oracle, fix, name, f, info, "wave, all LDS", "wform_lds")


# ---- 2. wave kernels, workspace forms -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SETS))
def test_wave_kernels_workspace_forms(pkg, lib, oracle, fix, name):  # noqa: F811
    """The set tiled to just beyond the batch at which the planner leaves the all-LDS form (asked of the handle), and -- where
    the planner's table (tests/golden/kernel_plans.txt.gz) has a second workspace form for the horizon: the slack arrays out as
    well -- to just beyond that batch too: QuatMpc N=10 / 5 and ConvexMpc N=10 take the gains-in-workspace form, QuatMpc N=20,
    ConvexMpc N=20 and the 8-point model both.  Against the all-LDS form on the unique records: forces within 1e-7 N (8-point
    1e-5) and identical iteration counts (the forms differ in where their arrays live); every copy returns the first one's bits;
    and the oracle's rules.  Measured: every workspace form returns the all-LDS form's BITS on every set (0.0 N), so the figures
    of test_wave_kernels_in_lds."""
    rec, (model, N, nu) = _records(pkg, name), (SETS[name][6], SETS[name][4], SETS[name][5])
    n = len(rec)
    fl, il = _wave_lds(pkg, lib, name)
    with _handle(pkg, lib, _params(pkg, lib, name), 4096) as s:
        b1 = _first_batch_beyond(s, "wform_lds", 4096)
        assert b1 > n and s.kernel_for_batch(b1) == "wform_ws"
        steps = [(b1, 5, None)]
        if N != 5:          # (the table enumerates N = 4, 10, ...: the N = 5 handle is asked alone)
            plan = F.plain_plan(model, N)
            ws = [(b, var, plan[i + 1][0] if i + 1 < len(plan) else None) for i, (b, fam, var) in enumerate(plan) if fam == 2]
            assert ws[0][0] == b1 and [v for _, v, _ in ws] == ([5] if N == 10 else [5, 6]), (ws, b1)
            steps = ws
        for b, var, end in steps:
            t = F.tiled(rec, b)
            assert end is None or len(t) < end, (name, b, len(t), end)
            assert s.kernel_for_batch(len(t)) == "wform_ws"
            f, info = getattr(s, SETS[name][2])(t)
            assert _last(pkg, s) == "wform_ws"
            tag = f"wave, workspace form {var} at {len(t)}"
            assert F.copies_identical(f, n) and F.copies_identical(info["status"], n) and F.copies_identical(info["iterations"], n), tag
            d = float(np.abs(f[:n] - fl).max())
            print(f"foothold-sets | {tag} | {name} | against the all-LDS form: {d:.2e} N, iteration counts equal "
                  f"{np.array_equal(info['iterations'][:n], il['iterations'])}")
            assert d < (1e-5 if nu == 24 else 1e-7), (tag, d)
            assert np.array_equal(info["iterations"][:n], il["iterations"]), tag
            _converged_rules(pkg, oracle, fix, name, f[:n], info[:n], tag, "wform_ws")


# ---- 3. round-1 family --------------------------------------------------------------------------------------------------------
def test_round_1_family(pkg, lib, oracle, fix):  # noqa: F811
    """QMPC_WFORM=0: the dense kernels -- the copy of the lever-arm terms in qmpc_device.h -- everything in LDS at 320 instances
    and, tiled beyond the batch the handle names, with the gains in the workspace.  Between the two forms the rule of
    tests/test_gpu_attitude_sets.py::test_round_1_family: two rounding families, so status equal, forces within 1e-7 N and
    iteration counts equal on >= 97 %.  Measured: 1.1e-11 N (all LDS) and 1.1e-11 N (workspace form) from the oracle, iteration counts equal on
    100 %; the two forms within 5.2e-12 N of each other, iteration counts equal on 100 %."""
    name = "quat_n10"
    rec = _records(pkg, name)
    n = len(rec)
    with _handle(pkg, lib, _params(pkg, lib, name), 4096, QMPC_WFORM=0) as s:
        assert s.kernel_for_batch(n) == "dense_lds"
        f, info = s.solve(rec)
        assert _last(pkg, s) == "dense_lds"
        _converged_rules(pkg, oracle, fix, name, f, info, "round-1 family, all LDS", "dense_lds")
        t = F.tiled(rec, _first_batch_beyond(s, "dense_lds", 4096))
        assert s.kernel_for_batch(len(t)) == "dense_ws"
        ft, it_ = s.solve(t)
        assert _last(pkg, s) == "dense_ws"
    assert F.copies_identical(ft, n) and F.copies_identical(it_["status"], n) and F.copies_identical(it_["iterations"], n)
    _converged_rules(pkg, oracle, fix, name, ft[:n], it_[:n], f"round-1 family, workspace form at {len(t)}", "dense_ws")
    d, share = float(np.abs(ft[:n] - f).max()), float((it_["iterations"][:n] == info["iterations"]).mean())
    print(f"foothold-sets | round-1 family | workspace form against all LDS: {d:.2e} N, {_both(name, np.abs(ft[:n] - f))}, "
          f"iteration counts equal on {100 * share:.2f} %")
    assert np.array_equal(it_["status"][:n], info["status"]) and d < 1e-7 and share >= 0.97, (d, share)


@pytest.mark.parametrize("name", ["quat_n10", "quat_n20"])
def test_linearisation_on_displaced_footholds(pkg, lib, oracle, name):  # noqa: F811
    """qmpc_linearize on the set: A, B and the rollout X against the oracle at the 1e-12 of
    tests/test_gpu_parity.py::test_linearisation_matches_oracle; the feet reach the blocks -- B differs from B on the
    generator's footholds on EVERY record.
    X is the rollout from the record's state under U = u_ref (include/qmpc.h), not the reference trajectory of the cost: by
    the call's definition pos_ref / vel_ref / acc_ref do not enter it, in the oracle no more than in the kernel, so a rule `X
    differs on every record of reference classes 1 - 3` cannot be met by the oracle itself (its X is bit-identical on the
    generator's references, asserted here).  What is held instead is the call's contract: A, B and X are the same BITS with
    the references moved as without.  That the references reach the kernels is held by every solve test of this module
    against the oracle, whose forces they move by 8 ... 169 N in the median (tests/test_foothold_sets_cpu.py).
    Measured: A within 1.6e-15 (N=10) and 1.1e-15 (N=20), B within 9.8e-19, X within 8.5e-14 of the oracle; B at least 2.2e-2 (1.3e-2)
    from B on the generator's footholds; X differs on 216 of 320 (188 of 288) records; the same bits on the generator's references."""
    rec = _records(pkg, name)
    N = SETS[name][4]
    no_refs = SETS[name][0](pkg, references=False)
    p = _params(pkg, lib, name)
    with _handle(pkg, lib, p, len(rec)) as s:
        A, B, X = s.linearize(rec)
        _, Bg, Xg = s.linearize(SETS[name][0](pkg, footholds=False))
        Ar, Br, Xr = s.linearize(no_refs)
    po = getattr(oracle, SETS[name][1])(N, 0)
    Ao, Bo, Xo = oracle.linearize(po, rec)
    dB = np.abs(B - Bo).reshape(len(rec), -1).max(axis=1)
    moved_B = np.abs(B - Bg).reshape(len(rec), -1).max(axis=1)
    moved_X = np.abs(X - Xg).reshape(len(rec), -1).max(axis=1)
    print(f"foothold-sets | qmpc_linearize | {name} | worst |A - A_oracle| {np.abs(A - Ao).max():.2e} | |B - B_oracle| {dB.max():.2e}, "
          f"per kind {{{_per(name, dB)}}} | |X - X_oracle| {np.abs(X - Xo).max():.2e}, per kind "
          f"{{{_per(name, np.abs(X - Xo))}}} | |B - B(generator's footholds)| at least {moved_B.min():.2e}, "
          f"X differs on {int((moved_X > 0).sum())} of {len(rec)} records (the rollout under u_ref) | same bits on the generator's references {_same(X, Xr)}")
    assert np.abs(X - Xo).max() < 1e-12
    assert np.abs(A - Ao).max() < 1e-12
    assert np.abs(B - Bo).max() < 1e-12
    assert (moved_B > 1e-6).all(), np.where(moved_B <= 1e-6)[0]
    assert _same(A, Ar) and _same(B, Br) and _same(X, Xr)
    assert _same(Xo, oracle.linearize(po, no_refs)[2])


# ---- 4. reference mode --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["quat_n10", "biped8_n16"])
def test_reference_mode_on_the_wave_kernels(pkg, lib, oracle, name):  # noqa: F811
    """MODE_REFERENCE (truncated AL-iLQR iterates) under the rule of test_reference_mode_on_device_matches_oracle_reference_mode:
    >= 99 % of the instances agree with the oracle to 1e-6 N with identical status and iteration words; swing forces exactly 0.
    (The oracle's reference mode ends most of these records at its 10-iteration cap and some with LINESEARCH_FAIL: the words
    must agree.)  Measured: QuatMpc 320 of 320 identical (worst 7.5e-7 N, on an `as drawn` and a vel_ref + 3 u record;
    status counts 60 OK / 215 MAX_ITER / 45 LINESEARCH_FAIL); 8-point 224 of 224 (3.3e-10 N; 47 / 146 / 31)."""
    rec = _records(pkg, name)
    f, info = _run(pkg, lib, name, mode=pkg.MODE_REFERENCE, family="wform_lds")
    fo, io = _oracle(pkg, oracle, name, 1)
    d = np.abs(f - fo).max(axis=1)
    same = (d < 1e-6) & (info["status"] == io["status"]) & (info["iterations"] == io["iterations"])
    print(f"foothold-sets | reference mode, wave kernels | {name} | family wform_lds | {int(same.sum())}/{len(rec)} identical "
          f"(1e-6 N, status, iterations) | worst {d.max():.2e} N, {_both(name, d)} | "
          f"status counts {np.bincount(info['status'], minlength=6).tolist()}")
    assert same.mean() >= 0.99
    assert np.abs(f[F.swing_rows(rec, SETS[name][5] // 3)]).max() == 0.0 and np.isfinite(f).all()


@pytest.mark.parametrize("name", ["quat_n10", "quat_n20", "biped8_n16"])
def test_lane_kernel_reference_mode(pkg, lib, oracle, name):  # noqa: F811
    """The rule of tests/test_gpu_lane.py::test_lane_kernel_reference_mode: status and iteration words identical to the oracle's
    on every instance, forces within 1e-6 N on >= 95 % (truncated iterates); swing forces exactly 0.
    Measured: within 1e-6 N on 100 % everywhere; worst 4.2e-10 (QuatMpc N=10), 1.8e-10 (N=20), 3.3e-10 N (8-point)."""
    rec = _records(pkg, name)
    f, info = _run(pkg, lib, name, mode=pkg.MODE_REFERENCE, family="lane", QMPC_VARIANT=4)
    fo, io = _oracle(pkg, oracle, name, 1)
    d = np.abs(f - fo).max(axis=1)
    print(f"foothold-sets | reference mode, lane kernel | {name} | family lane | within 1e-6 N on {100 * (d < 1e-6).mean():.2f} % | "
          f"worst {d.max():.2e} N, {_both(name, d)} | status counts {np.bincount(info['status'], minlength=6).tolist()}")
    assert np.array_equal(info["status"], io["status"]) and np.array_equal(info["iterations"], io["iterations"])
    assert (d < 1e-6).mean() >= 0.95
    assert np.abs(f[F.swing_rows(rec, SETS[name][5] // 3)]).max() == 0.0 and np.isfinite(f).all()


# ---- 5. lane kernel -----------------------------------------------------------------------------------------------------------
def _lane_handles(pkg, lib):  # noqa: F811
    """quat(10) on the four handles of QMPC_VARIANT=4: lane pairs on the sorted batch (default), QMPC_LANE_PAIR=0, QMPC_LANE_SORT=0, both"""
    if "lane4" not in _cache:
        _cache["lane4"] = {tag: (_lane(pkg, lib) if not knobs else _run(pkg, lib, "quat_n10", family="lane", QMPC_VARIANT=4, **knobs))
                           for tag, knobs in LANE_HANDLES.items()}
    return _cache["lane4"]


def test_lane_kernel_on_every_foothold_kind(pkg, lib, oracle, fix):  # noqa: F811
    """QMPC_VARIANT=4 on quat(10), four handles: lane pairs or the plain form with half the lanes masked, on the batch sorted by
    stance set or in its own order.  Each handle against the oracle; the order of the batch does not change a bit of either
    form, and the pair form returns the plain form's bits (the contract of
    tests/test_gpu_lane.py::test_lane_pairs_return_the_plain_forms_bits).  The lane kernel keeps the feedback part of its gain in
    single precision: long lever arms and large first steps are where that would show in the iteration counts.
    Measured: 1.4e-10 N from the oracle on all four handles, iteration counts equal on 100 %; 0 instances differ between any two.
    (A library whose lane unit takes leg 0's z for every leg's lever arm, or drops the acc_ref term of the reference
    trajectory, fails this test and test_lane_kernel_other_sets: profiles/r21_foothold_sets.txt has the newtons.)"""
    runs = _lane_handles(pkg, lib)
    for tag, (f, info) in runs.items():
        _converged_rules(pkg, oracle, fix, "quat_n10", f, info, f"lane kernel ({tag})", "lane")
    for form in ("pairs", "plain"):
        n, d, st, it_ = _bits_differ(runs[form + ", sorted"], runs[form + ", unsorted"])
        print(f"foothold-sets | lane kernel ({form}) | sorted against unsorted batch: {n} instances differ, largest difference {d:.2e} N")
        assert n == 0 and st and it_, (form, n, d)
    base = runs["pairs, sorted"]
    for tag in list(LANE_HANDLES)[1:]:
        n, d, st, it_ = _bits_differ(runs[tag], base)
        print(f"foothold-sets | lane kernel ({tag}) | against the default handle (pairs, sorted): {n} instances differ, largest difference "
              f"{d:.2e} N, status words equal {st}, iteration words equal {it_}")
        assert st and it_, tag
        assert n == 0, (tag, n, d)


@pytest.mark.parametrize("name", [n for n in SETS if n != "quat_n10"])
def test_lane_kernel_other_sets(pkg, lib, oracle, fix, name):  # noqa: F811
    """The other sets on the default lane handle (QMPC_VARIANT=4; ConvexMpc's lane form under QMPC_LANE_MIN=1).
    Measured: QuatMpc N=5 2.8e-10 N (iteration counts equal on 99.69 %), N=20 5.3e-10 N (99.31 %); ConvexMpc N=10 1.2e-10 N (100 %), N=20
    8.1e-10 N (99.69 %); 8-point 1.8e-10 N, foot wrench 2.1e-10 N (99.55 %): 1787 of the 1792 records of the six sets keep the oracle's count."""
    f, info = _lane(pkg, lib, name)
    _converged_rules(pkg, oracle, fix, name, f, info, "lane kernel (pairs, sorted)", "lane")


def test_lane_kernel_full_wavefronts(pkg, lib, oracle, fix):  # noqa: F811
    """The plain 64-lane form launches only when twice the batch exceeds the resident lanes (a handle of 70000, more than 32768
    instances): quat(10) tiled to 32960.  Every copy returns the first one's bits; the unique records follow the oracle and
    return the bits of the 320-instance launches, plain form and lane pairs.  Measured: 0 instances differ from either; 1.4e-10 N from the oracle."""
    rec = _records(pkg, "quat_n10")
    n = len(rec)
    runs = _lane_handles(pkg, lib)
    t = F.tiled(rec, 32769)
    f, info = _run(pkg, lib, "quat_n10", cap=70000, rec=t, family="lane", QMPC_VARIANT=4)
    assert F.copies_identical(f, n) and F.copies_identical(info["status"], n) and F.copies_identical(info["iterations"], n)
    _converged_rules(pkg, oracle, fix, "quat_n10", f[:n], info[:n], f"lane kernel, full wavefronts at {len(t)}", "lane")
    first = (f[:n], info[:n])
    for tag in ("plain, sorted", "pairs, sorted"):
        k, d, st, it_ = _bits_differ(first, runs[tag])
        print(f"foothold-sets | lane kernel, full wavefronts at {len(t)} | against the {n}-instance launch ({tag}): {k} instances differ, "
              f"largest difference {d:.2e} N, status words equal {st}, iteration words equal {it_}")
        assert st and it_, tag
        assert k == 0, (tag, k, d)


# ---- 6. warm start ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mu0", [0.0, 1e-6])
@pytest.mark.parametrize("knobs,family", [({}, "wform_lds"), ({"QMPC_VARIANT": 4}, "lane")], ids=["wave", "lane"])
def test_warm_start_onto_other_footholds(pkg, lib, oracle, knobs, family, mu0):  # noqa: F811
    """qmpc_solve_warm at N=10 with the default initial barrier and with the closed loop's low one (ipm_mu0 = 1e-6) on
    warm_pairs(10): a cold call, then the same record one controller tick later -- the feet moved by -0.005 lin_vel_body, the
    velocity 0.02 m/s up -- and, on every third record, the trot diagonals changed over with the landing legs on the footholds of
    the next kind of the grid, so the previous trajectory was solved for another geometry.  The rules of
    tests/test_gpu_motion_sets.py::test_warm_start_between_body_rates against oracle.solve_warm: status equal and all 0, forces
    within 1e-6 N, iteration counts equal on >= 90 % and within one on >= 95 %; swing forces of the new set exactly 0;
    trajectories within 1e-5 N.  Measured, warm tick: wave kernel 2.6e-11 N (mu0 = 0) and 6.8e-11 N (1e-6), iteration counts equal on 100 %; lane
    kernel 1.8e-10 and 6.0e-10 N, equal on 100 and 99.69 %, within one on 100 %; 14.6 (18.4) iterations warm against 15.9 (22.8) cold."""
    first, second = F.warm_pairs(pkg, 10)
    B, N = len(first), 10
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    po = oracle.default_params(N, 0)
    if mu0:
        p.ipm_mu0 = po.ipm_mu0 = mu0
    # (qmpc_solve_warm does not record its launch for QUERY_LAST_KERNEL: the family is the planner's for a warm-started call of
    # this size under these knobs -- its table -- which shares the plain solve's choice, asked of the handle)
    table = F.plain_plan("quat", N, knobs="QMPC_VARIANT=4" if knobs else "default", kind="warm")
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
    print(f"foothold-sets | warm start, ipm_mu0 = {mu0} | quat_n10 | family {family} | cold {np.abs(f0 - fo0).max():.2e} N, warm {np.abs(f1 - fo1).max():.2e} N, "
          f"{_both('quat_n10', np.abs(f1 - fo1))} | "
          f"iteration counts equal on {100 * (di == 0).mean():.2f} %, within one on {100 * (di <= 1).mean():.2f} % | "
          f"warm iterations {i1['iterations'].mean():.2f} (cold {i0['iterations'].mean():.2f}) | "
          f"status counts {np.bincount(i1['status'], minlength=6).tolist()}")
    assert np.array_equal(i0["status"], io0["status"]) and (i0["status"] == 0).all() and np.abs(f0 - fo0).max() < 1e-6
    assert np.array_equal(i1["status"], io1["status"]) and (i1["status"] == 0).all()
    assert np.abs(f1 - fo1).max() < 1e-6
    assert (di == 0).mean() >= 0.9 and (di <= 1).mean() >= 0.95, np.bincount(di)
    assert np.abs(f1[F.swing_rows(second)]).max() == 0.0
    assert np.abs(tu1.reshape(B, N, 12)[np.repeat(F.swing_rows(second)[:, None, :], N, axis=1)]).max() == 0.0
    assert np.abs(tu1.reshape(B, -1) - tuo1.reshape(B, -1)).max() < 1e-5


# ---- 7. hand-off --------------------------------------------------------------------------------------------------------------
def test_straggler_hand_off(pkg, lib, oracle, fix):  # noqa: F811
    """quat(10) tiled to just beyond the batch from which the default planner takes the lane kernel with the straggler hand-off
    (its table: 14336 at N = 10): the lane kernel stops at its cap and the wave kernel continues what is left from the hand-off's
    records -- at least 5 % of the batch, asserted from the oracle's counts (the aside kind runs to 36 iterations).  Against the
    same batch on the pure lane kernel (QMPC_LANE_CAP=0) under the rules of
    tests/test_gpu_stance_sets.py::test_straggler_hand_off: status equal, forces within 1e-7 N, iteration counts equal on
    >= 97 %; a second call returns the same bits; every copy the first one's bits; the same with QMPC_HANDOFF_RESTART=1.
    Measured at 14400 instances, cap 16: 31.2 % of the batch beyond the cap; 1.4e-10 N from the oracle and 1.3e-10 N from the pure
    lane kernel, iteration counts equal on 100 %, with and without the restart."""
    name = "quat_n10"
    rec = _records(pkg, name)
    n = len(rec)
    fo, io = _oracle(pkg, oracle, name)
    b = [b for b, fam, _ in F.plain_plan("quat", 10) if fam == 6][0]
    t = F.tiled(rec, b)
    fp, ip = _run(pkg, lib, name, rec=t, family="lane", QMPC_LANE_CAP=0)
    assert F.copies_identical(fp, n) and F.copies_identical(ip["status"], n) and F.copies_identical(ip["iterations"], n)
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
        assert F.copies_identical(f, n) and F.copies_identical(info["status"], n) and F.copies_identical(info["iterations"], n), tag
        f, info = f[:n], info[:n]
        _converged_rules(pkg, oracle, fix, name, f, info, tag, "lane_handoff")
        share = float((info["iterations"] == ip["iterations"]).mean())
        d = float(np.abs(f - fp).max())
        print(f"foothold-sets | {tag} | {100 * handed:.1f} % of the batch beyond the cap | against the pure lane kernel: {d:.2e} N, "
              f"{_both(name, np.abs(f - fp))}, iteration counts equal on {100 * share:.2f} %")
        assert np.array_equal(info["status"], ip["status"]) and d < 1e-7 and share >= 0.97, (tag, d, share)


# ---- 8. per-instance parameter paths ------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _convex_lane_handle(pkg, lib, p, cap):  # noqa: F811
    """A ConvexMpc handle whose plain and per-instance solves both take the lane kernel at any batch: QMPC_LANE_MIN=1,
    QMPC_LANE_CINST_MIN=1 (read by qmpc_create), the AUTO policy and the opt-in of the per-instance lane form"""
    saved = os.environ.pop("QMPC_LANE_CINST_MIN", None)
    os.environ["QMPC_LANE_CINST_MIN"] = "1"
    try:
        with _handle(pkg, lib, p, cap, QMPC_LANE_MIN=1) as s:
            s.set_instances_policy("auto")
            s.set_convex_lane_records(True)
            yield s
    finally:
        os.environ.pop("QMPC_LANE_CINST_MIN", None)
        if saved is not None:
            os.environ["QMPC_LANE_CINST_MIN"] = saved


def test_per_instance_paths_with_uniform_records(pkg, lib, oracle, fix):  # noqa: F811
    """Records that carry the handle's own values return the plain solve's bytes: qmpc_solve_instances on the wave kernel
    (default policy) and on the lane kernel (QMPC_INSTANCES_AUTO, QMPC_LANE_INST_MIN=64; the plain solve on the lane kernel too:
    QMPC_LANE_MIN=64), and qmpc_convex_solve_instances on the wave kernel and, with its opt-ins (AUTO,
    qmpc_set_convex_lane_records, QMPC_LANE_CINST_MIN=1, QMPC_LANE_MIN=1), on the lane kernel.
    Measured: bytes equal in all six; QuatMpc 4.5e-11 N (wave) and 1.4e-10 N (lane_handoff), ConvexMpc N=10 4.5e-11 / 1.2e-10 N and N=20
    1.7e-10 / 8.1e-10 N (wave / lane) from the oracle."""
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
    for name in ("convex_n10", "convex_n20"):
        rec = _records(pkg, name)
        p = _params(pkg, lib, name)
        with _handle(pkg, lib, p, n) as s:
            fam = s.kernel_for_convex_instances(n)
            assert fam == s.kernel_for_batch(n) == "wform_lds"
            fi, ii = s.convex_solve_instances(rec, pkg.instance_params(p, n))
            assert _last(pkg, s) == fam
            fp, ip = s.convex_solve(rec)
        assert _same(fi, fp) and _same(ii, ip)
        _converged_rules(pkg, oracle, fix, name, fi, ii, "convex_solve_instances, default policy", fam)
        with _convex_lane_handle(pkg, lib, p, n) as s:
            assert s.kernel_for_convex_instances(n) == s.kernel_for_batch(n) == "lane"
            fi, ii = s.convex_solve_instances(rec, pkg.instance_params(p, n))
            assert _last(pkg, s) == "lane"
            fp, ip = s.convex_solve(rec)
            assert _last(pkg, s) == "lane"
        assert _same(fi, fp) and _same(ii, ip)
        _converged_rules(pkg, oracle, fix, name, fi, ii, "convex_solve_instances, lane records", "lane")


@pytest.mark.parametrize("policy", ["wave", "auto"])
@pytest.mark.parametrize("model", ["quat", "convex"])
def test_random_variants_on_every_foothold_kind(pkg, lib, oracle, model, policy):  # noqa: F811
    """quat(10) / convex(10) with a robot of its own per instance (foothold_sets.variants / convex_variants: mass, inertia,
    friction, force bound, Q and R) on the wave kernel (default policy) and on the lane kernel (auto; QuatMpc
    QMPC_LANE_INST_MIN=64, ConvexMpc its opt-ins), against the oracle solved per instance with that instance's parameters, the
    way and under the tolerances of tests/test_gpu_instance_params.py::test_random_variants_against_the_oracle: every status
    word is the oracle's, and where that is 0 the forces are within 1e-6 N -- here on all 320 instances (the CPU suite holds the
    oracle to status 0 on every one).  Measured: QuatMpc 5.9e-11 N (wave kernel) and 1.0e-9 N (lane_handoff),
    ConvexMpc 4.2e-11 N (wave) and 5.4e-10 N (lane) from the oracle; every status 0 on both sides; iteration counts equal on 100 %."""
    name = model + "_n10"
    rec = _records(pkg, name)
    n = len(rec)
    p = _params(pkg, lib, name)
    if model == "quat":
        ip = F.variants(pkg, p)
        with _handle(pkg, lib, p, n, **({"QMPC_LANE_INST_MIN": 64} if policy == "auto" else {})) as s:
            s.set_instances_policy(policy)
            fam = s.kernel_for_instances(n)
            f, info = s.solve_instances(rec, ip)
            assert _last(pkg, s) == fam
    else:
        ip = F.convex_variants(pkg, p)
        with (_convex_lane_handle(pkg, lib, p, n) if policy == "auto" else _handle(pkg, lib, p, n)) as s:
            fam = s.kernel_for_convex_instances(n)
            f, info = s.convex_solve_instances(rec, ip)
            assert _last(pkg, s) == fam
    assert fam in (("lane", "lane_handoff") if policy == "auto" else ("wform_lds",)), fam
    if ("variants", model) not in _cache:
        solve = oracle.solve if model == "quat" else oracle.convex_solve
        _cache["variants", model] = [solve(pkg.params_with(p, ip[i]), rec[i:i + 1]) for i in range(n)]
    out = _cache["variants", model]
    fo = np.concatenate([o[0] for o in out])
    so = np.array([int(o[1]["status"][0]) for o in out])
    ito = np.array([int(o[1]["iterations"][0]) for o in out])
    d = np.abs(f - fo)
    print(f"foothold-sets | {'convex_' if model == 'convex' else ''}solve_instances, random variants, {policy} policy | {name} | family {fam} | "
          f"worst |f - f_oracle| {d.max():.2e} N, {_both(name, d)} | iteration counts equal on "
          f"{100 * (info['iterations'] == ito).mean():.2f} % | status counts {np.bincount(info['status'], minlength=6).tolist()} "
          f"(oracle {np.bincount(so, minlength=6).tolist()})")
    assert (so == 0).all()
    assert np.array_equal(info["status"], so)
    assert d.max() <= 1e-6


# ---- 9. device closed loop ----------------------------------------------------------------------------------------------------
def test_device_closed_loop_on_displaced_footholds(pkg, lib, oracle):  # noqa: F811
    """Eight standing robots (foothold_sets.loop_states) whose feet stand bunched, stretched, narrow, short, 0.10 m ahead and
    0.05 m aside of the default footholds, two on them; 40 ticks in stand mode at N = 10 with drop_ang_vel = 0.  The device loop against the same
    ticks built from the host classes, with the harness and bounds of
    tests/test_gpu_motion_sets.py::test_device_closed_loop_from_high_body_rates: contact flags exact, forces <= 1e-6 N at every
    tick, final states <= 1e-8; every robot holds status 0 over the 40 ticks; the persistent kernel and the per-tick form return
    the same bytes (a fresh child process per launch form: tests/_loop_foothold_worker.py).  The host classes launch the same
    kernel, so one independent check: the first tick's qmpc_input records are built in numpy from the initial states alone
    (foothold_sets.first_tick_inputs: foot_pos_body = R'(foot_pos_world - pos_world)) and solved by the oracle, and the first
    tick's traced forces are held to that within 1e-6 N -- the front kernel feeds the displaced feet: on every displaced robot
    they differ from the nominal robots' by more than 1e-3 N, a thousand times the bound of the comparison, so forces computed
    from the default footholds could not meet it (a robot at rest on a symmetric stance carries a quarter of its weight per
    leg whatever the width: the narrow robot's forces move by 0.13 N only, the one standing 0.10 m ahead by 14.6 N).  Measured: forces and states equal to the host classes' to the last bit (the host tick
    launches the same kernel for one robot); the first tick within 1.8e-14 N of the oracle on the records built in numpy; first-tick
    forces 0.59, 0.68, 0.13, 1.09, 14.6 and 9.4 N from a nominal robot's; every tick of every robot status 0 (10 - 11 iterations at
    the last); the two robots standing off-centre sink by 0.5 and 0.2 mm in 0.2 s; the two launch forms the same bytes."""
    import __graft_entry__ as g

    host = C.CDLL(str(g.build_host()))
    vp = C.c_void_p
    host.qh_loop_create_opts.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, vp, vp]; host.qh_loop_create_opts.restype = vp
    for fn in ("qh_loop_tick", "qh_loop_destroy", "qh_loop_device_status"):
        getattr(host, fn).argtypes = [vp]
    host.qh_loop_export.argtypes = [vp, vp]
    T, N = 40, 10
    lp = pkg.default_loop_params(lib)
    st_init = F.loop_states(pkg, lib, lp)
    B = len(st_init)
    displaced = np.array([k is not None for k in F.LOOP_KINDS])
    assert (st_init["foot_pos_world"].reshape(B, 4, 3)[..., 2] == 0.0).all()           # all feet on the ground
    s = pkg.Solver(M.params(pkg, "default_params", N, pkg.MODE_CONVERGED, lib), B, device=0, lib=lib)      # drop_ang_vel = 0, as the host classes below
    st, tf, tc = s.loop_run(st_init, T, lp, trace=True)
    s.close()
    assert (st["tick"] == T).all() and (st["status"] == 0).all(), st["status"]
    worst_f = worst_x = 0.0
    for i in range(B):
        h = host.qh_loop_create_opts(str(pkg.LIB_PATH).encode(), N, pkg.MODE_CONVERGED, 0, C.addressof(lp), st_init[i:i + 1].ctypes.data)
        assert h and host.qh_loop_device_status(h) == 0
        e = np.zeros(1, dtype=pkg.LOOP_STATE_DTYPE)
        for t in range(T):
            assert host.qh_loop_tick(h) == 1, (i, t)
            host.qh_loop_export(h, e.ctypes.data)
            assert e[0]["status"] == 0, (i, t, F.LOOP_KINDS[i])                          # every tick of every robot converges
            assert np.array_equal(e[0]["contacts"], tc[t, i]), (i, t, e[0]["contacts"], tc[t, i])     # exact
            worst_f = max(worst_f, float(np.abs(e[0]["forces_body"] - tf[t, i]).max()))
        host.qh_loop_destroy(h)
        d, r = st[i], e[0]
        for k in ("pos_world", "quat", "lin_vel_world", "ang_vel_body", "foot_pos_world", "pos_d_world", "quat_d", "grf_world",
                  "foot_target_world"):
            worst_x = max(worst_x, float(np.abs(d[k] - r[k]).max()))
    # the independent check of the first tick
    rec0 = F.first_tick_inputs(pkg, st_init)
    fo, io = oracle.solve(oracle.default_params(N, 0), rec0, threads=4)
    d0 = np.abs(tf[0] - fo).max(axis=1)
    nominal = np.where(~displaced)[0]
    fed = np.abs(tf[0] - tf[0, nominal[0]]).max(axis=1)
    sha = hashlib.sha256(st.tobytes() + tf.tobytes() + tc.tobytes()).hexdigest()
    print(f"foothold-sets | device closed loop, {B} robots x {T} ticks in stand mode | worst force difference to the host classes "
          f"{worst_f:.2e} N, worst state difference {worst_x:.2e} | first tick against the oracle on records built from the states "
          f"[N] " + ", ".join(f"{k or 'nominal'}: {v:.1e}" for k, v in zip(F.LOOP_KINDS, d0)) +
          f" | first tick's forces against a nominal robot's [N] {fed.round(2).tolist()}"
          f" | height after {T} ticks [m] {st['pos_world'][:, 2].round(4).tolist()}"
          f" | iterations of the last tick {st['iterations'].astype(int).tolist()}")
    assert worst_f <= 1e-6 and worst_x <= 1e-8
    assert (io["status"] == 0).all() and d0.max() <= 1e-6, d0
    assert (fed[displaced] > 1e-3).all() and (fed[~displaced] <= 1e-6).all(), fed
    worker = Path(__file__).resolve().parent / "_loop_foothold_worker.py"
    sums = {}
    for fused in ("0", "1"):
        r = subprocess.run([sys.executable, str(worker), str(T), str(N)], env=dict(os.environ, QMPC_LOOP_FUSED=fused),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        sums[fused] = [l for l in r.stdout.splitlines() if l.startswith("SHA")][0].split()[1]
    print(f"foothold-sets | device closed loop | per-tick form and persistent kernel: the same bytes {sums['0'] == sums['1']}")
    assert sums["0"] == sums["1"] and sha in sums.values()
