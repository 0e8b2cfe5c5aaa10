"""GPU suite (-m gpu): every solve kernel on every stance set and on both signs of the two quaternions (tests/stance_sets.py).

Every solve kernel branches on the stance mask of its instance -- the lane kernel's counting sort and wave-uniform point order,
the wave kernels' per-leg predicates, constraint bit field and warm-start shift, the hand-off's records -- and the state
generators draw three masks (all legs and the two trot diagonals; both feet, left, right) and quaternions with w > 0.  The
records here carry all 15 sets of four legs (16 of the 8-point model) and all four sign combinations; the CPU suite
(tests/test_stance_sets_cpu.py) certifies the oracle on the same records and keeps them inside the solver's envelope.

Rules, unless a test says otherwise (the project's own for the converged mode): status words equal to the oracle's and all 0;
forces within 1e-6 N (8-point model: corner forces 1e-5, foot wrench 1e-7); swing forces exactly 0; iteration counts equal on
>= 97 %; first-knot forces within 1e-6 (1e-5) of the stored certified points (tests/golden/stance_fixtures.npz).  No instance is
left out of a comparison.  Every test reads back the kernel family that ran.  Each prints a line `stance-sets | ...` with the
family, the worst force difference and the share of equal iteration counts (profiles/r15_stance_sets.txt is made of them)."""
import contextlib
import os
from pathlib import Path

import numpy as np
import pytest

import stance_sets as S

pytestmark = pytest.mark.gpu

KNOBS = ("QMPC_VARIANT", "QMPC_WFORM", "QMPC_LANE_MIN", "QMPC_LANE_INST_MIN", "QMPC_LANE_CAP", "QMPC_HANDOFF_RESTART",
         "QMPC_LANE_PAIR", "QMPC_LANE_SORT", "QMPC_LANE_REF_MIN")
# name: (records, default params, Solver call, oracle call, horizon, force components, model name of the planner's table)
SETS = {
    "quat_n5": (lambda pkg: S.quat(pkg, 5), "default_params", "solve", "solve", 5, 12, "quat"),
    "quat_n10": (lambda pkg: S.quat(pkg, 10), "default_params", "solve", "solve", 10, 12, "quat"),
    "quat_n20": (lambda pkg: S.quat(pkg, 20), "default_params", "solve", "solve", 20, 12, "quat"),
    "convex_n10": (S.convex, "default_convex_params", "convex_solve", "convex_solve", 10, 12, "convex"),
    "convex_n20": (S.convex, "default_convex_params", "convex_solve", "convex_solve", 20, 12, "convex"),
    "biped8_n16": (S.biped8, "default_biped8_params", "solve8", "solve8", 16, 24, "quat8"),
}
_cache = {}


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()   # raises if the HIP extension is missing: no fallback


@pytest.fixture(scope="module")
def fix():
    return np.load(Path(__file__).parent / "golden" / "stance_fixtures.npz")


@contextlib.contextmanager
def _handle(pkg, lib, p, cap, **knobs):
    """A handle created under exactly these tuning knobs (qmpc_create reads them; none of them is read later)"""
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update({k: str(v) for k, v in knobs.items()})
    try:
        s = pkg.Solver(p, cap, device=0, lib=lib)
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in saved.items() if v is not None})
    try:
        yield s
    finally:
        s.close()


def _last(pkg, s):
    return pkg.KERNEL_FAMILY[s.query(pkg.QUERY_LAST_KERNEL)]


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _params(pkg, lib, name, mode=None):
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


def _run(pkg, lib, name, cap=None, rec=None, mode=None, family=None, **knobs):
    """One solve of the set (or of `rec`) on a fresh handle; asserts the family that ran.  (forces, info)"""
    rec = _records(pkg, name) if rec is None else rec
    with _handle(pkg, lib, _params(pkg, lib, name, mode), cap or len(rec), **knobs) as s:
        planned = s.kernel_for_batch(len(rec))
        f, info = getattr(s, SETS[name][2])(rec)
        ran = _last(pkg, s)
    assert ran == planned and (family is None or ran == family), (name, knobs, planned, ran, family)
    return f, info


def _wrench8(rec, f):
    B = len(rec)
    feet, f = rec["foot_pos_body"].reshape(B, 8, 3), f.reshape(B, 8, 3)
    return np.concatenate([f.sum(1), np.cross(feet, f).sum(1)], axis=1)


def _converged_rules(pkg, oracle, fix, name, f, info, tag, family):
    """The converged mode's rules of this module on the unique records of a set; prints the record line"""
    rec = _records(pkg, name)
    nu = SETS[name][5]
    fo, io = _oracle(pkg, oracle, name)
    d = float(np.abs(f - fo).max())
    share = float((info["iterations"] == io["iterations"]).mean())
    dw = float(np.abs(_wrench8(rec, f) - _wrench8(rec, fo)).max()) if nu == 24 else None
    key = name if name + "_U" in fix.files else None
    dc = float(np.abs(f[:len(fix[key + "_U"])] - fix[key + "_U"][:, 0, :]).max()) if key else None
    print(f"stance-sets | {tag} | {name} | family {family} | worst |f - f_oracle| {d:.2e} N"
          + (f" (foot wrench {dw:.2e})" if dw is not None else "") + f" | iteration counts equal on {100 * share:.2f} %"
          + (f" | certified points within {dc:.2e} N" if dc is not None else "")
          + f" | status counts {np.bincount(info['status'], minlength=6).tolist()}")
    assert np.array_equal(info["status"], io["status"]) and (info["status"] == 0).all(), tag
    assert d < (1e-5 if nu == 24 else 1e-6), (tag, d)
    if nu == 24:
        assert dw < 1e-7, (tag, dw)
    assert np.abs(f[S.swing_rows(rec, nu // 3)]).max() == 0.0, tag
    assert share >= 0.97, (tag, share)
    if key:
        assert dc < (1e-5 if nu == 24 else 1e-6), (tag, dc)


def _sign_flips_return_the_same_bits(pkg, lib, oracle, tag, cap=None, **knobs):
    """quat(10) with w > 0 on both quaternions against its three sign flips on one handle: q and -q are one attitude and the
    arithmetic is sign-symmetric (the cost takes |q_ref' q|; `rot` is given), so forces, status and iteration words are the same
    bits.  All four runs are held to the oracle (which is itself bit-identical under the flips: tests/test_stance_sets_cpu.py):
    quat(10) itself negates quat_d on five of the 15 sets only, these runs put all four sign combinations on every set."""
    base = S.quat(pkg, 10, flipped=False)
    if "oracle_unflipped" not in _cache:
        _cache["oracle_unflipped"] = oracle.solve(oracle.default_params(10, 0), base, threads=8)
    fo, io = _cache["oracle_unflipped"]
    with _handle(pkg, lib, _params(pkg, lib, "quat_n10"), cap or len(base), **knobs) as s:
        f, info = s.solve(base)
        out = [(kw, s.solve(S.flip(base, **kw))) for kw in ({"quat": True}, {"quat_d": True}, {"quat": True, "quat_d": True})]
    worst = max(float(np.abs(g - f).max()) for _, (g, _) in out)
    same = all(_same(g, f) and np.array_equal(gi["status"], info["status"]) and np.array_equal(gi["iterations"], info["iterations"])
               for _, (g, gi) in out)
    print(f"stance-sets | {tag} | sign flips of quat / quat_d / both: bit-identical {same} (largest difference {worst:.2e} N)")
    for kw, (g, gi) in [({}, (f, info))] + out:
        assert np.array_equal(gi["status"], io["status"]) and (gi["status"] == 0).all(), (tag, kw)
        assert np.abs(g - fo).max() < 1e-6, (tag, kw)
        assert (gi["iterations"] == io["iterations"]).mean() >= 0.97, (tag, kw)
    assert same, (tag, worst)


def _wave_lds(pkg, lib, name):
    """The set on the all-LDS wave kernel (default planner, the set's own size): what the workspace forms are compared with"""
    if ("lds", name) not in _cache:
        _cache["lds", name] = _run(pkg, lib, name, family="wform_lds")
    return _cache["lds", name]


def _lane(pkg, lib, name="quat_n10"):
    if ("lane", name) not in _cache:
        _cache["lane", name] = _run(pkg, lib, name, family="lane", QMPC_VARIANT=4)
    return _cache["lane", name]


# ---- 1. wave kernels, everything in LDS ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SETS))
def test_wave_kernels_in_lds(pkg, lib, oracle, fix, name):
    """Default planner at the set's own size (480 / 288 / 256 instances): the wrench-form kernel with everything in LDS.
    Measured, worst force difference to the oracle (share of equal iteration counts where not 100 %): QuatMpc N=5 1.8e-11, N=10 3.5e-11,
    N=20 9.1e-11 N (98.96 %); ConvexMpc N=10 6.4e-12, N=20 1.5e-10 N (99.38 %); 8-point corner forces 1.1e-10, foot wrench 2.2e-10;
    the sign flips return the same bits."""
    f, info = _wave_lds(pkg, lib, name)
    _converged_rules(pkg, oracle, fix, name, f, info, "wave, all LDS", "wform_lds")
    if name == "quat_n10":
        _sign_flips_return_the_same_bits(pkg, lib, oracle, "wave, all LDS")


# ---- 2. wave kernels, workspace forms -----------------------------------------------------------------------------------------
def _first_batch_beyond(s, family, hi):
    """smallest batch for which the handle no longer plans `family` (the planner's choice is monotone in the batch)"""
    lo = 1
    assert s.kernel_for_batch(lo) == family and s.kernel_for_batch(hi) != family
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if s.kernel_for_batch(mid) == family else (lo, mid)
    return hi


@pytest.mark.parametrize("name", list(SETS))
def test_wave_kernels_workspace_forms(pkg, lib, oracle, fix, name):
    """The set tiled to just beyond the batch at which the planner leaves the all-LDS form (asked of the handle), and -- where
    the planner's table (tests/golden/kernel_plans.txt.gz) has a second workspace form for the horizon: the slack arrays out as
    well -- to just beyond that batch too (the family query does not tell the two apart): QuatMpc N=10 / 5 take the gains-in-
    workspace form, QuatMpc N=20, ConvexMpc N=20 and the 8-point model both.  Against the all-LDS form on the unique records:
    forces within 1e-7 N (8-point 1e-5) and identical iteration counts (the forms differ in where their arrays live); every copy
    returns the first one's bits; and the oracle's rules.
    Measured: every workspace form returns the all-LDS form's BITS on every set (0.0 N), so the figures of test_wave_kernels_in_lds."""
    rec, (model, N, nu) = _records(pkg, name), (SETS[name][6], SETS[name][4], SETS[name][5])
    n = len(rec)
    fl, il = _wave_lds(pkg, lib, name)
    with _handle(pkg, lib, _params(pkg, lib, name), 4096) as s:
        b1 = _first_batch_beyond(s, "wform_lds", 4096)
        assert b1 > n and s.kernel_for_batch(b1) == "wform_ws"
        steps = [(b1, 5, None)]
        if N != 5:          # (the table enumerates N = 4, 10, ...: the N = 5 handle is asked alone)
            plan = S.plain_plan(model, N)
            ws = [(b, var, plan[i + 1][0] if i + 1 < len(plan) else None) for i, (b, fam, var) in enumerate(plan) if fam == 2]
            assert ws[0][0] == b1 and [v for _, v, _ in ws] == ([5] if N == 10 else [5, 6]), (ws, b1)
            steps = ws
        for b, var, end in steps:
            t = S.tiled(rec, b)
            assert end is None or len(t) < end, (name, b, len(t), end)
            assert s.kernel_for_batch(len(t)) == "wform_ws"
            f, info = getattr(s, SETS[name][2])(t)
            assert _last(pkg, s) == "wform_ws"
            tag = f"wave, workspace form {var} at {len(t)}"
            assert S.copies_identical(f, n) and S.copies_identical(info["status"], n) and S.copies_identical(info["iterations"], n), tag
            d = float(np.abs(f[:n] - fl).max())
            print(f"stance-sets | {tag} | {name} | against the all-LDS form: {d:.2e} N, iteration counts equal "
                  f"{np.array_equal(info['iterations'][:n], il['iterations'])}")
            assert d < (1e-5 if nu == 24 else 1e-7), (tag, d)
            assert np.array_equal(info["iterations"][:n], il["iterations"]), tag
            _converged_rules(pkg, oracle, fix, name, f[:n], info[:n], tag, "wform_ws")


# ---- 3. round-1 family --------------------------------------------------------------------------------------------------------
def test_round_1_family(pkg, lib, oracle, fix):
    """QMPC_WFORM=0: the dense kernels, everything in LDS at 480 instances and, tiled beyond the batch the handle names, with
    the gains in the workspace.  Measured: 1.4e-11 N (all LDS) and 9.3e-12 N (workspace form) from the oracle, iteration counts
    equal on 100 %, the two forms within 1e-11 N of each other, the sign flips bit-identical."""
    name = "quat_n10"
    rec = _records(pkg, name)
    n = len(rec)
    with _handle(pkg, lib, _params(pkg, lib, name), 4096, QMPC_WFORM=0) as s:
        assert s.kernel_for_batch(n) == "dense_lds"
        f, info = s.solve(rec)
        assert _last(pkg, s) == "dense_lds"
        _converged_rules(pkg, oracle, fix, name, f, info, "round-1 family, all LDS", "dense_lds")
        t = S.tiled(rec, _first_batch_beyond(s, "dense_lds", 4096))
        assert s.kernel_for_batch(len(t)) == "dense_ws"
        ft, it_ = s.solve(t)
        assert _last(pkg, s) == "dense_ws"
    assert S.copies_identical(ft, n) and S.copies_identical(it_["status"], n) and S.copies_identical(it_["iterations"], n)
    _converged_rules(pkg, oracle, fix, name, ft[:n], it_[:n], f"round-1 family, workspace form at {len(t)}", "dense_ws")
    assert np.abs(ft[:n] - f).max() < 1e-7 and np.array_equal(it_["iterations"][:n], info["iterations"])
    _sign_flips_return_the_same_bits(pkg, lib, oracle, "round-1 family, all LDS", QMPC_WFORM=0)


# ---- 4. reference mode on the wave kernels ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,knobs,family", [("quat_n10", {}, "wform_lds"), ("convex_n10", {}, "wform_lds"),
                                               ("biped8_n16", {}, "wform_lds"), ("quat_n10", {"QMPC_WFORM": 0}, "dense_lds")])
def test_reference_mode_on_the_wave_kernels(pkg, lib, oracle, name, knobs, family):
    """MODE_REFERENCE (truncated AL-iLQR iterates) under the rule of test_reference_mode_on_device_matches_oracle_reference_mode:
    >= 99 % of the instances agree with the oracle to 1e-6 N with identical status and iteration words; swing forces exactly 0.
    (N = 20 is left out: qmpc_plan.h documents the wrench-form reference kernels' accuracy there.)
    Measured: QuatMpc 478 of 480 identical (the other two up to 1.4e-2 N; status counts 189 OK / 273 MAX_ITER / 18 NOT_PD), with
    QMPC_WFORM=0 480 of 480 (worst 1.2e-9 N); ConvexMpc 480 of 480 (4.2e-11); 8-point 256 of 256 (3.0e-10)."""
    rec = _records(pkg, name)
    f, info = _run(pkg, lib, name, mode=pkg.MODE_REFERENCE, family=family, **knobs)
    fo, io = _oracle(pkg, oracle, name, 1)
    d = np.abs(f - fo).max(axis=1)
    same = (d < 1e-6) & (info["status"] == io["status"]) & (info["iterations"] == io["iterations"])
    print(f"stance-sets | reference mode, wave kernels {knobs or ''} | {name} | family {family} | {int(same.sum())}/{len(rec)} identical "
          f"(1e-6 N, status, iterations) | worst {d.max():.2e} N | status counts {np.bincount(info['status'], minlength=6).tolist()}")
    assert same.mean() >= 0.99
    assert np.abs(f[S.swing_rows(rec, SETS[name][5] // 3)]).max() == 0.0 and np.isfinite(f).all()


# ---- 5. lane kernel -----------------------------------------------------------------------------------------------------------
LANE_HANDLES = {"pairs, sorted": {}, "plain, sorted": {"QMPC_LANE_PAIR": 0}, "pairs, unsorted": {"QMPC_LANE_SORT": 0},
                "plain, unsorted": {"QMPC_LANE_PAIR": 0, "QMPC_LANE_SORT": 0}}


def _lane_handles(pkg, lib):
    """quat(10) on the four handles of QMPC_VARIANT=4: lane pairs on the sorted batch (default), QMPC_LANE_PAIR=0, QMPC_LANE_SORT=0, both"""
    if "lane4" not in _cache:
        _cache["lane4"] = {tag: (_lane(pkg, lib) if not knobs else _run(pkg, lib, "quat_n10", family="lane", QMPC_VARIANT=4, **knobs))
                           for tag, knobs in LANE_HANDLES.items()}
    return _cache["lane4"]


def _bits_differ(a, b):
    """(instances whose forces differ, largest difference, status words equal, iteration words equal) of two (forces, info)"""
    d = np.abs(a[0] - b[0]).max(axis=1)
    return int((d > 0).sum()), float(d.max()), np.array_equal(a[1]["status"], b[1]["status"]), np.array_equal(a[1]["iterations"], b[1]["iterations"])


def test_lane_kernel_on_every_stance_set(pkg, lib, oracle, fix):
    """QMPC_VARIANT=4 on quat(10), four handles: lane pairs or the plain form with half the lanes masked, on the batch sorted by
    stance set or in its own order.  Sorted, a wavefront holds one stance set (two at a boundary) and the wave-uniform point
    order runs over 1, 2, 3 or 4 points; unsorted, every wavefront holds all 15 sets, and the union of its live lanes' sets
    shrinks as instances finish.  Each handle against the oracle; the order of the batch does not change a bit of either form
    (the permutation check of test_lane_kernel_equals_wave_kernel_on_the_same_batch); the sign flips return the same bits.

    This test found the pair form's apply pass undoing its own step on wavefronts with an ODD number of stance points (every
    one- and three-leg set ran to the iteration limit, 256 of 480 instances, forces up to 126 N off; qmpc_lane_core.h, pass_A).
    Measured after the fix: worst 1.1e-9 N, iteration counts equal on 100 %."""
    runs = _lane_handles(pkg, lib)
    for tag, (f, info) in runs.items():
        _converged_rules(pkg, oracle, fix, "quat_n10", f, info, f"lane kernel ({tag})", "lane")
    for form in ("pairs", "plain"):
        n, d, st, it_ = _bits_differ(runs[form + ", sorted"], runs[form + ", unsorted"])
        print(f"stance-sets | lane kernel ({form}) | sorted against unsorted batch: {n} instances differ, largest difference {d:.2e} N")
        assert n == 0 and st and it_, (form, n, d)
    _sign_flips_return_the_same_bits(pkg, lib, oracle, "lane kernel (pairs, sorted)", QMPC_VARIANT=4)
    _sign_flips_return_the_same_bits(pkg, lib, oracle, "lane kernel (plain, unsorted)", QMPC_VARIANT=4, QMPC_LANE_PAIR=0, QMPC_LANE_SORT=0)


def test_lane_pairs_return_the_plain_forms_bits_on_every_stance_set(pkg, lib):
    """The contract of tests/test_gpu_lane.py::test_lane_pairs_return_the_plain_forms_bits on quat(10): the four handles return
    identical forces, status and iteration words.

    This test found the second fault of the pair forms.  After the pass_A fix the status and iteration words were identical and
    the forces bit-identical on the eleven sets with two or more stance legs, but on 0001 / 0010 / 0100 / 1000 the pair form
    differed from the plain form on 27 / 21 / 23 / 26 of 32 instances by up to 9.5e-10 / 3.9e-10 / 1.1e-10 / 1.3e-10 N.  Splitting
    one pass at a time placed it in the pair form of the backward pass; the operation was initial_rows' `cr uz - fz_max`, which
    the compiler fused in one instantiation and not in the other.  The row's residual is exactly 0 whenever the reference input
    is at least 1 N inside the force limit; with one stance leg it carries the whole weight, above fz_max.  Now fused explicitly.
    Measured since: 0 instances differ on every handle."""
    runs = _lane_handles(pkg, lib)
    base = runs["pairs, sorted"]
    worst = {}
    for tag in list(LANE_HANDLES)[1:]:
        worst[tag] = _bits_differ(runs[tag], base)
        n, d, st, it_ = worst[tag]
        print(f"stance-sets | lane kernel ({tag}) | against the default handle (pairs, sorted): {n} instances differ, largest difference "
              f"{d:.2e} N, status words equal {st}, iteration words equal {it_}")
    for tag, (n, d, st, it_) in worst.items():
        assert st and it_, tag
    for tag, (n, d, st, it_) in worst.items():
        assert n == 0, (tag, n, d)


@pytest.mark.parametrize("name", [n for n in SETS if n != "quat_n10"])
def test_lane_kernel_other_sets(pkg, lib, oracle, fix, name):
    """The other sets on the default handle of QMPC_VARIANT=4.  Measured: QuatMpc N=5 4.5e-10 N, N=20 1.6e-9 N (iteration counts equal
    on 97.22 %: 280 of 288); ConvexMpc 4.3e-11 / 9.2e-11; 8-point 5.2e-11 (foot wrench 1.1e-10).  Before the fix of pass_A: N=5
    256 and N=20 128 instances at the iteration limit."""
    f, info = _lane(pkg, lib, name)
    _converged_rules(pkg, oracle, fix, name, f, info, "lane kernel (pairs, sorted)", "lane")


# ---- 6. lane kernel, full wavefronts ------------------------------------------------------------------------------------------
def test_lane_kernel_full_wavefronts(pkg, lib, oracle, fix):
    """The plain 64-lane form launches only when twice the batch exceeds the resident lanes (a handle of 70000, more than 32768
    instances): quat(10) tiled to 33120.  Every copy returns the first one's bits; the unique records follow the oracle and
    return the bits of the 480-instance launch with QMPC_LANE_PAIR=0 (the same form, half its lanes masked) -- and, the issue's
    rule, of the default 480-instance launch (lane pairs).
    Measured: 0 instances differ from either (before the fix of initial_rows: 97 of 480, the one-leg sets, by up to 9.5e-10 N from
    the lane pairs); 1.2e-9 N from the oracle."""
    rec = _records(pkg, "quat_n10")
    n = len(rec)
    runs = _lane_handles(pkg, lib)
    t = S.tiled(rec, 32769)
    f, info = _run(pkg, lib, "quat_n10", cap=70000, rec=t, family="lane", QMPC_VARIANT=4)
    assert S.copies_identical(f, n) and S.copies_identical(info["status"], n) and S.copies_identical(info["iterations"], n)
    _converged_rules(pkg, oracle, fix, "quat_n10", f[:n], info[:n], f"lane kernel, full wavefronts at {len(t)}", "lane")
    first = (f[:n], info[:n])
    for tag in ("plain, sorted", "pairs, sorted"):
        k, d, st, it_ = _bits_differ(first, runs[tag])
        print(f"stance-sets | lane kernel, full wavefronts at {len(t)} | against the 480-instance launch ({tag}): {k} instances differ, "
              f"largest difference {d:.2e} N, status words equal {st}, iteration words equal {it_}")
        assert st and it_, tag
        assert k == 0, (tag, k, d)


# ---- 7. lane kernel, reference mode -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["quat_n10", "quat_n20", "convex_n10", "biped8_n16"])
def test_lane_kernel_reference_mode(pkg, lib, oracle, name):
    """The rule of tests/test_gpu_lane.py::test_lane_kernel_reference_mode: status and iteration words identical to the oracle's
    on every instance, forces within 1e-6 N on >= 95 % (truncated iterates); swing forces exactly 0.
    Measured: within 1e-6 N on 100 % everywhere; worst 2.2e-10 (QuatMpc N=10), 3.0e-10 (N=20), 4.3e-11 (ConvexMpc), 3.0e-10 N (8-point)."""
    rec = _records(pkg, name)
    f, info = _run(pkg, lib, name, mode=pkg.MODE_REFERENCE, family="lane", QMPC_VARIANT=4)
    fo, io = _oracle(pkg, oracle, name, 1)
    d = np.abs(f - fo).max(axis=1)
    print(f"stance-sets | reference mode, lane kernel | {name} | family lane | within 1e-6 N on {100 * (d < 1e-6).mean():.2f} % | worst {d.max():.2e} N "
          f"| status counts {np.bincount(info['status'], minlength=6).tolist()}")
    assert np.array_equal(info["status"], io["status"]) and np.array_equal(info["iterations"], io["iterations"])
    assert (d < 1e-6).mean() >= 0.95
    assert np.abs(f[S.swing_rows(rec, SETS[name][5] // 3)]).max() == 0.0 and np.isfinite(f).all()


# ---- 8. warm start ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knobs,family", [({}, "wform_lds"), ({"QMPC_VARIANT": 4}, "lane")], ids=["wave", "lane"])
def test_warm_start_between_every_pair_of_stance_sets(pkg, lib, oracle, knobs, family):
    """qmpc_solve_warm at N=10 with the closed loop's low initial barrier (ipm_mu0 = 1e-6): a cold call on one stance set, then
    the next tick from its trajectory on another -- every ordered pair of the 15 sets twice, so the warm start's per-leg shift
    meets every leg landing, lifting off, staying down and staying up.  The rules of test_lane_kernel_warm_start_matches_oracle
    against oracle.solve_warm: status equal and all 0, forces within 1e-6 N, iteration counts equal on >= 90 % and within one on
    >= 95 %; swing forces of the new set exactly 0.
    Measured: wave kernel cold 3.9e-11, warm 5.0e-11 N, iteration counts equal on 100 %; lane kernel cold 8.0e-10, warm 5.1e-10 N,
    equal on 99.33 %, within one on 99.78 %."""
    first, second = S.warm_pairs(pkg)
    B, N = len(first), 10
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    p.ipm_mu0 = 1e-6
    # (qmpc_solve_warm does not record its launch for QUERY_LAST_KERNEL: the family is the planner's for a warm-started call of
    # this size under these knobs -- its table -- which shares the plain solve's choice, asked of the handle)
    table = S.plain_plan("quat", N, knobs="QMPC_VARIANT=4" if knobs else "default", kind="warm")
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
    print(f"stance-sets | warm start | family {family} | cold {np.abs(f0 - fo0).max():.2e} N, warm {np.abs(f1 - fo1).max():.2e} N | "
          f"iteration counts equal on {100 * (di == 0).mean():.2f} %, within one on {100 * (di <= 1).mean():.2f} % | "
          f"warm iterations {i1['iterations'].mean():.2f} (cold {i0['iterations'].mean():.2f})")
    assert np.array_equal(i0["status"], io0["status"]) and (i0["status"] == 0).all() and np.abs(f0 - fo0).max() < 1e-6
    assert np.array_equal(i1["status"], io1["status"]) and (i1["status"] == 0).all()
    assert np.abs(f1 - fo1).max() < 1e-6
    assert (di == 0).mean() >= 0.9 and (di <= 1).mean() >= 0.95, np.bincount(di)
    assert np.abs(f1[S.swing_rows(second)]).max() == 0.0
    assert np.abs(tu1.reshape(B, N, 12)[np.repeat(S.swing_rows(second)[:, None, :], N, axis=1)]).max() == 0.0
    assert np.abs(tu1.reshape(B, -1) - tuo1.reshape(B, -1)).max() < 1e-5


# ---- 9. hand-off --------------------------------------------------------------------------------------------------------------
def test_straggler_hand_off(pkg, lib, oracle, fix):
    """QMPC_LANE_MIN=64, QMPC_LANE_CAP=12 on quat(10): the lane kernel stops at 12 iterations and the wave kernel continues what
    is left from the hand-off's records (`resume`) -- on these sets most of the batch.  Against the same handle with
    QMPC_LANE_CAP=0 (the pure lane kernel): status equal, forces within 1e-7 N (the rule of
    test_straggler_hand_off_of_large_batches), iteration counts equal on >= 97 % (that test's 99.9 % presumes 32768 instances: at
    480 it would forbid a single threshold case); a second call returns the same bits; the same with QMPC_HANDOFF_RESTART=1.
    Measured: 87.9 % of the batch beyond the cap; 1.2e-10 N from the oracle, 1.1e-9 N from the pure lane kernel, iteration counts
    equal on 100 %, with and without the restart.  (Before the fix of pass_A the hand-off returned status 0 with forces 27 N off.)"""
    name = "quat_n10"
    rec = _records(pkg, name)
    fo, io = _oracle(pkg, oracle, name)
    handed = float((io["iterations"] > 12).mean())
    assert handed >= 0.1, handed
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
        print(f"stance-sets | {tag} | {100 * handed:.1f} % of the batch beyond the cap | against the pure lane kernel: {d:.2e} N, "
              f"iteration counts equal on {100 * share:.2f} %")
        assert np.array_equal(info["status"], ip["status"]) and d < 1e-7 and share >= 0.97, (tag, d, share)


# ---- 10. per-instance parameter paths, uniform records ------------------------------------------------------------------------
def test_per_instance_paths_with_uniform_records(pkg, lib, oracle, fix):
    """Records that carry the handle's own values return the plain solve's bytes (test_uniform_records_equal_the_plain_solve of
    the three per-instance modules): qmpc_solve_instances on the wave kernel (default policy) and on the lane kernel
    (QMPC_INSTANCES_AUTO, QMPC_LANE_INST_MIN=64; the plain solve on the lane kernel too: QMPC_LANE_MIN=64), and
    qmpc_convex_solve_instances at N=20.  Measured: bytes equal in all three; 3.5e-11 N (wave), 1.8e-10 N (lane_handoff) and 1.5e-10 N
    (ConvexMpc) from the oracle."""
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
    rec = _records(pkg, "convex_n20")
    p = _params(pkg, lib, "convex_n20")
    with _handle(pkg, lib, p, n) as s:
        fam = s.kernel_for_convex_instances(n)
        assert fam == s.kernel_for_batch(n) == "wform_lds"
        fi, ii = s.convex_solve_instances(rec, pkg.instance_params(p, n))
        assert _last(pkg, s) == fam
        fp, ip = s.convex_solve(rec)
    assert _same(fi, fp) and _same(ii, ip)
    _converged_rules(pkg, oracle, fix, "convex_n20", fi, ii, "convex_solve_instances", fam)
