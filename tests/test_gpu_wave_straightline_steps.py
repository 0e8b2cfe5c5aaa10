"""GPU suite (-m gpu): the step-length ratio tests of the one-wave kernels, written without short-circuit evaluation, and
the weakly-active flags that follow them.

recover_directions_w keeps the smallest s / (-ds) and lam / (-dlam) of a lane's six rows as fractions: `(dsv < 0) & ((pd == 0)
| (sv pd < pn (-dsv)))`, with `&` / `|` on the comparisons' values so that the six rows of a contact point are straight-line
code (qmpc_wform.h; tools/isa_regions.py counts the regions).  The truth table is that of `&&` / `||`, so nothing that is
computed may move; apply_w then takes the step and sets the weakly-active (Tapia) flag of every row from it.  The cases
are the ones in which the expressions take every side:
  QuatMpc, N = 1, 10, 11       4 N crosses 64 lanes at N = 11 (a second trip of the lane loops); N = 10 is bench.py's kernel
  ConvexMpc, N = 1, 10
  8-point model, N = 1, 8      the LEAN path of apply_w (directions recomputed from dU, flags in a bit field)
    -- 64 records each, record k on stance set k mod 15 of MASKS4 (k mod 16 of MASKS8) of tests/stance_sets.py, the module
       that holds the stance sets (tests/instance_lane_sets.py holds none): swing legs take the `stance == false` selects
  QuatMpc N = 10, far          the 64 records of tests/foothold_sets.py with all feet 0.30 m ahead or 0.25 m aside of nominal
                               (eight of each of the four reference classes): steps are shortened in most iterations, so
                               the ratio tests replace their fraction often.  The CPU oracle takes 21.0 iterations on them
                               on average (at most 36) against 13.6 on the same records as the generator draws them, more
                               on 56 of the 64 and as many on three; the test holds that too
  QuatMpc N = 10, warm         a cold solve on one stance set, then a warm-started one (ipm_mu0 = 1e-6) on another: records
                               7 k mod 450 of stance_sets.warm_pairs (all 15 sets on either tick), 47 of 64 with a leg
                               that has just landed.  A landed leg starts from the initial slack with a direction of
                               exactly 0 on a row: `pd == 0`

Rules, those of the neighbouring wave tests (tests/test_gpu_wave_batched_loads.py, tests/test_gpu_stance_sets.py): status
words equal to the oracle's and all 0; forces within 1e-6 N (8-point model: corner forces 1e-5, foot wrench 1e-7); swing
forces exactly 0 -- and here the iteration words equal to the oracle's on EVERY record.  Then the same records tiled to just
beyond the all-LDS form's last batch (asked of the handle): the workspace form's forces, status and iteration words are the
all-LDS form's BYTES.  No case is left out."""
import numpy as np
import pytest

import foothold_sets as F
import stance_sets as S
from test_gpu_stance_sets import _first_batch_beyond, _handle, _last, _same, _wrench8

pytestmark = pytest.mark.gpu

# model: (records, config, default params, Solver call / oracle call, stance sets, contact points)
MODELS = {
    "quat": ("random_go1_trot_states", 2, "default_params", "solve", S.MASKS4, 4),
    "convex": ("random_go1_convex_states", 12, "default_convex_params", "convex_solve", S.MASKS4, 4),
    "biped8": ("random_biped8_states", 5, "default_biped8_params", "solve8", S.MASKS8, 8),
}
CASES = [("quat", 1), ("quat", 10), ("quat", 11), ("convex", 1), ("convex", 10), ("biped8", 1), ("biped8", 8)]
CAP = 16384
NREC = 64


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


def _rules(tag, nl, rec, f, info, fo, io):
    d = float(np.abs(f - fo).max())
    equal = int((info["iterations"] == io["iterations"]).sum())
    dw = float(np.abs(_wrench8(rec, f) - _wrench8(rec, fo)).max()) if nl == 8 else None
    print(f"straight-line | {tag} | worst |f - f_oracle| {d:.2e} N" + (f" (foot wrench {dw:.2e})" if dw is not None else "")
          + f" | iteration words equal on {equal} of {len(rec)}, mean {info['iterations'].mean():.2f} | status counts "
          f"{np.bincount(info['status'], minlength=6).tolist()}")
    assert np.array_equal(info["status"], io["status"]) and (info["status"] == 0).all(), tag
    assert d < (1e-5 if nl == 8 else 1e-6), (tag, d)
    if nl == 8:
        assert dw < 1e-7, (tag, dw)
    assert np.abs(f[S.swing_rows(rec, nl)]).max() == 0.0, tag
    assert np.array_equal(info["iterations"], io["iterations"]), (tag, equal)


def _both_forms(pkg, lib, p, rec, call, tag):
    """(forces, info) of the all-LDS form on rec, after holding the workspace form on the tiled records to its bytes"""
    n = len(rec)
    with _handle(pkg, lib, p, CAP) as s:
        assert s.kernel_for_batch(n) == "wform_lds"
        f, info = getattr(s, call)(rec)
        assert _last(pkg, s) == "wform_lds"
        t = S.tiled(rec, _first_batch_beyond(s, "wform_lds", CAP))
        assert len(t) <= CAP and s.kernel_for_batch(len(t)) == "wform_ws"
        ft, it_ = getattr(s, call)(t)
        assert _last(pkg, s) == "wform_ws"
    nd = int((np.abs(ft[:n] - f).max(axis=1) > 0).sum())
    print(f"straight-line | {tag} | workspace form at {len(t)} instances against the all-LDS form: {nd} instances differ, largest "
          f"difference {float(np.abs(ft[:n] - f).max()):.2e} N, iteration words equal {np.array_equal(it_['iterations'][:n], info['iterations'])}")
    assert S.copies_identical(ft, n) and S.copies_identical(it_["status"], n) and S.copies_identical(it_["iterations"], n), tag
    assert _same(ft[:n], f) and _same(it_["status"][:n], info["status"]) and _same(it_["iterations"][:n], info["iterations"]), tag
    return f, info


@pytest.mark.parametrize("model,N", CASES, ids=[f"{m}-N{N}" for m, N in CASES])
def test_every_model_on_every_stance_set(pkg, lib, oracle, model, N):
    gen, config, params, call, masks, nl = MODELS[model]
    rec = getattr(pkg, gen)(NREC, config_id=config)
    rec["contacts"] = np.array(masks, dtype=np.float64)[np.arange(NREC) % len(masks)]
    fo, io = getattr(oracle, call)(getattr(oracle, params)(N, 0), rec, threads=8)
    tag = f"{model} N={N}"
    f, info = _both_forms(pkg, lib, getattr(pkg, params)(N, pkg.MODE_CONVERGED, lib), rec, call, tag)
    _rules(tag + ", all LDS", nl, rec, f, info, fo, io)


def test_footholds_and_references_far_from_nominal(pkg, lib, oracle):
    N = 10
    far = np.isin(F.cells("quat", N)[0], [F.KINDS.index("ahead"), F.KINDS.index("aside")])
    rec = F.quat(pkg, N)[far]
    assert len(rec) == NREC
    po = oracle.default_params(N, 0)
    fo, io = oracle.solve(po, rec, threads=8)
    _, inom = oracle.solve(po, F.quat(pkg, N, footholds=False, references=False)[far], threads=8)
    print(f"straight-line | far from nominal | oracle iterations mean {io['iterations'].mean():.2f} (at most {io['iterations'].max()}), "
          f"on the generator's records {inom['iterations'].mean():.2f} (at most {inom['iterations'].max()})")
    assert io["iterations"].mean() > inom["iterations"].mean() + 5 and (io["iterations"] >= inom["iterations"]).mean() >= 0.9
    f, info = _both_forms(pkg, lib, pkg.default_params(N, pkg.MODE_CONVERGED, lib), rec, "solve", "quat N=10, far from nominal")
    _rules("quat N=10, far from nominal, all LDS", 4, rec, f, info, fo, io)


def test_warm_started_second_solve_on_another_stance_set(pkg, lib, oracle):
    N = 10
    first, second = S.warm_pairs(pkg)
    pick = (7 * np.arange(NREC)) % len(first)
    first, second = first[pick], second[pick]
    landed = ((second["contacts"] == 1) & (first["contacts"] == 0)).any(axis=1)
    assert landed.sum() >= NREC // 2, int(landed.sum())
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    p.ipm_mu0 = 1e-6
    with _handle(pkg, lib, p, CAP) as s:
        assert s.kernel_for_batch(NREC) == "wform_lds"      # (a warm-started call shares the plain solve's choice)
        f0, i0, tu0 = s.solve_warm(first, None)
        f1, i1, tu1 = s.solve_warm(second, tu0)
        b1 = _first_batch_beyond(s, "wform_lds", CAP)
        t0, t1 = S.tiled(first, b1), S.tiled(second, b1)
        assert len(t0) <= CAP and s.kernel_for_batch(len(t0)) == "wform_ws"
        g0, j0, tv0 = s.solve_warm(t0, None)
        g1, j1, tv1 = s.solve_warm(t1, tv0)
    for a, b in ((g0, f0), (j0["status"], i0["status"]), (j0["iterations"], i0["iterations"]), (tv0, tu0),
                 (g1, f1), (j1["status"], i1["status"]), (j1["iterations"], i1["iterations"]), (tv1, tu1)):
        assert S.copies_identical(a, NREC) and _same(a[:NREC], b)
    po = oracle.default_params(N, 0)
    po.ipm_mu0 = 1e-6
    fo0, io0, _ = oracle.solve_warm(po, first, None, threads=8)
    fo1, io1, _ = oracle.solve_warm(po, second, tu0, threads=8)
    print(f"straight-line | warm start | {int(landed.sum())} of {NREC} records with a landed leg | workspace form at {len(t0)}: the all-LDS form's bytes")
    _rules("quat N=10, cold tick, all LDS", 4, first, f0, i0, fo0, io0)
    _rules("quat N=10, warm tick on another stance set, all LDS", 4, second, f1, i1, fo1, io1)
