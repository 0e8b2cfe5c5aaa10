"""GPU suite (-m gpu): the lane-parallel phases of the one-wave kernels (all-LDS form) on ConvexMpc's problem and on the
8-point model, at the horizons where their trip counts change.

In the all-LDS form (one wave per SIMD) two lane-parallel phases of an iteration, the wrench pass and the directions, load
their LDS operands up front into registers of their own (`ONEW`, qmpc_wform.h), and the trial rollout broadcasts the wrench
inside DPP row 0; the workspace forms keep the loads where the operands are used and compile to the code they had.
QuatMpc's kernel is covered by tests/test_gpu_wave_phase_loads.py; here are the other two models, whose instantiations
of the same phases the compiler schedules, and may contract, on its own:
  ConvexMpc, N = 1, 10, 11, 17, 20   6 N and 4 N cross 64 lanes at N = 11 and N = 17; N = 10 is bench.py's ConvexMpc kernel of
                                     this form; N = 20 is the horizon at which an earlier form of this change returned other bytes
  8-point,   N = 1, 8, 9, 11, 16     8 N crosses 64 lanes at N = 9, 6 N at N = 11
64 records per case, record k on stance set k mod 15 of MASKS4 (k mod 16 of MASKS8) of tests/stance_sets.py: swing legs
included (the `stance == false` side of the directions); the early iterations' shortened steps run the wrench pass with dU.

Rules, those of the model's stance-set test (tests/test_gpu_stance_sets.py): status words equal to the oracle's and all 0;
forces within 1e-6 N (8-point model: corner forces 1e-5, foot wrench 1e-7); swing forces exactly 0; iteration counts equal on
>= 97 %.  Then the same records tiled to just beyond the all-LDS form's last batch (asked of the handle): the workspace
form's forces, status and iteration words are the all-LDS form's BYTES.  The workspace forms are the parent commit's code,
instruction for instruction (profiles/r19_isa_same.txt), and the parent's two forms return the same bytes in all ten cases
(profiles/r19_tests_parent.log), so this holds the all-LDS forms to the parent's arithmetic.  No case is left out.
Measured: 0 instances differ in all ten cases.  (With the ConvexMpc directions' Winv product left to the compiler's contraction
all five ConvexMpc cases differ, 27 .. 64 instances by up to 1.2e-10 N: profiles/r19_tests_unpinned_directions.log;
cv_winv_mul_dirs pins the pairing.)"""
import numpy as np
import pytest

import stance_sets as S
from test_gpu_stance_sets import _first_batch_beyond, _handle, _last, _same, _wrench8

pytestmark = pytest.mark.gpu

# model: (records, default params, Solver call, oracle call, stance sets, contact points)
MODELS = {
    "convex": ("random_go1_convex_states", 12, "default_convex_params", "convex_solve", "convex_solve", S.MASKS4, 4),
    "biped8": ("random_biped8_states", 5, "default_biped8_params", "solve8", "solve8", S.MASKS8, 8),
}
CASES = [("convex", N) for N in (1, 10, 11, 17, 20)] + [("biped8", N) for N in (1, 8, 9, 11, 16)]
CAP = 16384      # (ConvexMpc at N = 1 stays in the all-LDS form up to 7680 instances)


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


def _records(pkg, model, n=64):
    gen, config, _, _, _, masks, _ = MODELS[model]
    rec = getattr(pkg, gen)(n, config_id=config)
    rec["contacts"] = np.array(masks, dtype=np.float64)[np.arange(n) % len(masks)]
    return rec


def _rules(tag, model, rec, f, info, fo, io):
    nl = MODELS[model][6]
    d = float(np.abs(f - fo).max())
    share = float((info["iterations"] == io["iterations"]).mean())
    dw = float(np.abs(_wrench8(rec, f) - _wrench8(rec, fo)).max()) if nl == 8 else None
    print(f"batched-loads | {tag} | worst |f - f_oracle| {d:.2e} N" + (f" (foot wrench {dw:.2e})" if dw is not None else "")
          + f" | iteration counts equal on {100 * share:.2f} % | status counts {np.bincount(info['status'], minlength=6).tolist()}")
    assert np.array_equal(info["status"], io["status"]) and (info["status"] == 0).all(), tag
    assert d < (1e-5 if nl == 8 else 1e-6), (tag, d)
    if nl == 8:
        assert dw < 1e-7, (tag, dw)
    assert np.abs(f[S.swing_rows(rec, nl)]).max() == 0.0, tag
    assert share >= 0.97, (tag, share)


@pytest.mark.parametrize("model,N", CASES, ids=[f"{m}-N{N}" for m, N in CASES])
def test_all_lds_form_against_the_oracle_and_the_workspace_forms_bytes(pkg, lib, oracle, model, N):
    _, _, params, call, ocall, _, _ = MODELS[model]
    rec = _records(pkg, model)
    n = len(rec)
    fo, io = getattr(oracle, ocall)(getattr(oracle, params)(N, 0), rec, threads=8)
    p = getattr(pkg, params)(N, pkg.MODE_CONVERGED, lib)
    with _handle(pkg, lib, p, CAP) as s:
        assert s.kernel_for_batch(n) == "wform_lds"
        f, info = getattr(s, call)(rec)
        assert _last(pkg, s) == "wform_lds"
        b1 = _first_batch_beyond(s, "wform_lds", CAP)
        t = S.tiled(rec, b1)
        assert len(t) <= CAP and s.kernel_for_batch(len(t)) == "wform_ws"
        ft, it_ = getattr(s, call)(t)
        assert _last(pkg, s) == "wform_ws"
    _rules(f"{model} N={N}, all LDS", model, rec, f, info, fo, io)
    nd = int((np.abs(ft[:n] - f).max(axis=1) > 0).sum())
    print(f"batched-loads | {model} N={N} | workspace form at {len(t)} instances against the all-LDS form: {nd} instances differ, "
          f"largest difference {float(np.abs(ft[:n] - f).max()):.2e} N, iteration words equal "
          f"{np.array_equal(it_['iterations'][:n], info['iterations'])}")
    assert S.copies_identical(ft, n) and S.copies_identical(it_["status"], n) and S.copies_identical(it_["iterations"], n)
    assert _same(ft[:n], f) and _same(it_["status"][:n], info["status"]) and _same(it_["iterations"][:n], info["iterations"])
