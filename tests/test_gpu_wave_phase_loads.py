"""GPU suite (-m gpu): the trial rollout and the lane-parallel phases of the wave kernels at the horizons where their trip
counts change.

The trial rollout of the one-wave-per-SIMD form (rollout_closed_w<PF>, qmpc_wform.h) prefetches the next knot's gain row
only and loads the old state and the Jacobian blocks at the head of their own knot; its loop body holds two knots.  The
lane-parallel phases run in trips of 64 lanes.  The horizons are the ones where a trip structure changes:
  N = 1   a single knot: the rollout's two-knot body runs its first half only (no next knot to prefetch for), 6 / 4 live lanes
  N = 10  the benchmark's workload
  N = 11  an odd number of knots in the two-knot body; 6 N = 66 > 64: the wrench pass takes a second, partial trip
  N = 17  4 N = 68 > 64: the per-point phases (pre-pass, directions, apply) take a second, partial trip
64 QuatMpc records per horizon, record k on stance set k mod 15 of tests/stance_sets.py (all 15 non-empty sets of four
legs, one- and three-leg sets included; at N = 17 the nine sets of ENVELOPE_N20, three-leg sets included: beyond them the
converged mode does not converge in the CPU oracle either -- at N = 17 set 1000 ends at the iteration limit).

Rules, those of tests/test_gpu_stance_sets.py: status words equal to the oracle's and all 0, forces within 1e-6 N, swing
forces exactly 0, iteration counts equal on >= 97 %; the workspace forms return the all-LDS form's bytes."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import stance_sets as S
from test_gpu_stance_sets import _first_batch_beyond, _handle, _last, _same

pytestmark = pytest.mark.gpu

HORIZONS = (1, 10, 11, 17)
_cache = {}


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


def _records(pkg, N, n=64):
    masks = S.MASKS4 if N <= 12 else S.ENVELOPE_N20
    rec = pkg.random_go1_trot_states(n, config_id=3 if N > 12 else 2)
    rec["contacts"] = np.array(masks, dtype=np.float64)[np.arange(n) % len(masks)]
    return rec


def _oracle(pkg, oracle, N):
    if N not in _cache:
        _cache[N] = oracle.solve(oracle.default_params(N, 0), _records(pkg, N), threads=8)
    return _cache[N]


def _rules(tag, rec, f, info, fo, io):
    d = float(np.abs(f - fo).max())
    share = float((info["iterations"] == io["iterations"]).mean())
    print(f"phase-loads | {tag} | worst |f - f_oracle| {d:.2e} N | iteration counts equal on {100 * share:.2f} % | "
          f"status counts {np.bincount(info['status'], minlength=6).tolist()}")
    assert np.array_equal(info["status"], io["status"]) and (info["status"] == 0).all(), tag
    assert d < 1e-6, (tag, d)
    assert np.abs(f[S.swing_rows(rec)]).max() == 0.0, tag
    assert share >= 0.97, (tag, share)


@pytest.mark.parametrize("N", HORIZONS)
def test_all_lds_form_against_the_oracle_and_the_workspace_forms_bytes(pkg, lib, oracle, N):
    """The 64 records on the all-LDS kernel (the planner's choice at this size) against the oracle; then tiled to just beyond the
    batch at which the handle leaves the all-LDS form, as tests/test_gpu_stance_sets.py selects the workspace form: every copy
    returns the all-LDS form's bytes (forces, status and iteration words)."""
    rec = _records(pkg, N)
    n = len(rec)
    fo, io = _oracle(pkg, oracle, N)
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    with _handle(pkg, lib, p, 8192) as s:
        assert s.kernel_for_batch(n) == "wform_lds"
        f, info = s.solve(rec)
        assert _last(pkg, s) == "wform_lds"
        f2, info2 = s.solve(rec)      # the handle's LDS and workspace as the first call left them
        b1 = _first_batch_beyond(s, "wform_lds", 8192)
        t = S.tiled(rec, b1)
        assert s.kernel_for_batch(len(t)) == "wform_ws"
        ft, it_ = s.solve(t)
        assert _last(pkg, s) == "wform_ws"
    _rules(f"N={N}, all LDS", rec, f, info, fo, io)
    assert _same(f, f2) and _same(info["iterations"], info2["iterations"]) and _same(info["status"], info2["status"])
    print(f"phase-loads | N={N} | workspace form at {len(t)} instances against the all-LDS form: "
          f"largest difference {float(np.abs(ft[:n] - f).max()):.2e} N")
    assert S.copies_identical(ft, n) and S.copies_identical(it_["status"], n) and S.copies_identical(it_["iterations"], n)
    assert _same(ft[:n], f) and _same(it_["status"][:n], info["status"]) and _same(it_["iterations"][:n], info["iterations"])


def test_second_workspace_form_returns_the_same_bytes(pkg, lib):
    """From N = 13 on the planner has a second workspace form for the larger batches of the family (the slack arrays out of
    LDS as well, a lean layout without direction arrays: tests/golden/kernel_plans.txt.gz shows it at N = 20 from 1025 instances
    up to the lane kernel's first batch).  The family word does not tell the two forms apart, so the batch is the last one of
    the family, found by bisection on this handle: N = 17, the 64 records tiled, every copy the all-LDS form's bytes."""
    N = 17
    rec = _records(pkg, N)
    n = len(rec)
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    with _handle(pkg, lib, p, 32768) as s:
        f, info = s.solve(rec)
        assert _last(pkg, s) == "wform_lds"
        b1 = _first_batch_beyond(s, "wform_lds", 32768)
        b2 = _first_batch_beyond_family(s, b1, 32768)
        t = S.tiled(rec, b2 - n)[:b2 - 1]
        assert s.kernel_for_batch(len(t)) == "wform_ws"
        ft, it_ = s.solve(t)
        assert _last(pkg, s) == "wform_ws"
    k = (len(t) // n) * n
    assert S.copies_identical(ft[:k], n) and S.copies_identical(it_["iterations"][:k], n)
    assert _same(ft[:n], f) and _same(it_["status"][:n], info["status"]) and _same(it_["iterations"][:n], info["iterations"])


def _first_batch_beyond_family(s, lo, hi):
    """smallest batch > lo at which the handle plans another family than at lo"""
    fam = s.kernel_for_batch(lo)
    assert s.kernel_for_batch(hi) != fam
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if s.kernel_for_batch(mid) == fam else (lo, mid)
    return hi


def test_warm_started_second_solve_on_another_stance_set(pkg, lib, oracle):
    """One handle, N = 10: a cold qmpc_solve_warm on one stance set, then the next tick from its trajectory with every
    instance on ANOTHER set (record k moves from set k mod 15 to set (k + 7) mod 15: legs land, lift off, stay).  What a solve
    keeps per stance set between the iterations must not survive into the next solve.  The rules of
    test_warm_start_between_every_pair_of_stance_sets against oracle.solve_warm."""
    N, n = 10, 64
    first = _records(pkg, N)
    second = first.copy()
    second["lin_vel_body"] += 0.02
    second["contacts"] = np.array(S.MASKS4, dtype=np.float64)[(np.arange(n) + 7) % 15]
    assert not (first["contacts"] == second["contacts"]).all(axis=1).any()
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    p.ipm_mu0 = 1e-6
    with _handle(pkg, lib, p, n) as s:
        assert s.kernel_for_batch(n) == "wform_lds"
        f0, i0, tu0 = s.solve_warm(first, None)
        f1, i1, tu1 = s.solve_warm(second, tu0)
    po = oracle.default_params(N, 0)
    po.ipm_mu0 = 1e-6
    fo0, io0, _ = oracle.solve_warm(po, first, None, threads=8)
    fo1, io1, tuo1 = oracle.solve_warm(po, second, tu0, threads=8)
    di = np.abs(i1["iterations"].astype(int) - io1["iterations"].astype(int))
    print(f"phase-loads | warm start | cold {np.abs(f0 - fo0).max():.2e} N, warm {np.abs(f1 - fo1).max():.2e} N | "
          f"iteration counts equal on {100 * (di == 0).mean():.2f} %, within one on {100 * (di <= 1).mean():.2f} %")
    assert np.array_equal(i0["status"], io0["status"]) and (i0["status"] == 0).all() and np.abs(f0 - fo0).max() < 1e-6
    assert np.array_equal(i1["status"], io1["status"]) and (i1["status"] == 0).all()
    assert np.abs(f1 - fo1).max() < 1e-6
    assert (di == 0).mean() >= 0.9 and (di <= 1).mean() >= 0.95, np.bincount(di)
    assert np.abs(f1[S.swing_rows(second)]).max() == 0.0
    assert np.abs(tu1.reshape(n, -1) - tuo1.reshape(n, -1)).max() < 1e-5


@pytest.mark.parametrize("warm", ["cold", "warm"])
def test_persistent_loop_across_a_gait_switch_equals_the_per_tick_launches(warm):
    """Eight robots stand for 6 ticks and then trot for 40: stance and swing ticks both occur, so the stance set of a robot
    changes while its wave keeps the robot's LDS (the persistent kernel) -- against the per-tick launch form, byte for byte,
    as tests/test_gpu_parity.py::test_persistent_loop_kernel_equals_the_per_tick_sequence compares them (its worker; the form
    is read from the environment once per process)."""
    worker = Path(__file__).resolve().parent / "_loop_worker.py"
    robots, ticks = 8, 40
    out = {}
    for fused in ("0", "1"):
        env = dict(os.environ, QMPC_LOOP_FUSED=fused)
        r = subprocess.run([sys.executable, str(worker), str(robots), str(ticks), "10", "0", "quat", warm], env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        out[fused] = [l for l in r.stdout.splitlines() if l.startswith("SHA")][0]
    print("phase-loads | closed loop |", warm, "|", out["1"])
    assert out["0"] == out["1"]
    swing = int(out["1"].split()[3])
    assert 0 < swing < 4 * ticks * (robots - 1)      # (robot 2's records are rejected: it never steps)
