"""GPU suite (-m gpu): QuatMpc solves with a contact schedule over the horizon (qmpc_solve_schedule*, include/qmpc.h; DESIGN.md
section 3z; qmpc_wform_sched.hip: qmpc_solve_w_sched_kernel).

1. a constant schedule gives qmpc_solve_instances*' bytes on every variant the planner takes (all-LDS, workspace, long-horizon
   all-LDS, slack-in-workspace), with per-instance records and with iparams = NULL against uniform records, host and device calls
2. the GPU's trajectories on the fixture instances are the certified points of tests/golden/schedule_fixtures.npz
3. the GPU's own answers under the four schedule families pass the certificate of tests/kkt_schedule.py (the independent
   problem statement: the oracle has no per-knot contacts), with tests/test_kkt_certificate.py's tolerances; every instance solves
4. the schedule acts: forces move to the new legs at the switch knot, and the first knot already differs
5. instances are independent (permutation, per-instance verdicts) and the call-level refusals hold"""
import numpy as np
import pytest

import kkt_schedule as KS
from test_kkt_certificate import TOL_FEASIBILITY, TOL_INDEPENDENT, TOL_STATIONARITY

pytestmark = pytest.mark.gpu

from pathlib import Path  # noqa: E402

FIX = Path(__file__).resolve().parent / "golden" / "schedule_fixtures.npz"
# the smallest batches at which the planner takes each variant: (N, B) -> family, LDS-resident or not
SIZES = {(10, 1024): "wform_lds", (10, 8192): "wform_ws", (20, 256): "wform_lds", (20, 4096): "wform_ws"}
FAMILIES = ("constant", "trot_four_other", "trot_other", "trot_three")


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


@pytest.fixture(scope="module")
def fix():
    return np.load(FIX)


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.fixture(scope="module")
def solved(pkg, lib):
    """(N, B, family) -> (records, schedule, forces, info, traj_u, traj_x) of one schedule call on the handle's own values; each
    solved once and shared, never changed."""
    cache = {}

    def get(N, B, fam):
        if (N, B, fam) not in cache:
            p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
            rec = pkg.random_go1_trot_states(B, config_id=2)
            sched = pkg.schedule_families(rec, N)[fam]
            s = pkg.Solver(p, B, device=0, lib=lib)
            assert s.kernel_for_schedule(B) == SIZES[(N, B)]
            out = s.solve_schedule(rec, sched, None, want_traj=True)
            assert pkg.KERNEL_FAMILY[s.query(pkg.QUERY_LAST_KERNEL)] == SIZES[(N, B)]
            s.close()
            for a in (rec, sched) + out:
                a.setflags(write=False)
            cache[(N, B, fam)] = (rec, sched) + out
        return cache[(N, B, fam)]

    return get


# ---- 1. identity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,B", list(SIZES))
def test_constant_schedule_equals_solve_instances(pkg, lib, N, B):
    import torch

    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    rec = np.concatenate([pkg.go1_stand_input(), pkg.random_go1_trot_states(B - 1, config_id=2)])
    sched = pkg.constant_schedule(rec, N)
    ip = pkg.random_go1_variants(6, seed=7)[np.arange(B) % 6]
    s = pkg.Solver(p, B, device=0, lib=lib)
    s.set_instances_policy("auto")      # the lane kernel has no schedule form: the policy changes nothing for this call
    assert s.kernel_for_schedule(B) == SIZES[(N, B)]
    s.set_instances_policy("wave")
    assert s.kernel_for_schedule(B) == SIZES[(N, B)] == s.kernel_for_instances(B)
    want = s.solve_instances(rec, ip, want_traj=True)
    got = s.solve_schedule(rec, sched, ip, want_traj=True)
    assert pkg.KERNEL_FAMILY[s.query(pkg.QUERY_LAST_KERNEL)] == SIZES[(N, B)]
    assert (want[1]["status"] == 0).mean() > 0.95
    for a, b, name in zip(got, want, ("forces", "info", "traj_u", "traj_x")):
        assert _same(a, b), name
    # iparams = NULL: the handle's own values, against uniform records through qmpc_solve_instances
    want_u = s.solve_instances(rec, pkg.instance_params(p, B), want_traj=True)
    got_u = s.solve_schedule(rec, sched, None, want_traj=True)
    for a, b, name in zip(got_u, want_u, ("forces", "info", "traj_u", "traj_x")):
        assert _same(a, b), name
    # the device-buffer calls: qmpc_solve_instances_device's forces and records, and the host call's trajectories
    d_in = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    d_ip = torch.from_numpy(ip.view(np.uint8).copy()).cuda()
    d_sc = torch.from_numpy(sched.copy()).cuda()
    d_f = torch.full((2, B, 12), -1.0, dtype=torch.float64, device="cuda")
    d_info = torch.zeros(2, B * pkg.INFO_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_tu = torch.full((B, N, 12), -1.0, dtype=torch.float64, device="cuda")
    d_tx = torch.full((B, N + 1, 13), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    s.solve_instances_device(B, d_in.data_ptr(), d_ip.data_ptr(), d_f[0].data_ptr(), d_info[0].data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    s.solve_schedule_device(B, d_in.data_ptr(), d_ip.data_ptr(), d_sc.data_ptr(), d_f[1].data_ptr(), d_info[1].data_ptr(), d_tu.data_ptr(),
                            d_tx.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    f, info = d_f.cpu().numpy(), d_info.cpu().numpy()
    assert _same(f[0], f[1]) and _same(info[0], info[1])
    assert _same(f[1], got[0]) and info[1].tobytes() == got[1].tobytes()
    assert _same(d_tu.cpu().numpy(), got[2]) and _same(d_tx.cpu().numpy(), got[3])
    # ... without records, info and trajectories
    d_f[1].fill_(-1.0)
    torch.cuda.synchronize()
    s.solve_schedule_device(B, d_in.data_ptr(), 0, d_sc.data_ptr(), d_f[1].data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    assert _same(d_f[1].cpu().numpy(), got_u[0])
    s.close()


# ---- 2. certified points -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,B", list(SIZES))
def test_certified_points(pkg, fix, solved, N, B):
    case, n = ("n10", 8) if N == 10 else ("n20", 2)
    assert _same(pkg.random_go1_trot_states(B, config_id=2)[:8], pkg.random_go1_trot_states(8, config_id=2))
    for fam in fix[case + "_families"]:
        rec, sched, f, info, tu, tx = solved(N, B, str(fam))
        U = fix[f"{case}_{fam}_U"]
        assert (info["status"][:n] == 0).all(), (fam, info["status"][:n])
        d = np.abs(tu[:n] - U).max()
        print(f"N={N} B={B} {fam}: max |traj_u - certified point| = {d:.2e} N over {n} instances")
        assert d <= TOL_INDEPENDENT, fam


# ---- 3. the certificate on the GPU's own answers --------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("N,B,n", [(10, 1024, 64), (10, 8192, 16), (20, 4096, 16)])
def test_gpu_answers_pass_the_certificate(pkg, lib, solved, N, B, n, fam):
    rec, sched, f, info, tu, tx = solved(N, B, fam)
    assert (info["status"][:n] == 0).all(), np.flatnonzero(info["status"][:n] != 0)      # every instance: none is left out
    par = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    worst = {"stationarity_nnls": 0.0, "violation": 0.0, "swing_force": 0.0}
    for i in range(n):
        prob = KS.ScheduleProblem(par, rec[i], sched[i])
        r = prob.kkt(tu[i])
        for k in worst:
            worst[k] = max(worst[k], r[k])
        swing = tu[i].reshape(N, 4, 3)[prob.conk == 0]
        assert (swing == 0.0).all() and not np.signbit(swing).any(), i      # every swing (knot, leg): exactly +0.0
    print(f"N={N} B={B} {fam}: stationarity_nnls {worst['stationarity_nnls']:.2e} violation {worst['violation']:.2e} over {n} "
          f"instances, iterations mean {info['iterations'][:n].mean():.1f} max {info['iterations'][:n].max()}")
    assert worst["stationarity_nnls"] <= TOL_STATIONARITY
    assert worst["violation"] <= TOL_FEASIBILITY
    assert worst["swing_force"] == 0.0
    assert _same(f[:n], tu[:n, 0])


# ---- 4. the schedule acts ----------------------------------------------------------------------------------------------------------
def test_the_schedule_moves_the_forces(solved):
    N, B, n = 10, 1024, 64
    rec, sched, f, info, tu, tx = solved(N, B, "trot_other")
    _, _, fc, ic, tuc, _ = solved(N, B, "constant")
    cut = (2 * N) // 5
    F = tu[:n].reshape(n, N, 4, 3)
    bits = (sched[:n, :, None] >> np.arange(4)) & 1      # [n][N][4]
    old, new = bits[:, 0] == 1, bits[:, 0] == 0          # [n][4]
    trot = np.flatnonzero(old.sum(1) == 2)               # (a record whose four legs all stand has no old legs to leave)
    assert trot.size >= n // 2 and (bits[trot, cut:] == new[trot, None, :]).all() and (bits[trot, :cut] == old[trot, None, :]).all()
    for i in trot:
        assert (F[i][cut:, old[i]] == 0.0).all() and (np.abs(F[i][:cut, old[i]]).max(axis=2) > 0).all()
        assert (np.abs(F[i][cut:, new[i]]).max(axis=2) > 0).all() and (F[i][:cut, new[i]] == 0.0).all()
    d0 = np.abs(f[:n] - fc[:n]).max(axis=1)
    print(f"first-knot force, trot -> other against constant: max {d0.max():.3e} N, median {np.median(d0):.3e} N")
    assert (ic["status"][:n] == 0).all() and (info["status"][:n] == 0).all()
    assert (d0 > 1e-3).any()


# ---- 5. independence and verdicts -----------------------------------------------------------------------------------------------
def test_permutation_and_per_instance_verdicts(pkg, lib):
    N, B = 10, 1024
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    rec = pkg.random_go1_trot_states(B, config_id=2)
    fams = pkg.schedule_families(rec, N)
    sched = np.stack([fams[n] for n in FAMILIES])[np.arange(B) % 4, np.arange(B)]      # the four families interleaved
    ip = pkg.random_go1_variants(6, seed=7)[np.arange(B) % 6]
    s = pkg.Solver(p, B, device=0, lib=lib)
    base = s.solve_schedule(rec, sched, ip, want_traj=True)
    perm = np.random.default_rng(1).permutation(B)
    got = s.solve_schedule(rec[perm], sched[perm], ip[perm], want_traj=True)
    for a, b in zip(got, base):
        assert _same(a, b[perm])
    # one instance with an empty knot, one with a byte of 16, one with an invalid record
    bad_s, bad_i = sched.copy(), ip.copy()
    bad_s[100, 7] = 0
    bad_s[200, 3] = 16
    bad_i["mass"][300] = -1.0
    f, info, tu, tx = s.solve_schedule(rec, bad_s, bad_i, want_traj=True)
    for i, code in ((100, pkg.NO_CONTACT), (200, pkg.BAD_PARAMS), (300, pkg.BAD_PARAMS)):
        assert info["status"][i] == code and info["iterations"][i] == 0, (i, info[i])
        assert not f[i].any() and not tu[i].any() and not tx[i].any()
    keep = np.setdiff1d(np.arange(B), (100, 200, 300))
    for a, b in zip((f, info, tu, tx), base):
        assert _same(a[keep], b[keep])
    # ... and a run without the bad instances gives the neighbours the same bytes
    alone = s.solve_schedule(rec[keep], sched[keep], ip[keep], want_traj=True)
    for a, b in zip((f, info, tu, tx), alone):
        assert _same(a[keep], b)
    s.close()


def test_unsupported_handles_and_sizes(pkg, lib, monkeypatch):
    rec = pkg.random_go1_trot_states(8, config_id=2)
    for params in (pkg.default_convex_params(20, pkg.MODE_CONVERGED, lib), pkg.default_biped8_params(16, pkg.MODE_CONVERGED, lib),
                   pkg.default_params(10, pkg.MODE_REFERENCE, lib)):
        s = pkg.Solver(params, 8, device=0, lib=lib)
        assert s.kernel_for_schedule(8) == "none"
        with pytest.raises(pkg.QmpcError) as e:
            s.solve_schedule(rec, pkg.constant_schedule(rec, params.horizon))
        assert e.value.code == pkg.UNSUPPORTED
        s.close()
    p = pkg.default_params(10, pkg.MODE_CONVERGED, lib)
    s = pkg.Solver(p, 16, device=0, lib=lib)
    rec17 = pkg.random_go1_trot_states(17, config_id=2)
    with pytest.raises(pkg.QmpcError) as e:
        s.solve_schedule(rec17, pkg.constant_schedule(rec17, 10))
    assert e.value.code == pkg.BATCH_TOO_LARGE
    # the host call's schedule staging: N bytes per instance, on first use, counted
    s.prepare_instances()
    before = s.query(pkg.QUERY_DEVICE_BYTES)
    s.solve_schedule(rec, pkg.constant_schedule(rec, 10))
    assert s.query(pkg.QUERY_DEVICE_BYTES) - before == 10 * 16
    s.close()
    monkeypatch.setenv("QMPC_WFORM", "0")      # read by qmpc_create: no wrench-form kernel at all
    s = pkg.Solver(p, 8, device=0, lib=lib)
    assert s.kernel_for_schedule(8) == "none"
    with pytest.raises(pkg.QmpcError) as e:
        s.solve_schedule(rec, pkg.constant_schedule(rec, 10))
    assert e.value.code == pkg.UNSUPPORTED
    s.close()
