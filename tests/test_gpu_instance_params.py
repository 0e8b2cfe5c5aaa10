"""GPU suite (-m gpu): per-instance robot and cost parameters (qmpc_solve_instances*, include/qmpc.h).

Instance i is solved with the handle's parameters and the mass, inertia, friction coefficient, force bound and cost weights
of its own record.  The kernel (qmpc_wform.hip: qmpc_solve_w_inst_kernel) is the wrench-form wave kernel of a plain solve
with P read per workgroup, so wherever both calls take the same variant the results are those of a plain solve on a handle
carrying the instance's values, bit for bit; across variants (and against the lane kernel of large plain batches) they agree
to rounding, and against the CPU oracle to 1e-6 N."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


def _states(pkg, B, config_id=2):
    return np.concatenate([pkg.go1_stand_input(), pkg.random_go1_trot_states(B - 1, config_id=config_id)])


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.mark.parametrize("N,B", [(10, 1), (10, 1024), (10, 8192), (20, 256), (20, 4096)])
def test_uniform_records_equal_the_plain_solve(pkg, lib, N, B):
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    rec = _states(pkg, B) if B > 1 else pkg.go1_stand_input()
    s = pkg.Solver(p, B, device=0, lib=lib)
    assert s.kernel_for_instances(B) == s.kernel_for_batch(B)
    assert s.kernel_for_instances(B) in ("wform_lds", "wform_ws")
    fi, ii, tui, txi = s.solve_instances(rec, pkg.instance_params(p, B), want_traj=True)
    assert pkg.KERNEL_FAMILY[s.query(pkg.QUERY_LAST_KERNEL)] == s.kernel_for_instances(B)
    fp, ip, tup, txp = s.solve(rec, want_traj=True)
    s.close()
    assert (ii["status"] == 0).mean() > 0.95
    assert _same(fi, fp) and _same(ii, ip) and _same(tui, tup) and _same(txi, txp)


def test_the_handles_own_physics_are_ignored(pkg, lib):
    B = 1024
    go1 = pkg.default_params(10, pkg.MODE_CONVERGED, lib)
    heavy = go1.copy()
    heavy.mass = 30.0
    for k in range(9):
        heavy.inertia[k] *= 3.0
    heavy.mu, heavy.fz_max = 0.2, 500.0
    for k in range(13):
        heavy.q_weights[k] *= 2.0
    rec = _states(pkg, B)
    sh = pkg.Solver(heavy, B, device=0, lib=lib)
    fi, ii = sh.solve_instances(rec, pkg.instance_params(go1, B))
    fh, _ = sh.solve(rec)
    sh.close()
    sg = pkg.Solver(go1, B, device=0, lib=lib)
    fg, ig = sg.solve(rec)
    sg.close()
    assert _same(fi, fg) and _same(ii, ig)
    assert np.abs(fh - fg).max() > 1.0      # (the heavy handle's own solve is another problem)


def _groups(pkg, lib, N, B, K=6, seed=7):
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    sets = pkg.random_go1_variants(K, seed=seed)
    ip = sets[np.arange(B) % K]
    rec = _states(pkg, B)
    s = pkg.Solver(p, B, device=0, lib=lib)
    fam = s.kernel_for_instances(B)
    f, info, tu, tx = s.solve_instances(rec, ip, want_traj=True)
    s.close()
    for g in range(K):
        idx = np.arange(g, B, K)
        sg = pkg.Solver(pkg.params_with(p, sets[g]), len(idx), device=0, lib=lib)
        yield g, idx, fam, sg.kernel_for_batch(len(idx)), (f[idx], info[idx], tu[idx], tx[idx]), sg.solve(rec[idx], want_traj=True)
        sg.close()


@pytest.mark.parametrize("B", [1024, 8192])
def test_heterogeneous_batch_equals_per_handle_solves(pkg, lib, B):
    for g, idx, fam, fam_g, got, want in _groups(pkg, lib, 10, B):
        assert fam == fam_g, (g, fam, fam_g)
        assert (got[1]["status"] == 0).mean() > 0.95
        for a, b in zip(got, want):
            assert _same(a, b), g


def test_heterogeneous_batch_long_horizon(pkg, lib):
    for g, idx, fam, fam_g, got, want in _groups(pkg, lib, 20, 2048):
        assert np.array_equal(got[1]["status"], want[1]["status"]), g
        assert np.abs(got[0] - want[0]).max() < 1e-7, g


def test_random_variants_against_the_oracle(pkg, lib, oracle):
    B, N = 4096, 10
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    ip = pkg.random_go1_variants(B, seed=11)
    rec = _states(pkg, B)
    s = pkg.Solver(p, B, device=0, lib=lib)
    f, info = s.solve_instances(rec, ip)
    s.close()
    assert (info["status"] == 0).mean() > 0.95
    sample = np.unique(np.linspace(0, B - 1, 256).astype(int))
    for i in sample:
        fo, io = oracle.solve(pkg.params_with(p, ip[i]), rec[i:i + 1])
        assert info["status"][i] == io["status"][0], i
        if io["status"][0] == 0:
            assert np.abs(f[i] - fo[0]).max() <= 1e-6, (i, np.abs(f[i] - fo[0]).max())


def test_each_instance_keeps_its_own_friction_cone(pkg, lib):
    B, N = 1024, 10
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    p.mu = 0.9
    rng = np.random.default_rng(3)
    ip = pkg.instance_params(p, B)
    ip["mu"] = rng.uniform(0.3, 0.5, B)
    ip["fz_max"] = rng.uniform(60.0, 120.0, B)
    rec = pkg.random_go1_trot_states(B, config_id=4, tilt_max=0.5)
    # fast lateral references from rest: the solve wants large horizontal forces, which the cone clips
    rec["lin_vel_body"] = 0.0
    rec["vel_ref_body"][:, 0] = rng.choice([-2.0, 2.0], B)
    rec["vel_ref_body"][:, 1] = rng.uniform(-1.0, 1.0, B)
    s = pkg.Solver(p, B, device=0, lib=lib)
    f, info = s.solve_instances(rec, ip)
    f9, _ = s.solve(rec)
    s.close()
    ok = info["status"] == 0
    assert ok.mean() > 0.9
    R = rec["rot"].reshape(B, 3, 3)
    fw = np.einsum("bij,blj->bli", R, f.reshape(B, 4, 3))      # world-frame force per leg
    stance = rec["contacts"] > 0
    mu = ip["mu"][:, None]
    fric = np.maximum.reduce([fw[..., 0] - mu * fw[..., 2], -fw[..., 0] - mu * fw[..., 2],
                              fw[..., 1] - mu * fw[..., 2], -fw[..., 1] - mu * fw[..., 2]])
    assert (fric[ok][stance[ok]] <= 1e-6).all(), fric[ok][stance[ok]].max()
    assert (fw[..., 2][ok][stance[ok]] <= ip["fz_max"][:, None].repeat(4, 1)[ok][stance[ok]] + 1e-6).all()
    active = (fric >= -1e-6) & stance & ok[:, None]
    assert active.any(axis=1).sum() >= 10, active.any(axis=1).sum()
    assert np.abs(f - f9)[active.any(axis=1)].max() > 1e-3


def test_bad_records_are_flagged_alone(pkg, lib):
    B, N = 512, 10
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    good = pkg.random_go1_variants(B, seed=5)
    rec = _states(pkg, B)
    bad = good.copy()
    plant = {3: ("mass", np.nan), 10: ("mass", 0.0), 17: ("inertia", 0.0), 24: ("inertia", np.inf), 30: ("r_weights", 0.0),
             41: ("q_weights", -1.0), 50: ("w", -1.0), 60: ("mu", 0.0), 70: ("fz_max", -5.0), 80: ("fz_max", np.nan)}
    for i, (field, v) in plant.items():
        if field in ("r_weights", "q_weights"):
            bad[field][i, 2] = v
        else:
            bad[field][i] = v
    s = pkg.Solver(p, B, device=0, lib=lib)
    fb, ib, tub, txb = s.solve_instances(rec, bad, want_traj=True)
    fg, ig, tug, txg = s.solve_instances(rec, good, want_traj=True)
    s.close()
    idx = np.array(sorted(plant))
    assert (ib["status"][idx] == pkg.BAD_PARAMS).all() and (ib["iterations"][idx] == 0).all()
    assert (fb[idx] == 0).all() and (tub[idx] == 0).all() and (txb[idx] == 0).all()
    assert (ig["status"] != pkg.BAD_PARAMS).all()
    rest = np.setdiff1d(np.arange(B), idx)
    assert _same(fb[rest], fg[rest]) and _same(ib[rest], ig[rest]) and _same(tub[rest], tug[rest]) and _same(txb[rest], txg[rest])


def test_large_batch_stays_on_the_wave_kernel(pkg, lib, oracle):
    B, N = 32768, 10
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    rec = pkg.random_go1_trot_states(B, config_id=2)
    s = pkg.Solver(p, B, device=0, lib=lib)
    assert s.kernel_for_instances(B) == "wform_ws"
    assert s.kernel_for_batch(B) in ("lane", "lane_handoff")
    fi, ii = s.solve_instances(rec, pkg.instance_params(p, B))
    assert pkg.KERNEL_FAMILY[s.query(pkg.QUERY_LAST_KERNEL)] == "wform_ws"
    fp, ip = s.solve(rec)
    assert np.array_equal(ii["status"], ip["status"])
    assert np.abs(fi - fp).max() < 1e-7
    iv = pkg.random_go1_variants(B, seed=13)
    fv, infv = s.solve_instances(rec, iv)
    s.close()
    for i in np.linspace(0, B - 1, 128).astype(int):
        fo, io = oracle.solve(pkg.params_with(p, iv[i]), rec[i:i + 1])
        assert infv["status"][i] == io["status"][0], i
        if io["status"][0] == 0:
            assert np.abs(fv[i] - fo[0]).max() <= 1e-6, i


def test_device_entry_and_instance_independence(pkg, lib):
    import torch

    B, N = 2048, 10
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    rec = _states(pkg, B)
    ip = pkg.random_go1_variants(B, seed=17)
    s = pkg.Solver(p, B, device=0, lib=lib)
    f, info = s.solve_instances(rec, ip)
    d_in = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    d_ip = torch.from_numpy(ip.view(np.uint8).copy()).cuda()
    d_f = torch.full((B, 12), -1.0, dtype=torch.float64, device="cuda")
    d_info = torch.zeros(B * pkg.INFO_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    s.solve_instances_device(B, d_in.data_ptr(), d_ip.data_ptr(), d_f.data_ptr(), d_info.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    assert _same(d_f.cpu().numpy(), f) and d_info.cpu().numpy().tobytes() == info.tobytes()
    perm = np.random.default_rng(1).permutation(B)
    fp, ipf = s.solve_instances(rec[perm], ip[perm])
    s.close()
    assert _same(fp, f[perm]) and _same(ipf, info[perm])


def test_unsupported_handles_and_sizes(pkg, lib, monkeypatch):
    rec = pkg.random_go1_trot_states(8, config_id=2)
    for params in (pkg.default_convex_params(20, pkg.MODE_CONVERGED, lib), pkg.default_biped8_params(16, pkg.MODE_CONVERGED, lib),
                   pkg.default_params(10, pkg.MODE_REFERENCE, lib)):
        s = pkg.Solver(params, 8, device=0, lib=lib)
        assert s.kernel_for_instances(8) == "none"
        with pytest.raises(pkg.QmpcError) as e:
            s.solve_instances(rec, pkg.instance_params(params, 8))
        assert e.value.code == pkg.UNSUPPORTED
        s.close()
    p = pkg.default_params(10, pkg.MODE_CONVERGED, lib)
    s = pkg.Solver(p, 16, device=0, lib=lib)
    with pytest.raises(pkg.QmpcError) as e:
        s.solve_instances(pkg.random_go1_trot_states(17, config_id=2), pkg.instance_params(p, 17))
    assert e.value.code == pkg.BATCH_TOO_LARGE
    before = s.query(pkg.QUERY_DEVICE_BYTES)
    s.prepare_instances()
    grown = s.query(pkg.QUERY_DEVICE_BYTES) - before
    assert 760 * 16 <= grown <= 800 * 16, grown
    s.close()
    monkeypatch.setenv("QMPC_WFORM", "0")      # read by qmpc_create: no wrench-form kernel at all
    s = pkg.Solver(p, 8, device=0, lib=lib)
    assert s.kernel_for_instances(8) == "none"
    with pytest.raises(pkg.QmpcError) as e:
        s.solve_instances(rec, pkg.instance_params(p, 8))
    assert e.value.code == pkg.UNSUPPORTED
    s.close()
