"""GPU suite (-m gpu): per-instance robot and cost parameters for ConvexMpc's problem (qmpc_convex_solve_instances*,
include/qmpc.h).

Instance i is solved with the handle's parameters and the mass, inertia, friction coefficient, force bound and cost weights of
its own record.  The kernel (qmpc_wform_cinst.hip: qmpc_solve_cw_inst_kernel) is qmpc_solve_cw_kernel with P read per
workgroup, so wherever a plain qmpc_convex_solve takes the same wrench-form variant the results are those of a plain solve on a
handle carrying the instance's values, bit for bit; where the plain solve takes the round-1 kernel they agree to the rounding
between ConvexMpc's wave families (status words equal, forces within 1e-7 N: the bound of tests/test_gpu_parity.py between
those families), and against the CPU oracle to 1e-6 N (the project's ConvexMpc parity bound).

Batch sizes, from the enumeration of tests/native/records_plan_host.cpp --check convex (default knobs): the smallest batch on variant
3 / 5 / 6 is 1 / 513 / 1025 at N = 20 (the plain solve takes the same variants there) and 1 / 769 / 2049 at N = 10 (where the
plain solve of 2049 instances takes the round-1 kernel)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _family(pkg, s):
    return pkg.KERNEL_FAMILY[s.query(pkg.QUERY_LAST_KERNEL)]


@pytest.mark.parametrize("N,B,same_variant", [(20, 1, True), (20, 513, True), (20, 1025, True), (10, 1, True), (10, 65, True),
                                               (10, 769, True), (10, 2049, False)])
def test_uniform_records_equal_the_plain_solve(pkg, lib, N, B, same_variant):
    p = pkg.default_convex_params(N, pkg.MODE_CONVERGED, lib)
    rec = pkg.random_go1_convex_states(B, config_id=13)
    s = pkg.Solver(p, B, device=0, lib=lib)
    fam = s.kernel_for_convex_instances(B)
    assert fam in ("wform_lds", "wform_ws") and s.kernel_for_instances(B) == "none"
    assert (fam == s.kernel_for_batch(B)) == same_variant
    fi, ii, tui, txi = s.convex_solve_instances(rec, pkg.instance_params(p, B), want_traj=True)
    assert _family(pkg, s) == fam
    fp, ip, tup, txp = s.convex_solve(rec, want_traj=True)
    s.close()
    assert (ii["status"] == 0).mean() > 0.95
    if same_variant:
        assert _same(fi, fp) and _same(ii, ip) and _same(tui, tup) and _same(txi, txp)
    else:
        print(f"N={N} B={B}: per-instance {fam} against the plain solve's round-1 kernel: max |df| {np.abs(fi - fp).max():.2e} N")
        assert np.array_equal(ii["status"], ip["status"])
        assert np.abs(fi - fp).max() <= 1e-7


def test_the_handles_own_physics_are_ignored(pkg, lib):
    B, N = 256, 20
    go1 = pkg.default_convex_params(N, pkg.MODE_CONVERGED, lib)
    heavy = go1.copy()
    heavy.mass = 30.0
    for k in range(9):
        heavy.inertia[k] *= 3.0
    heavy.mu, heavy.fz_max = 0.2, 500.0
    for k in range(13):
        heavy.q_weights[k] *= 2.0
    rec = pkg.random_go1_convex_states(B, config_id=13)
    sh = pkg.Solver(heavy, B, device=0, lib=lib)
    fi, ii = sh.convex_solve_instances(rec, pkg.instance_params(go1, B))
    fh, _ = sh.convex_solve(rec)
    sh.close()
    sg = pkg.Solver(go1, B, device=0, lib=lib)
    fg, ig = sg.convex_solve(rec)
    sg.close()
    assert _same(fi, fg) and _same(ii, ig)
    assert np.abs(fh - fg).max() > 1.0      # (the heavy handle's own solve is another problem)


def test_interleaved_parameter_sets_equal_per_handle_solves(pkg, lib):
    B, N, K = 256, 20, 4
    p = pkg.default_convex_params(N, pkg.MODE_CONVERGED, lib)
    sets = pkg.random_go1_convex_variants(K, seed=7)
    ip = sets[np.arange(B) % K]
    rec = pkg.random_go1_convex_states(B, config_id=13)
    s = pkg.Solver(p, B, device=0, lib=lib)
    fam = s.kernel_for_convex_instances(B)
    f, info, tu, tx = s.convex_solve_instances(rec, ip, want_traj=True)
    s.close()
    assert (info["status"] == 0).mean() > 0.95
    for g in range(K):
        idx = np.arange(g, B, K)
        sg = pkg.Solver(pkg.params_with(p, sets[g]), len(idx), device=0, lib=lib)
        fam_g = sg.kernel_for_batch(len(idx))
        want = sg.convex_solve(rec[idx], want_traj=True)
        sg.close()
        got = (f[idx], info[idx], tu[idx], tx[idx])
        if fam == fam_g:
            for a, b in zip(got, want):
                assert _same(a, b), g
        else:
            assert np.array_equal(got[1]["status"], want[1]["status"]), g
            assert np.abs(got[0] - want[0]).max() <= 1e-7, g
    assert np.abs(f[0::K] - f[1::K]).max() > 1e-3      # (the sets are different problems)


def test_random_records_against_the_oracle(pkg, lib, oracle):
    """256 random records at N = 20 (states config 13, records seed 11: the oracle reports every one of them OK, checked without
    a device; the cap is 5 % not-OK)."""
    B, N = 256, 20
    p = pkg.default_convex_params(N, pkg.MODE_CONVERGED, lib)
    ip = pkg.random_go1_convex_variants(B, seed=11)
    rec = pkg.random_go1_convex_states(B, config_id=13)
    s = pkg.Solver(p, B, device=0, lib=lib)
    f, info = s.convex_solve_instances(rec, ip)
    s.close()
    not_ok, worst = 0, 0.0
    for i in range(B):
        fo, io = oracle.convex_solve(pkg.params_with(p, ip[i]), rec[i:i + 1])
        assert info["status"][i] == io["status"][0], i
        if io["status"][0] == 0:
            worst = max(worst, float(np.abs(f[i] - fo[0]).max()))
        else:
            not_ok += 1
    print(f"per-instance ConvexMpc solve against the oracle: worst {worst:.2e} N, {not_ok} of {B} not OK")
    assert not_ok <= 0.05 * B
    assert worst <= 1e-6


def test_bad_records_are_flagged_alone(pkg, lib):
    B, N = 96, 20
    p = pkg.default_convex_params(N, pkg.MODE_CONVERGED, lib)
    good = pkg.random_go1_convex_variants(B, seed=5)
    rec = pkg.random_go1_convex_states(B, config_id=13)
    bad = good.copy()
    plant = {3: ("mass", np.nan), 10: ("mass", 0.0), 17: ("inertia", 0.0), 24: ("mu", 0.0), 31: ("mass", -2.0), 40: ("mu", -0.5),
             # the two fields ConvexMpc does not read are validated like the rest
             50: ("w", -1.0), 60: ("q_weights12", np.inf)}
    for i, (field, v) in plant.items():
        if field == "q_weights12":
            bad["q_weights"][i, 12] = v
        else:
            bad[field][i] = v
    s = pkg.Solver(p, B, device=0, lib=lib)
    fb, ib, tub, txb = s.convex_solve_instances(rec, bad, want_traj=True)
    fg, ig, tug, txg = s.convex_solve_instances(rec, good, want_traj=True)
    s.close()
    idx = np.array(sorted(plant))
    assert (ib["status"][idx] == pkg.BAD_PARAMS).all() and (ib["iterations"][idx] == 0).all()
    assert (fb[idx] == 0).all() and (tub[idx] == 0).all() and (txb[idx] == 0).all()
    assert (ig["status"] != pkg.BAD_PARAMS).all()
    rest = np.setdiff1d(np.arange(B), idx)
    assert _same(fb[rest], fg[rest]) and _same(ib[rest], ig[rest]) and _same(tub[rest], tug[rest]) and _same(txb[rest], txg[rest])


def test_device_entry_and_instance_independence(pkg, lib):
    import torch

    B, N = 600, 20      # variant 5 (513 ... 1024 instances)
    p = pkg.default_convex_params(N, pkg.MODE_CONVERGED, lib)
    rec = pkg.random_go1_convex_states(B, config_id=13)
    ip = pkg.random_go1_convex_variants(B, seed=17)
    s = pkg.Solver(p, B, device=0, lib=lib)
    s.set_instances_policy("auto")      # there is no lane form of this call: the policy changes nothing
    assert s.kernel_for_convex_instances(B) == "wform_ws"
    f, info = s.convex_solve_instances(rec, ip)
    d_in = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    d_ip = torch.from_numpy(ip.view(np.uint8).copy()).cuda()
    d_f = torch.full((B, 12), -1.0, dtype=torch.float64, device="cuda")
    d_info = torch.zeros(B * pkg.INFO_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    s.convex_solve_instances_device(B, d_in.data_ptr(), d_ip.data_ptr(), d_f.data_ptr(), d_info.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    assert _same(d_f.cpu().numpy(), f) and d_info.cpu().numpy().tobytes() == info.tobytes()
    perm = np.random.default_rng(1).permutation(B)
    fp, ipf = s.convex_solve_instances(rec[perm], ip[perm])
    s.close()
    assert _same(fp, f[perm]) and _same(ipf, info[perm])


def test_unsupported_handles_and_sizes(pkg, lib, monkeypatch):
    rec = pkg.random_go1_convex_states(8, config_id=13)
    pc = pkg.default_convex_params(20, pkg.MODE_CONVERGED, lib)
    for params in (pkg.default_params(10, pkg.MODE_CONVERGED, lib), pkg.default_biped8_params(16, pkg.MODE_CONVERGED, lib),
                   pkg.default_convex_params(20, pkg.MODE_REFERENCE, lib)):
        s = pkg.Solver(params, 8, device=0, lib=lib)
        assert s.query(pkg.QUERY_KERNEL_FOR_CONVEX_INSTANCES, 8) == 0 and s.kernel_for_convex_instances(8) == "none"
        assert s.convex_records() is False
        with pytest.raises(pkg.QmpcError) as e:
            s.convex_solve_instances(rec, pkg.instance_params(pc, 8))
        assert e.value.code == pkg.UNSUPPORTED
        s.close()
    s = pkg.Solver(pc, 16, device=0, lib=lib)
    with pytest.raises(pkg.QmpcError) as e:
        s.convex_solve_instances(pkg.random_go1_convex_states(17, config_id=13), pkg.instance_params(pc, 17))
    assert e.value.code == pkg.BATCH_TOO_LARGE
    before = s.query(pkg.QUERY_DEVICE_BYTES)
    s.prepare_instances()      # the buffers of qmpc_prepare_instances, on a ConvexMpc handle too
    grown = s.query(pkg.QUERY_DEVICE_BYTES) - before
    assert 760 * 16 <= grown <= 800 * 16, grown
    s.convex_solve_instances(rec, pkg.instance_params(pc, 8))
    assert s.query(pkg.QUERY_DEVICE_BYTES) - before == grown
    s.close()
    monkeypatch.setenv("QMPC_WFORM", "0")      # read by qmpc_create: no wrench-form kernel at all
    s = pkg.Solver(pc, 8, device=0, lib=lib)
    assert s.kernel_for_convex_instances(8) == "none"
    with pytest.raises(pkg.QmpcError) as e:
        s.convex_solve_instances(rec, pkg.instance_params(pc, 8))
    assert e.value.code == pkg.UNSUPPORTED
    s.close()
