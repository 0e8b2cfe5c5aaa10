"""GPU suite (-m gpu): ConvexMpc's per-instance robot and cost parameters on the lane-per-instance kernel
(qmpc_set_convex_lane_records under QMPC_INSTANCES_AUTO, include/qmpc.h; qmpc_lane_cinst.hip: qmpc_lane_cinst_kernel).

The kernel is the plain ConvexMpc lane kernel with the record's fields read per lane, so with records equal to the handle's values
it gives the bytes of qmpc_convex_solve on the lane kernel -- forces, info and both trajectories --, a mixed batch equals plain
lane solves on handles carrying each set, a shard equals its block and a permuted batch gives the permuted result.  Against the
wave family the status words are equal and the forces agree to the project's cross-family 1e-7 N, against the CPU oracle to
ConvexMpc's parity bound of 1e-6 N.

Sizes.  QMPC_LANE_CINST_MIN=1 and QMPC_LANE_MIN=1 bring both lane forms down to 1 instance, 65 (a tail across a wavefront) and
2500 (79 half-masked wavefronts).  A handle holds min(64 * ceil(max_batch / 32), 65536) resident lanes (ensure_lane_buffers); a
batch of more than half of them runs full 64-lane wavefronts, and a batch 65 beyond them sends the first wavefronts into a second
round, which rewrites their parameter rows: 32833 and 65601 instances on a handle of 65601."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


@pytest.fixture
def lane_everywhere(monkeypatch):
    monkeypatch.setenv("QMPC_LANE_CINST_MIN", "1")      # (read by qmpc_create)
    monkeypatch.setenv("QMPC_LANE_MIN", "1")


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _last(pkg, s):
    return pkg.KERNEL_FAMILY[s.query(pkg.QUERY_LAST_KERNEL)]


def _lane_solver(pkg, lib, p, B):
    s = pkg.Solver(p, B, device=0, lib=lib)
    s.set_instances_policy("auto")
    s.set_convex_lane_records(True)
    return s


def _resident_lanes(max_batch):
    return min(64 * ((max_batch + 31) // 32), 65536)


def test_the_lane_form_is_opt_in(pkg, lib, monkeypatch):
    monkeypatch.setenv("QMPC_LANE_CINST_MIN", "1000")
    B, S, N = 2500, 600, 10
    p = pkg.default_convex_params(N, pkg.MODE_CONVERGED, lib)
    rec = pkg.random_go1_convex_states(B, config_id=13)
    ip = pkg.random_go1_convex_variants(B, seed=17)
    s = pkg.Solver(p, B, device=0, lib=lib)
    assert s.convex_lane_records() is False and s.query(pkg.QUERY_CONVEX_LANE_RECORDS) == 0
    wave_family = s.kernel_for_convex_instances(B)
    assert wave_family.startswith("wform")
    w0 = s.convex_solve_instances(rec, ip, want_traj=True)
    assert _last(pkg, s) == wave_family
    ws = s.convex_solve_instances(rec[:S], ip[:S], want_traj=True)
    # without the setting AUTO gives today's kernel and bytes
    s.set_instances_policy("auto")
    assert s.kernel_for_convex_instances(B) == wave_family
    a = s.convex_solve_instances(rec, ip, want_traj=True)
    assert _last(pkg, s) == wave_family and all(_same(x, y) for x, y in zip(a, w0))
    # with it the query and the last kernel say lane from the switch-over on
    s.set_convex_lane_records(True)
    assert s.convex_lane_records() is True
    assert s.kernel_for_convex_instances(B) == "lane" and s.kernel_for_convex_instances(1000) == "lane"
    assert s.kernel_for_convex_instances(999).startswith("wform") and s.kernel_for_convex_instances(S).startswith("wform")
    lane = s.convex_solve_instances(rec, ip, want_traj=True)
    assert _last(pkg, s) == "lane"
    # ... another rounding family: status words equal, forces within the cross-family bound
    err = np.abs(lane[0] - w0[0]).max()
    print(f"lane against wave form, {B} random records: max |df| {err:.2e} N, statuses {np.unique(lane[1]['status']).tolist()}")
    assert np.array_equal(lane[1]["status"], w0[1]["status"]) and (lane[1]["status"] == pkg.OK).mean() > 0.95
    assert err <= 1e-7
    # below the switch-over the wave form, bit for bit
    b = s.convex_solve_instances(rec[:S], ip[:S], want_traj=True)
    assert _last(pkg, s).startswith("wform") and all(_same(x, y) for x, y in zip(b, ws))
    # the policy still decides
    s.set_instances_policy("wave")
    assert s.kernel_for_convex_instances(B) == wave_family
    s.set_instances_policy("auto")
    assert s.kernel_for_convex_instances(B) == "lane"
    # switching off restores the old behaviour
    s.set_convex_lane_records(False)
    assert s.convex_lane_records() is False and s.kernel_for_convex_instances(B) == wave_family
    c = s.convex_solve_instances(rec, ip, want_traj=True)
    assert _last(pkg, s) == wave_family and all(_same(x, y) for x, y in zip(c, w0))
    for bad in (2, -1):
        assert lib.qmpc_set_convex_lane_records(s._h, bad) == pkg.BAD_ARGUMENT
    s.close()
    # the setting does nothing on a handle of another model
    pq = pkg.default_params(10, pkg.MODE_CONVERGED, lib)
    sq = pkg.Solver(pq, 64, device=0, lib=lib)
    sq.set_instances_policy("auto")
    before = (sq.kernel_for_instances(64), sq.kernel_for_convex_instances(64), sq.loop_instances_plan(64, True, False))
    sq.set_convex_lane_records(True)
    assert before == (sq.kernel_for_instances(64), sq.kernel_for_convex_instances(64), sq.loop_instances_plan(64, True, False))
    sq.close()


@pytest.mark.parametrize("N,B,max_batch", [(10, 1, 1), (10, 65, 65), (10, 2500, 2500), (10, "half", 65601), (10, "beyond", 65601),
                                           (20, 2500, 2500)])
def test_uniform_records_equal_the_plain_lane_solve(pkg, lib, lane_everywhere, N, B, max_batch):
    lanes = _resident_lanes(max_batch)
    if B == "half":
        B = lanes // 2 + 65          # full 64-lane wavefronts
    elif B == "beyond":
        B = lanes + 65               # the first wavefronts take a second round
    p = pkg.default_convex_params(N, pkg.MODE_CONVERGED, lib)
    rec = pkg.random_go1_convex_states(B, config_id=13)
    s = _lane_solver(pkg, lib, p, max_batch)
    assert s.kernel_for_convex_instances(B) == "lane" and s.kernel_for_batch(B) == "lane"
    fi, ii, tui, txi = s.convex_solve_instances(rec, pkg.instance_params(p, B), want_traj=True)
    assert _last(pkg, s) == "lane"
    fp, ip, tup, txp = s.convex_solve(rec, want_traj=True)
    assert _last(pkg, s) == "lane"
    s.close()
    assert txi.shape == (B, N + 1, 12)
    assert (ii["status"] == pkg.OK).mean() > 0.95 or B == 1
    print(f"N={N} B={B} ({lanes} resident lanes): iterations mean {ii['iterations'].mean():.1f} max {ii['iterations'].max()}")
    assert _same(fi, fp) and _same(ii, ip) and _same(tui, tup) and _same(txi, txp)


def test_interleaved_parameter_sets_shards_and_permutations(pkg, lib, lane_everywhere):
    B, N, K, H = 2500, 10, 4, 1000
    p = pkg.default_convex_params(N, pkg.MODE_CONVERGED, lib)
    sets = pkg.random_go1_convex_variants(K, seed=7)
    ip = sets[np.arange(B) % K]
    rec = pkg.random_go1_convex_states(B, config_id=13)
    s = _lane_solver(pkg, lib, p, B)
    got = s.convex_solve_instances(rec, ip, want_traj=True)
    assert _last(pkg, s) == "lane"
    shard = s.convex_solve_instances(rec[:H], ip[:H], want_traj=True)
    perm = np.random.default_rng(1).permutation(B)
    shuf = s.convex_solve_instances(rec[perm], ip[perm], want_traj=True)
    assert _last(pkg, s) == "lane"
    s.close()
    assert (got[1]["status"] == pkg.OK).mean() > 0.95
    for a, b in zip(shard, got):
        assert _same(a, b[:H])
    for a, b in zip(shuf, got):
        assert _same(a, b[perm])
    for g in range(K):
        idx = np.arange(g, B, K)
        sg = pkg.Solver(pkg.params_with(p, sets[g]), len(idx), device=0, lib=lib)
        want = sg.convex_solve(rec[idx], want_traj=True)
        assert _last(pkg, sg) == "lane"
        sg.close()
        for a, b in zip(got, want):
            assert _same(a[idx], b), g
    assert np.abs(got[0][0::K] - got[0][1::K]).max() > 1e-3      # (the sets are different problems)


def test_random_records_against_the_oracle(pkg, lib, oracle, lane_everywhere):
    B, N = 2500, 10
    p = pkg.default_convex_params(N, pkg.MODE_CONVERGED, lib)
    ip = pkg.random_go1_convex_variants(B, seed=11)
    rec = pkg.random_go1_convex_states(B, config_id=13)
    s = _lane_solver(pkg, lib, p, B)
    f, info = s.convex_solve_instances(rec, ip)
    assert _last(pkg, s) == "lane"
    s.close()
    idx = np.unique(np.linspace(0, B - 1, 128).astype(int))
    assert len(idx) == 128
    worst, not_ok = 0.0, 0
    for i in idx:
        fo, io = oracle.convex_solve(pkg.params_with(p, ip[i]), rec[i:i + 1])
        assert info["status"][i] == io["status"][0], i
        if io["status"][0] == pkg.OK:
            worst = max(worst, float(np.abs(f[i] - fo[0]).max()))
        else:
            not_ok += 1
    print(f"lane form against the oracle on {len(idx)} samples: worst {worst:.2e} N, {not_ok} not OK")
    assert not_ok <= 0.05 * len(idx)
    assert worst <= 1e-6
    # every converged instance keeps its own cone and force bound (world-frame forces)
    ok = info["status"] == pkg.OK
    fw = f.reshape(B, 4, 3)
    stance = rec["contacts"] > 0
    mu = ip["mu"][:, None]
    fric = np.maximum.reduce([fw[..., 0] - mu * fw[..., 2], -fw[..., 0] - mu * fw[..., 2], fw[..., 1] - mu * fw[..., 2],
                              -fw[..., 1] - mu * fw[..., 2]])
    bound = fw[..., 2] - ip["fz_max"][:, None]
    sel = ok[:, None] & stance
    print(f"cone excess {fric[sel].max():.2e} N, force bound excess {bound[sel].max():.2e} N over {int(ok.sum())} converged instances")
    assert ok.mean() > 0.95 and (fric[sel] <= 1e-6).all() and (bound[sel] <= 1e-6).all()


def test_bad_records_and_a_nan_record_are_flagged_alone(pkg, lib, lane_everywhere):
    B, N = 200, 10
    p = pkg.default_convex_params(N, pkg.MODE_CONVERGED, lib)
    good = pkg.random_go1_convex_variants(B, seed=5)
    rec = pkg.random_go1_convex_states(B, config_id=13)
    rec["euler"][70, 0] = np.nan
    bad = good.copy()
    plant = {3: ("mass", np.nan), 10: ("mass", 0.0), 17: ("inertia", 0.0), 24: ("mu", 0.0), 31: ("mass", -2.0), 40: ("mu", -0.5),
             50: ("w", -1.0), 60: ("q_weights12", np.inf), 199: ("fz_max", -1.0)}
    for i, (field, v) in plant.items():
        if field == "q_weights12":
            bad["q_weights"][i, 12] = v
        else:
            bad[field][i] = v
    s = _lane_solver(pkg, lib, p, B)
    fb, ib, tub, txb = s.convex_solve_instances(rec, bad, want_traj=True)
    assert _last(pkg, s) == "lane"
    fg, ig, tug, txg = s.convex_solve_instances(rec, good, want_traj=True)
    s.close()
    idx = np.array(sorted(plant))
    assert (ib["status"][idx] == pkg.BAD_PARAMS).all() and (ib["iterations"][idx] == 0).all()
    assert txb.shape == (B, N + 1, 12) and tub.shape == (B, N, 12)
    assert (fb[idx] == 0).all() and (tub[idx] == 0).all() and (txb[idx] == 0).all()
    assert (ig["status"] != pkg.BAD_PARAMS).all()
    assert ib["status"][70] == ig["status"][70] == pkg.NAN_INPUT
    rest = np.setdiff1d(np.arange(B), idx)
    assert (ib["status"][np.setdiff1d(rest, [70])] == pkg.OK).mean() > 0.95
    assert _same(fb[rest], fg[rest]) and _same(ib[rest], ig[rest]) and _same(tub[rest], tug[rest]) and _same(txb[rest], txg[rest])


def test_device_entry_and_prepared_buffers(pkg, lib, lane_everywhere):
    import torch

    B, N = 2500, 10
    p = pkg.default_convex_params(N, pkg.MODE_CONVERGED, lib)
    rec = pkg.random_go1_convex_states(B, config_id=13)
    ip = pkg.random_go1_convex_variants(B, seed=19)
    s = _lane_solver(pkg, lib, p, B)
    before = s.query(pkg.QUERY_DEVICE_BYTES)
    s.prepare_instances()      # the lane workspace, the sort scratch and the parameter rows too: a capture allocates nothing
    held = s.query(pkg.QUERY_DEVICE_BYTES)
    assert held - before >= 760 * B + 312 * _resident_lanes(B)
    d_in = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    d_ip = torch.from_numpy(ip.view(np.uint8).copy()).cuda()
    d_f = torch.full((B, 12), -1.0, dtype=torch.float64, device="cuda")
    d_info = torch.zeros(B * pkg.INFO_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    s.convex_solve_instances_device(B, d_in.data_ptr(), d_ip.data_ptr(), d_f.data_ptr(), d_info.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    assert _last(pkg, s) == "lane" and s.query(pkg.QUERY_DEVICE_BYTES) == held
    f, info = s.convex_solve_instances(rec, ip)
    assert s.query(pkg.QUERY_DEVICE_BYTES) == held
    s.close()
    assert _same(d_f.cpu().numpy(), f) and d_info.cpu().numpy().tobytes() == info.tobytes()
    # a handle that did not opt in prepares what it always did
    w = pkg.Solver(p, B, device=0, lib=lib)
    w.set_instances_policy("auto")
    b0 = w.query(pkg.QUERY_DEVICE_BYTES)
    w.prepare_instances()
    grown = w.query(pkg.QUERY_DEVICE_BYTES) - b0
    w.close()
    assert 760 * B <= grown <= 800 * B, grown
