"""GPU suite (-m gpu): per-instance robot and cost parameters on the lane-per-instance kernel (include/qmpc.h:
qmpc_set_instances_policy(QMPC_INSTANCES_AUTO); qmpc_lane_inst.hip, qmpc_wform_inst_list.hip).

Under AUTO a large qmpc_solve_instances* batch runs the lane kernel's passes with the seven record fields read per lane, to the
plain solve's iteration cap, and the per-instance list kernel continues the stragglers.  The default policy keeps the wave
kernels (tests/test_gpu_instance_params.py pins that).  Input sets S1 .. S4: tests/instance_lane_sets.py."""
import numpy as np
import pytest

from instance_lane_sets import BAD_RECORDS, SETS, cone_violation, input_set, plant_bad, sample

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _auto(pkg, lib, p, max_batch):
    s = pkg.Solver(p, max_batch, device=0, lib=lib)
    s.set_instances_policy("auto")
    return s


def _last(pkg, s):
    return pkg.KERNEL_FAMILY[s.query(pkg.QUERY_LAST_KERNEL)]


def _report(tag, got, want):
    """(bytes equal, status words equal, largest force difference, instances that differ) of (forces, info, ...) tuples"""
    df = np.abs(got[0] - want[0]).max(axis=1)
    same = all(_same(a, b) for a, b in zip(got, want))
    print(f"{tag}: bytes equal {same}, status equal {np.array_equal(got[1]['status'], want[1]['status'])}, "
          f"max |df| {df.max():.3e} N, differing instances {int((df > 0).sum())} of {len(df)}, "
          f"iteration counts differ on {int((got[1]['iterations'] != want[1]['iterations']).sum())}")
    return same


def test_default_policy_is_unchanged_and_auto_is_per_handle(pkg, lib):
    B = 32768
    p, rec, ip = input_set(pkg, lib, "S1")
    s = pkg.Solver(p, B, device=0, lib=lib)
    assert s.instances_policy() == "wave" and s.kernel_for_instances(B) == "wform_ws"
    small = {b: s.kernel_for_instances(b) for b in (1, 1024, 8192)}
    f0, i0 = s.solve_instances(rec, ip)
    assert _last(pkg, s) == "wform_ws"
    s.set_instances_policy("auto")
    assert s.instances_policy() == "auto" and s.kernel_for_instances(B) in ("lane_handoff", "lane")
    assert s.kernel_for_instances(B) == s.kernel_for_batch(B)
    assert {b: s.kernel_for_instances(b) for b in small} == small
    f1, i1 = s.solve_instances(rec, ip)
    assert _last(pkg, s) == s.kernel_for_instances(B)
    assert np.array_equal(i1["status"], i0["status"]) and np.abs(f1 - f0).max() < 1e-7      # two rounding families
    # below the switch-over AUTO is the wave form, bit for bit
    fs, is_ = s.solve_instances(rec[:2048], ip[:2048])
    assert _last(pkg, s) == "wform_ws"
    s.set_instances_policy("wave")
    assert s.kernel_for_instances(B) == "wform_ws"
    f2, i2 = s.solve_instances(rec, ip)
    assert _last(pkg, s) == "wform_ws" and _same(f2, f0) and _same(i2, i0)
    fw, iw = s.solve_instances(rec[:2048], ip[:2048])
    assert _same(fs, fw) and _same(is_, iw)
    with pytest.raises(pkg.QmpcError) as e:
        s.set_instances_policy(5)
    assert e.value.code == pkg.BAD_ARGUMENT and s.instances_policy() == "wave"
    s.close()


def test_refusing_handles_refuse_under_either_policy(pkg, lib, monkeypatch):
    rec = pkg.random_go1_trot_states(8, config_id=2)
    for params in (pkg.default_convex_params(20, pkg.MODE_CONVERGED, lib), pkg.default_biped8_params(16, pkg.MODE_CONVERGED, lib),
                   pkg.default_params(10, pkg.MODE_REFERENCE, lib)):
        s = _auto(pkg, lib, params, 8)
        assert s.kernel_for_instances(8) == "none"
        with pytest.raises(pkg.QmpcError) as e:
            s.solve_instances(rec, pkg.instance_params(params, 8))
        assert e.value.code == pkg.UNSUPPORTED
        s.close()
    monkeypatch.setenv("QMPC_WFORM", "0")
    p = pkg.default_params(10, pkg.MODE_CONVERGED, lib)
    s = _auto(pkg, lib, p, 8)
    assert s.kernel_for_instances(8) == "none"
    with pytest.raises(pkg.QmpcError) as e:
        s.solve_instances(rec, pkg.instance_params(p, 8))
    assert e.value.code == pkg.UNSUPPORTED
    s.close()


@pytest.mark.parametrize("name", ["S1", "S2", "S3", "S4"])
def test_auto_against_the_oracle(pkg, lib, oracle, name):
    N, B = SETS[name]
    p, rec, ip = input_set(pkg, lib, name)
    s = _auto(pkg, lib, p, B)
    assert s.kernel_for_instances(B) == "lane_handoff"
    f, info = s.solve_instances(rec, ip)
    assert _last(pkg, s) == "lane_handoff"
    s.close()
    worst = 0.0
    for i in sample(B, 128):
        fo, io = oracle.solve(pkg.params_with(p, ip[i]), rec[i:i + 1])
        assert info["status"][i] == io["status"][0], (name, int(i), int(info["status"][i]), int(io["status"][0]))
        worst = max(worst, float(np.abs(f[i] - fo[0]).max()))
    print(f"{name}: status counts {np.bincount(info['status'], minlength=7).tolist()}, mean iterations {info['iterations'].mean():.2f}, "
          f"sampled forces within {worst:.2e} N of the oracle")
    assert worst <= 1e-6
    if name == "S4":      # every instance keeps its own friction cone and force bound
        ok = info["status"] == 0
        fric, bound = cone_violation(rec, ip, f)
        assert ok.mean() > 0.9
        assert (fric[ok] <= 1e-6).all() and (bound[ok] <= 1e-6).all(), (fric[ok].max(), bound[ok].max())
        assert (fric[ok] >= -1e-6).sum() >= 10      # ... and the cone is active somewhere


@pytest.mark.parametrize("B", [32768, 65536])
def test_uniform_records_equal_the_plain_lane_solve(pkg, lib, B):
    """Pair forms (32768) and plain forms (65536), N=10: the per-lane-parameter passes against qmpc_solve on the same handle.
    Measured on the final build: forces, info and both trajectories are byte-identical."""
    p = pkg.default_params(10, pkg.MODE_CONVERGED, lib)
    rec = pkg.random_go1_trot_states(B, config_id=2)
    s = _auto(pkg, lib, p, B)
    got = s.solve_instances(rec, pkg.instance_params(p, B), want_traj=True)
    assert _last(pkg, s) == "lane_handoff"
    want = s.solve(rec, want_traj=True)
    assert _last(pkg, s) == "lane_handoff"
    s.close()
    same = _report(f"uniform records B={B}", got, want)
    assert np.array_equal(got[1]["status"], want[1]["status"]) and np.abs(got[0] - want[0]).max() < 1e-7
    assert same


def test_interleaved_groups_and_shards_equal_per_handle_lane_solves(pkg, lib):
    """Four parameter sets interleaved at 65536 instances against four plain 16384-instance solves on handles carrying the
    sets (both sides lane_handoff), and a 32768-instance shard against its block of the 65536-instance call.
    Measured on the final build: byte-identical in both comparisons."""
    B, K, N = 65536, 4, 10
    p = pkg.default_params(N, pkg.MODE_CONVERGED, lib)
    sets = pkg.random_go1_variants(K, seed=7, base=p)
    ip = sets[np.arange(B) % K]
    rec = pkg.random_go1_trot_states(B, config_id=2)
    s = _auto(pkg, lib, p, B)
    f, info, tu, tx = s.solve_instances(rec, ip, want_traj=True)
    assert _last(pkg, s) == "lane_handoff"
    shard = s.solve_instances(rec[B // 2:], ip[B // 2:], want_traj=True)
    assert _last(pkg, s) == "lane_handoff"
    s.close()
    same = _report("shard 32768 of 65536", shard, (f[B // 2:], info[B // 2:], tu[B // 2:], tx[B // 2:]))
    assert np.array_equal(shard[1]["status"], info["status"][B // 2:]) and np.abs(shard[0] - f[B // 2:]).max() < 1e-7
    for g in range(K):
        idx = np.arange(g, B, K)
        sg = pkg.Solver(pkg.params_with(p, sets[g]), len(idx), device=0, lib=lib)
        assert sg.kernel_for_batch(len(idx)) == "lane_handoff"
        want = sg.solve(rec[idx], want_traj=True)
        sg.close()
        got = (f[idx], info[idx], tu[idx], tx[idx])
        same = _report(f"group {g}", got, want) and same
        assert np.array_equal(got[1]["status"], want[1]["status"]) and np.abs(got[0] - want[0]).max() < 1e-7, g
    assert same


def test_determinism_permutation_and_device_entry(pkg, lib):
    import torch

    B = 32768
    p, rec, ip = input_set(pkg, lib, "S1")
    s = _auto(pkg, lib, p, B)
    f, info, tu, tx = s.solve_instances(rec, ip, want_traj=True)
    f2, info2, tu2, tx2 = s.solve_instances(rec, ip, want_traj=True)
    assert _same(f, f2) and _same(info, info2) and _same(tu, tu2) and _same(tx, tx2)
    perm = np.random.default_rng(1).permutation(B)
    fp, infp, tup, txp = s.solve_instances(rec[perm], ip[perm], want_traj=True)
    assert _same(fp, f[perm]) and _same(infp, info[perm]) and _same(tup, tu[perm]) and _same(txp, tx[perm])
    d_in = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    d_ip = torch.from_numpy(ip.view(np.uint8).copy()).cuda()
    d_f = torch.full((B, 12), -1.0, dtype=torch.float64, device="cuda")
    d_info = torch.zeros(B * pkg.INFO_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    s.solve_instances_device(B, d_in.data_ptr(), d_ip.data_ptr(), d_f.data_ptr(), d_info.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    assert _last(pkg, s) == "lane_handoff"
    assert _same(d_f.cpu().numpy(), f) and d_info.cpu().numpy().tobytes() == info.tobytes()
    s.close()


def test_bad_records_are_flagged_alone(pkg, lib):
    B, N = 32768, 10
    p, rec, good = input_set(pkg, lib, "S1")
    # the ten cases, and one at an index the stance sort moves: the sort groups the batch by stance mask in ascending order,
    # and this instance's own index lies outside the positions of its group
    con = (rec["contacts"] != 0).astype(int) @ (1 << np.arange(4))
    start = {k: int((con < k).sum()) for k in np.unique(con)}
    outside = [b for b in range(100, B) if not (start[con[b]] <= b < start[con[b]] + int((con == con[b]).sum()))]
    assert outside
    moved = outside[0]
    plant = dict(BAD_RECORDS)
    plant[moved] = ("mass", -2.0)
    s = _auto(pkg, lib, p, B)
    fb, ib, tub, txb = s.solve_instances(rec, plant_bad(good, plant), want_traj=True)
    assert _last(pkg, s) == "lane_handoff"
    fg, ig, tug, txg = s.solve_instances(rec, good, want_traj=True)
    cap = s.query(pkg.QUERY_LANE_CAP, 1)
    s.close()
    idx = np.array(sorted(plant))
    assert (ib["status"][idx] == pkg.BAD_PARAMS).all() and (ib["iterations"][idx] == 0).all()
    assert (fb[idx] == 0).all() and (tub[idx] == 0).all() and (txb[idx] == 0).all()
    assert (ig["status"] != pkg.BAD_PARAMS).all()
    rest = np.setdiff1d(np.arange(B), idx)
    assert _same(fb[rest], fg[rest]) and _same(ib[rest], ig[rest]) and _same(tub[rest], tug[rest]) and _same(txb[rest], txg[rest])
    # the instances handed over (those that ran beyond the cap) are the same in both calls
    assert cap > 0 and (ig["iterations"] > cap).sum() > 0
    assert np.array_equal(ib["iterations"][rest] > cap, ig["iterations"][rest] > cap)


@pytest.mark.parametrize("B", [1, 65, 4096])
def test_small_batches_through_the_lane_kernel(pkg, lib, monkeypatch, B):
    """QMPC_VARIANT=4: the pure lane kernel at every size -- tail wavefronts, and pair mode with one instance."""
    p = pkg.default_params(10, pkg.MODE_CONVERGED, lib)
    rec = np.concatenate([pkg.go1_stand_input(), pkg.random_go1_trot_states(B - 1, config_id=2)]) if B > 1 else pkg.go1_stand_input()
    ip = pkg.random_go1_variants(B, seed=19, base=p)
    if B > 8:
        rec["contacts"][3] = 0.0
        rec["quat"][6, 0] = np.inf
        ip["mu"][5] = -1.0
    sw = pkg.Solver(p, B, device=0, lib=lib)
    fw, iw, tuw, txw = sw.solve_instances(rec, ip, want_traj=True)
    sw.close()
    monkeypatch.setenv("QMPC_VARIANT", "4")
    s = _auto(pkg, lib, p, B)
    assert s.kernel_for_instances(B) == "lane"
    f, info, tu, tx = s.solve_instances(rec, ip, want_traj=True)
    assert _last(pkg, s) == "lane"
    s.close()
    assert np.array_equal(info["status"], iw["status"])
    assert np.abs(f - fw).max() < 1e-7
    if B > 8:
        assert info["status"][3] == pkg.NO_CONTACT and info["status"][6] == pkg.NAN_INPUT and info["status"][5] == pkg.BAD_PARAMS
        assert (f[5] == 0).all() and (tu[5] == 0).all() and (tx[5] == 0).all() and info["iterations"][5] == 0


def test_buffers(pkg, lib):
    B = 32768
    p, rec, ip = input_set(pkg, lib, "S1")
    s = pkg.Solver(p, B, device=0, lib=lib)
    before = s.query(pkg.QUERY_DEVICE_BYTES)
    s.prepare_instances()      # WAVE: what it always allocated
    grown = s.query(pkg.QUERY_DEVICE_BYTES) - before
    assert 760 * B <= grown <= 800 * B, grown
    s.close()
    for prepare in ("prepare_instances", "prepare"):
        s = _auto(pkg, lib, p, B)
        before = s.query(pkg.QUERY_DEVICE_BYTES)
        if prepare == "prepare":
            s.prepare(B)
        else:
            s.prepare_instances()
        ready = s.query(pkg.QUERY_DEVICE_BYTES)
        assert ready - before > 800 * B      # the lane workspace, the parameter rows and the hand-off records too
        f, info = s.solve_instances(rec, ip)
        assert _last(pkg, s) == "lane_handoff" and s.query(pkg.QUERY_DEVICE_BYTES) == ready, prepare
        assert s.query(pkg.QUERY_HANDOFF_ALLOC_FAILED) == 0
        s.close()
