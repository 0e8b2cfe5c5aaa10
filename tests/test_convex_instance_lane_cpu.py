"""CPU suite: ConvexMpc's per-instance robot and cost parameters on the lane-per-instance kernel (qmpc_set_convex_lane_records
under QMPC_INSTANCES_AUTO, include/qmpc.h) without a device.

tests/native/lane_cinst_host.cpp is a g++ build of the lane core's per-lane-parameter instantiation for ConvexMpc's model (the
text hipcc compiles into qmpc_lane_cinst_kernel): the instance fields of the parameters come from the lane's rows of a parameter
block, everything else from the handle's block.  Host arithmetic uses the same expressions whatever the source, so its results
must equal, byte for byte, the plain core's on a handle that carries the instance's values -- a difference is a field read from
the wrong place.  tests/native/convex_lane_plan_host.cpp enumerates the planner with the setting off and on."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
SRC = HERE / "native" / "lane_cinst_host.cpp"
LIB = HERE / "native" / "liblane_cinst_host.so"
PLAN_SRC = HERE / "native" / "convex_lane_plan_host.cpp"
CORE = REPO / "quaternion-mpc_amd" / "csrc"
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def lib(pkg):
    import __graft_entry__ as g

    g.build_hip()
    return pkg.load_library()


@pytest.fixture(scope="module")
def host(pkg):
    deps = [SRC, CORE / "qmpc_lane_core.h", CORE / "qmpc_params_dev.h", REPO / "include" / "qmpc.h"]
    if not LIB.exists() or any(LIB.stat().st_mtime < d.stat().st_mtime for d in deps):
        # no contraction: the oracle is compiled without it as well
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas",
                        "-o", str(LIB), str(SRC)], check=True)
    h = C.CDLL(str(LIB))
    h.lane_host_convex_solve.restype = C.c_int
    h.lane_host_convex_solve_instances.restype = C.c_int
    vp = C.c_void_p

    class Host:
        @staticmethod
        def solve(p, rec):
            rec = np.ascontiguousarray(rec)
            B = rec.shape[0]
            f = np.zeros((B, 12))
            info = np.zeros(B, dtype=pkg.INFO_DTYPE)
            rc = h.lane_host_convex_solve(C.byref(p), B, rec.ctypes.data_as(vp), f.ctypes.data_as(vp), info.ctypes.data_as(vp))
            assert rc == 0, rc
            return f, info

        @staticmethod
        def solve_instances(p, rec, ip):
            rec, ip = np.ascontiguousarray(rec), np.ascontiguousarray(ip)
            B = rec.shape[0]
            assert ip.shape[0] == B and ip.dtype == pkg.INSTANCE_PARAMS_DTYPE
            f = np.full((B, 12), np.nan)
            info = np.zeros(B, dtype=pkg.INFO_DTYPE)
            rc = h.lane_host_convex_solve_instances(C.byref(p), B, rec.ctypes.data_as(vp), ip.ctypes.data_as(vp), f.ctypes.data_as(vp),
                                                    info.ctypes.data_as(vp))
            assert rc == 0, rc
            return f, info

    return Host


@pytest.mark.parametrize("N", [10, 20])
def test_uniform_records_equal_the_plain_core(pkg, lib, host, N):
    p = pkg.default_convex_params(N, pkg.MODE_CONVERGED, lib)
    rec = pkg.random_go1_convex_states(256, config_id=13)
    rec["contacts"][3] = 0.0
    rec["euler"][6, 0] = np.inf
    f, info = host.solve_instances(p, rec, pkg.instance_params(p, len(rec)))
    fp, ip = host.solve(p, rec)
    assert info["status"][3] == pkg.NO_CONTACT and info["status"][6] == pkg.NAN_INPUT
    assert (info["status"] == pkg.OK).sum() >= 250
    assert f.tobytes() == fp.tobytes() and info.tobytes() == ip.tobytes()


@pytest.mark.parametrize("N", [10, 20])
def test_random_variants_equal_per_handle_solves_and_the_oracle(pkg, lib, oracle, host, N):
    B = 256
    p = pkg.default_convex_params(N, pkg.MODE_CONVERGED, lib)
    rec = pkg.random_go1_convex_states(B, config_id=13)
    ip = pkg.random_go1_convex_variants(B, seed=17)
    f, info = host.solve_instances(p, rec, ip)
    assert (info["status"] == pkg.OK).all()
    sampled = set(np.unique(np.linspace(0, B - 1, 32).astype(int)).tolist())
    worst = 0.0
    for i in range(B):
        pi = pkg.params_with(p, ip[i])
        f1, i1 = host.solve(pi, rec[i:i + 1])
        assert f[i].tobytes() == f1[0].tobytes() and info[i:i + 1].tobytes() == i1.tobytes(), i
        if i in sampled:      # sampled instances against the oracle's ConvexMpc solve
            fo, io = oracle.convex_solve(pi, rec[i:i + 1])
            assert info["status"][i] == io["status"][0], i
            worst = max(worst, float(np.abs(f[i] - fo[0]).max()))
    print(f"N={N}: {len(sampled)} samples within {worst:.2e} N of the oracle; iterations mean {info['iterations'].mean():.1f} "
          f"max {info['iterations'].max()}")
    assert worst <= 1e-6


def test_the_handles_own_physics_are_ignored(pkg, lib, host):
    """Every instance field comes from the lane's rows: a handle with another robot gives the same bytes."""
    go1 = pkg.default_convex_params(10, pkg.MODE_CONVERGED, lib)
    heavy = go1.copy()
    heavy.mass, heavy.mu, heavy.fz_max = 30.0, 0.2, 500.0
    for k in range(9):
        heavy.inertia[k] *= 3.0
    for k in range(13):
        heavy.q_weights[k] *= 2.0
    for k in range(12):
        heavy.r_weights[k] *= 5.0
    rec = pkg.random_go1_convex_states(128, config_id=13)
    ip = pkg.random_go1_convex_variants(128, seed=7)
    fa, ia = host.solve_instances(go1, rec, ip)
    fb, ib = host.solve_instances(heavy, rec, ip)
    assert fa.tobytes() == fb.tobytes() and ia.tobytes() == ib.tobytes()
    fh, _ = host.solve(heavy, rec)
    assert np.abs(fh - fa).max() > 1.0


def test_bad_records_are_flagged_alone(pkg, lib, host):
    B = 128
    p = pkg.default_convex_params(10, pkg.MODE_CONVERGED, lib)
    good = pkg.random_go1_convex_variants(B, seed=5)
    rec = pkg.random_go1_convex_states(B, config_id=13)
    bad = good.copy()
    plant = {3: ("mass", np.nan), 10: ("mass", 0.0), 17: ("inertia", 0.0), 24: ("mu", 0.0), 31: ("mass", -2.0), 40: ("mu", -0.5),
             50: ("w", -1.0), 60: ("fz_max", np.nan)}
    for i, (field, v) in plant.items():
        bad[field][i] = v
    fb, ib = host.solve_instances(p, rec, bad)
    fg, ig = host.solve_instances(p, rec, good)
    idx = np.array(sorted(plant))
    assert (ib["status"][idx] == pkg.BAD_PARAMS).all() and (ib["iterations"][idx] == 0).all() and (fb[idx] == 0).all()
    assert (ig["status"] != pkg.BAD_PARAMS).all()
    rest = np.setdiff1d(np.arange(B), idx)
    assert fb[rest].tobytes() == fg[rest].tobytes() and ib[rest].tobytes() == ig[rest].tobytes()


def test_planner_with_the_setting_off_and_on(tmp_path):
    exe = tmp_path / "convex_lane_plan_host"
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-o", str(exe), str(PLAN_SRC)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr
    assert "convex lane planner:" in r.stdout and "passed: 0 failures" in r.stdout
    m = re.search(r"lane plans seen: solves (\d+), loop ticks (\d+)", r.stdout)
    assert m and int(m.group(1)) > 0 and int(m.group(2)) > 0


def test_abi_without_a_device(pkg, lib):
    header = (REPO / "include" / "qmpc.h").read_text()
    m = re.search(r"QMPC_QUERY_CONVEX_LANE_RECORDS\s*=\s*(\d+)", header)
    assert m and int(m.group(1)) == pkg.QUERY_CONVEX_LANE_RECORDS == 14
    assert re.search(r"qmpc_status\s+qmpc_set_convex_lane_records\(qmpc_handle\*\s*h,\s*int32_t\s+on\);", header)
    assert pkg.QUERY_CONVEX_RECORDS == 13 and pkg.QUERY_KERNEL_FOR_CONVEX_INSTANCES == 12
    nm = subprocess.run(["nm", "-D", "--defined-only", str(CORE / "libqmpc_hip.so")], check=True, capture_output=True, text=True).stdout
    assert "qmpc_set_convex_lane_records" in pkg.EXPORTED_SYMBOLS and re.search(r" T qmpc_set_convex_lane_records$", nm, re.M)
    for hidden in ("qmpc_lane_cinst_launch_only", "qmpc_lane_cinst_upload_params", "qmpc_lane_cinst_sort_launch"):
        assert hidden not in nm, hidden      # (the unit's launchers are hidden: not part of the C ABI)
    assert lib.qmpc_set_convex_lane_records.argtypes == [C.c_void_p, C.c_int32] and lib.qmpc_set_convex_lane_records.restype == C.c_int32
    for on in (0, 1, 2, -1):
        assert lib.qmpc_set_convex_lane_records(None, on) == pkg.BAD_ARGUMENT
    v = C.c_int64(-77)
    assert lib.qmpc_query(None, pkg.QUERY_CONVEX_LANE_RECORDS, C.c_int64(0), C.byref(v)) == pkg.BAD_ARGUMENT and v.value == -77
    for name in ("set_convex_lane_records", "convex_lane_records"):
        assert hasattr(pkg.Solver, name), name
    import __graft_entry__ as g

    units = {n: (deps, flags) for n, deps, flags in g.hip_units()}
    assert "qmpc_lane_cinst" in units and (CORE / "qmpc_lane_cinst.hip").exists()
    assert units["qmpc_lane_cinst"] == units["qmpc_lane_inst"]      # the twin's sources and flags
