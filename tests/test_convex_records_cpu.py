"""CPU suite: per-robot controller and plant records for ConvexMpc solves and loops (qmpc_convex_solve_instances*,
qmpc_set_convex_records; include/qmpc.h) without a device.

tests/native/records_plan_host.cpp (--check convex) enumerates plan_convex_instances and the loop planner under the setting over
the planner's whole input space; the ABI: the symbols are exported, a null handle is refused, the header and the binding agree
on the queries' numbers, the build's unit table carries the two new translation units, the record generator of the fleet
under the sibling controller, and the oracle's own not-OK rate on the sample of the GPU parity test.  What needs a handle -- the
setting defaults to 0 and the query reads it back, the new query answers 0 on a QuatMpc handle -- is asserted in the GPU suite
(tests/test_gpu_convex_records.py, tests/test_gpu_convex_instances.py): no handle exists without a device."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
PLAN_SRC = HERE / "native" / "records_plan_host.cpp"
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def lib(pkg):
    import __graft_entry__ as g

    g.build_hip()
    return pkg.load_library()


def test_planner_of_the_convex_calls(tmp_path):
    exe = tmp_path / "records_plan_host"
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-o", str(exe), str(PLAN_SRC)], check=True)
    r = subprocess.run([str(exe), "--check", "convex"], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "convex records planner:" in r.stdout and "passed: 0 failures" in r.stdout
    # the batches the GPU tests run at (tests/test_gpu_convex_instances.py, tests/test_gpu_convex_records.py)
    assert "N=10: smallest enumerated batch on variant 3: 1, 5: 769, 6: 2049" in r.stdout
    assert "N=20: smallest enumerated batch on variant 3: 1, 5: 513, 6: 1025" in r.stdout


def test_abi_without_a_device(pkg, lib):
    new = ("qmpc_convex_solve_instances", "qmpc_convex_solve_instances_device", "qmpc_set_convex_records")
    nm = subprocess.run(["nm", "-D", "--defined-only", str(REPO / "quaternion-mpc_amd" / "csrc" / "libqmpc_hip.so")], check=True,
                        capture_output=True, text=True).stdout
    for sym in new:
        assert sym in pkg.EXPORTED_SYMBOLS and re.search(r" T " + sym + r"$", nm, re.M), sym
    # (the launchers of the two new units are hidden: not part of the C ABI)
    assert "qmpc_wform_cinst_solve_launch" not in nm and "rec_fused_launch" not in nm
    rec = np.zeros(4, dtype=pkg.CONVEX_INPUT_DTYPE)
    ip = np.zeros(4, dtype=pkg.INSTANCE_PARAMS_DTYPE)
    f = np.zeros((4, 12))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    assert lib.qmpc_convex_solve_instances(None, 4, vp(rec), vp(ip), vp(f), None, None, None) == pkg.BAD_ARGUMENT
    assert lib.qmpc_convex_solve_instances_device(None, 4, vp(rec), vp(ip), vp(f), None, None) == pkg.BAD_ARGUMENT
    assert lib.qmpc_set_convex_records.argtypes == [C.c_void_p, C.c_int32] and lib.qmpc_set_convex_records.restype == C.c_int32
    for on in (0, 1, 2, -1):
        assert lib.qmpc_set_convex_records(None, on) == pkg.BAD_ARGUMENT
    for q in (pkg.QUERY_CONVEX_RECORDS, pkg.QUERY_KERNEL_FOR_CONVEX_INSTANCES):
        v = C.c_int64(-77)
        assert lib.qmpc_query(None, q, C.c_int64(4), C.byref(v)) == pkg.BAD_ARGUMENT and v.value == -77


def test_header_binding_and_unit_table_agree(pkg):
    header = (REPO / "include" / "qmpc.h").read_text()
    m = re.search(r"QMPC_QUERY_KERNEL_FOR_CONVEX_INSTANCES\s*=\s*(\d+)", header)
    assert m and int(m.group(1)) == pkg.QUERY_KERNEL_FOR_CONVEX_INSTANCES == 12
    m = re.search(r"QMPC_QUERY_CONVEX_RECORDS\s*=\s*(\d+)", header)
    assert m and int(m.group(1)) == pkg.QUERY_CONVEX_RECORDS == 13
    assert re.search(r"qmpc_status\s+qmpc_set_convex_records\(qmpc_handle\*\s*h,\s*int32_t\s+on\);", header)
    assert re.search(r"qmpc_status\s+qmpc_convex_solve_instances\(qmpc_handle\*\s*h,\s*int32_t\s+batch,\s*const\s+qmpc_convex_input\*\s*in,", header)
    assert re.search(r"qmpc_status\s+qmpc_convex_solve_instances_device\(", header)
    # the numbers the new values must not have moved
    assert (pkg.QUERY_LOOP_WARM_RECORDS, pkg.QUERY_INSTANCES_POLICY, pkg.QUERY_LOOP_INSTANCES_PLAN, pkg.QUERY_KERNEL_FOR_INSTANCES) == (11, 10, 9, 8)
    for name in ("convex_solve_instances", "convex_solve_instances_device", "set_convex_records", "convex_records",
                 "kernel_for_convex_instances"):
        assert hasattr(pkg.Solver, name), name
    import __graft_entry__ as g

    units = {n: (deps, flags) for n, deps, flags in g.hip_units()}
    csrc = REPO / "quaternion-mpc_amd" / "csrc"
    for new, twin in (("qmpc_wform_cinst", "qmpc_wform"), ("qmpc_loop_crec", "qmpc_loop_push")):
        assert new in units and (csrc / (new + ".hip")).exists()
        assert units[new][1] == units[twin][1] and units[new][0] == units[twin][0]      # the twin's flags and sources
    # the loops' unit is the shared text once more, not a copy of it
    text = (csrc / "qmpc_loop_crec.hip").read_text()
    assert '#include "qmpc_loop_rec.inc"' in text and "#define QMPC_REC_CONVEX" in text and "#define QMPC_REC_EXT 2" in text
    assert "__global__" not in text


def test_random_go1_convex_variants(lib, pkg):
    a = pkg.random_go1_convex_variants(300, seed=3)
    assert a.dtype == pkg.INSTANCE_PARAMS_DTYPE and a.shape == (300,)
    # counter-based: instance i does not depend on the batch it is drawn in
    assert a[200:].tobytes() == pkg.random_go1_convex_variants(100, seed=3, first=200).tobytes()
    assert pkg.random_go1_convex_variants(300, seed=4).tobytes() != a.tobytes()
    base = pkg.default_convex_params(10, pkg.MODE_CONVERGED, lib)
    q = pkg.random_go1_variants(300, seed=3)
    # one fleet under both controllers: the robots' mass, friction and force bound are those of random_go1_variants
    assert np.array_equal(a["mass"], q["mass"]) and np.array_equal(a["mu"], q["mu"]) and np.array_equal(a["fz_max"], q["fz_max"])
    assert (a["mass"] >= 10).all() and (a["mass"] <= 16).all() and (a["mu"] >= 0.3).all() and (a["mu"] <= 0.9).all()
    nz = np.asarray(base.q_weights[:]) != 0
    qs = a["q_weights"][:, nz] / np.asarray(base.q_weights[:])[None, nz]
    rs = a["r_weights"] / np.asarray(base.r_weights[:])[None]
    assert (a["q_weights"][:, ~nz] == 0).all() and (a["w"] == base.w).all()
    assert np.allclose(qs, qs[:, :1]) and (qs >= 0.5).all() and (qs <= 2).all()
    assert np.allclose(rs, rs[:, :1]) and (rs >= 0.5).all() and (rs <= 2).all()
    I = a["inertia"].reshape(-1, 3, 3)
    assert np.array_equal(I, I.transpose(0, 2, 1)) and (np.linalg.eigvalsh(I) > 0).all()
    ratio = np.diagonal(I, axis1=1, axis2=2) / np.diag(np.asarray(base.inertia[:]).reshape(3, 3))[None]
    per_axis = ratio / (a["mass"] / base.mass)[:, None]
    assert (per_axis >= 0.8 - 1e-12).all() and (per_axis <= 1.2 + 1e-12).all()
    # every record is valid, and params_with puts it on a ConvexMpc handle
    p = pkg.params_with(base, a[7])
    assert p.model == base.model and p.mass == a["mass"][7] and p.mu == a["mu"][7]


def test_the_oracle_alone_stays_within_the_not_ok_cap(pkg, lib, oracle):
    """The sample of tests/test_gpu_convex_instances.py::test_random_records_against_the_oracle (256 records at N = 20, states
    config 13, records seed 11): at most 5 % of it may be not OK for the oracle, whatever the device does."""
    B, N = 256, 20
    p = pkg.default_convex_params(N, pkg.MODE_CONVERGED, lib)
    ip = pkg.random_go1_convex_variants(B, seed=11)
    rec = pkg.random_go1_convex_states(B, config_id=13)
    status = np.array([int(oracle.convex_solve(pkg.params_with(p, ip[i]), rec[i:i + 1])[1]["status"][0]) for i in range(B)])
    print(f"oracle alone: {(status != 0).sum()} of {B} not OK")
    assert (status != 0).sum() <= 0.05 * B
