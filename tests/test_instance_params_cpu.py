"""CPU suite: per-instance robot and cost parameters (qmpc_solve_instances*, include/qmpc.h) without a device.

The record's ABI (size, the seven fields qmpc_instance_params_from copies), the call-level argument checks that need no
handle, the planner rule of the per-instance call over the planner's whole input space (tests/native/records_plan_host.cpp
--check instances), and tests/native/instance_host.cpp: the shared helper of the expansion kernel against the host's
fill_dev_params, byte for byte.  The harnesses are compiled host-only by hipcc, like tests/native/plan_host.cpp."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
SRC = HERE / "native" / "instance_host.cpp"
PLAN_SRC = HERE / "native" / "records_plan_host.cpp"
CSRC = HERE.parent / "quaternion-mpc_amd" / "csrc"
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def lib(pkg):
    import __graft_entry__ as g

    g.build_hip()
    return pkg.load_library()


def test_record_size(lib, pkg):
    assert lib.qmpc_sizeof_instance_params() == pkg.INSTANCE_PARAMS_DTYPE.itemsize == 304


def test_instance_params_from_copies_the_seven_fields(lib, pkg):
    p = pkg.default_params(10, pkg.MODE_CONVERGED, lib)
    out = np.full(1, np.nan, dtype=pkg.INSTANCE_PARAMS_DTYPE)      # every byte overwritten or the comparison fails
    lib.qmpc_instance_params_from(C.byref(p), out.ctypes.data_as(C.c_void_p))
    want = pkg.instance_params(p, 1)
    assert out.tobytes() == want.tobytes()
    assert out["mass"][0] == p.mass and list(out["inertia"][0]) == list(p.inertia)
    assert out["mu"][0] == p.mu and out["fz_max"][0] == p.fz_max and out["w"][0] == p.w
    assert list(out["q_weights"][0]) == list(p.q_weights) and list(out["r_weights"][0]) == list(p.r_weights)
    # ... and params_with puts them back: the same bytes as the handle's parameters
    assert bytes(pkg.params_with(pkg.default_params(10, pkg.MODE_CONVERGED, lib), out[0])) == bytes(p)


def test_null_arguments_are_rejected(lib, pkg):
    rec = np.zeros(4, dtype=pkg.INPUT_DTYPE)
    ip = np.zeros(4, dtype=pkg.INSTANCE_PARAMS_DTYPE)
    f = np.zeros((4, 12))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    assert lib.qmpc_solve_instances(None, 4, vp(rec), vp(ip), vp(f), None, None, None) == pkg.BAD_ARGUMENT
    assert lib.qmpc_solve_instances_device(None, 4, vp(rec), vp(ip), vp(f), None, None) == pkg.BAD_ARGUMENT
    assert lib.qmpc_prepare_instances(None) == pkg.BAD_ARGUMENT
    v = C.c_int64(7)
    assert lib.qmpc_query(None, pkg.QUERY_KERNEL_FOR_INSTANCES, 4, C.byref(v)) == pkg.BAD_ARGUMENT and v.value == 7
    lib.qmpc_instance_params_from(None, None)      # a no-op, not a crash


def test_status_string(lib, pkg):
    s = lib.qmpc_status_string(pkg.BAD_PARAMS)
    assert pkg.BAD_PARAMS == 6 and s and s != lib.qmpc_status_string(99)


def test_planner_rule_and_shared_helper(tmp_path):
    for src, args, line in ((PLAN_SRC, ["--check", "instances"], "instances planner:"), (SRC, [], "10000 valid records equal")):
        exe = tmp_path / src.stem
        subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-o", str(exe), str(src)], check=True)
        r = subprocess.run([str(exe), *args], capture_output=True, text=True)
        print(r.stdout)
        assert r.returncode == 0, r.stdout + r.stderr
        assert line in r.stdout and "passed: 0 failures" in r.stdout


def test_params_header_stays_gpp_compilable(tmp_path):
    """qmpc_params_dev.h (with the helper the expansion kernel shares) is also built by g++ (tests/test_lane_core_cpu.py)."""
    src = tmp_path / "t.cpp"
    src.write_text(f'#include "{CSRC / "qmpc_params_dev.h"}"\nint main() {{ return 0; }}\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", str(src)], check=True)


def test_random_go1_variants(lib, pkg):
    a = pkg.random_go1_variants(300, seed=3)
    assert a.dtype == pkg.INSTANCE_PARAMS_DTYPE and a.shape == (300,)
    # counter-based: instance i does not depend on the batch it is drawn in
    b = pkg.random_go1_variants(100, seed=3, first=200)
    assert a[200:].tobytes() == b.tobytes()
    assert pkg.random_go1_variants(300, seed=4).tobytes() != a.tobytes()
    base = pkg.default_params(10, pkg.MODE_CONVERGED, lib)
    assert (a["mass"] >= 10).all() and (a["mass"] <= 16).all()
    assert (a["mu"] >= 0.3).all() and (a["mu"] <= 0.9).all()
    assert (a["fz_max"] >= 80).all() and (a["fz_max"] <= 200).all()
    nz = np.asarray(base.q_weights[:]) != 0
    qs = a["q_weights"][:, nz] / np.asarray(base.q_weights[:])[None, nz]
    rs = a["r_weights"] / np.asarray(base.r_weights[:])[None]
    assert (a["q_weights"][:, ~nz] == 0).all()
    assert np.allclose(qs, qs[:, :1]) and (qs >= 0.5).all() and (qs <= 2).all()
    assert np.allclose(rs, rs[:, :1]) and (rs >= 0.5).all() and (rs <= 2).all()
    assert (a["w"] == base.w).all()
    I = a["inertia"].reshape(-1, 3, 3)
    assert np.array_equal(I, I.transpose(0, 2, 1)) and (np.linalg.eigvalsh(I) > 0).all()
    ratio = np.diagonal(I, axis1=1, axis2=2) / np.diag(np.asarray(base.inertia[:]).reshape(3, 3))[None]
    per_axis = ratio / (a["mass"] / base.mass)[:, None]
    assert (per_axis >= 0.8 - 1e-12).all() and (per_axis <= 1.2 + 1e-12).all()
