"""CPU suite: the closed loop with per-robot controller and plant records (qmpc_loop_run_instances*, include/qmpc.h) without
a device.

The plant record's ABI, the call-level argument checks that need no handle, tests/native/loop_instances_host.cpp: the
plant validity rule and the disturbed plant step against the plain one (bit for bit with a zero disturbance), and the planner
rule of the call over the planner's input space (tests/native/records_plan_host.cpp --check loop).  The harnesses are compiled
host-only by hipcc, like tests/native/instance_host.cpp."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
SRC = HERE / "native" / "loop_instances_host.cpp"
PLAN_SRC = HERE / "native" / "records_plan_host.cpp"
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def lib(pkg):
    import __graft_entry__ as g

    g.build_hip()
    return pkg.load_library()


def test_plant_record_size(lib, pkg):
    assert lib.qmpc_sizeof_plant_params() == pkg.PLANT_PARAMS_DTYPE.itemsize == 128


def test_plant_params_from_copies_mass_and_inertia(lib, pkg):
    p = pkg.default_params(10, pkg.MODE_CONVERGED, lib)
    out = np.full(1, np.nan, dtype=pkg.PLANT_PARAMS_DTYPE)      # every byte overwritten or the comparison fails
    lib.qmpc_plant_params_from(C.byref(p), out.ctypes.data_as(C.c_void_p))
    assert out.tobytes() == pkg.plant_params(p, 1).tobytes()
    assert out["mass"][0] == p.mass and list(out["inertia"][0]) == list(p.inertia)
    assert (out["ext_force_world"] == 0).all() and (out["ext_torque_body"] == 0).all()
    assert not np.signbit(out["ext_force_world"]).any() and not np.signbit(out["ext_torque_body"]).any()
    lib.qmpc_plant_params_from(None, None)      # a no-op, not a crash


def test_null_arguments_are_rejected(lib, pkg):
    lp = pkg.default_loop_params(lib)
    st = np.zeros(2, dtype=pkg.LOOP_STATE_DTYPE)
    ctrl = np.zeros(2, dtype=pkg.INSTANCE_PARAMS_DTYPE)
    plant = np.zeros(2, dtype=pkg.PLANT_PARAMS_DTYPE)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    for f in (lib.qmpc_loop_run_instances, lib.qmpc_loop_run_instances_device):
        extra = [None] if f is lib.qmpc_loop_run_instances_device else []
        assert f(None, C.byref(lp), 2, vp(st), 5, vp(ctrl), vp(plant), None, None, *extra) == pkg.BAD_ARGUMENT
    v = C.c_int64(7)
    assert lib.qmpc_query(None, pkg.QUERY_LOOP_INSTANCES_PLAN, 4, C.byref(v)) == pkg.BAD_ARGUMENT and v.value == 7


def test_random_go1_plants(lib, pkg):
    a = pkg.random_go1_plants(300, seed=3, force=(0.0, 30.0))
    assert a.dtype == pkg.PLANT_PARAMS_DTYPE and a.shape == (300,)
    assert a[200:].tobytes() == pkg.random_go1_plants(100, seed=3, first=200, force=(0.0, 30.0)).tobytes()   # counter-based
    assert pkg.random_go1_plants(300, seed=4, force=(0.0, 30.0)).tobytes() != a.tobytes()
    base = pkg.default_params(10, pkg.MODE_CONVERGED, lib)
    assert (a["mass"] >= base.mass).all() and (a["mass"] <= base.mass + 4).all()
    I = a["inertia"].reshape(-1, 3, 3)
    assert np.array_equal(I, I.transpose(0, 2, 1)) and (np.linalg.eigvalsh(I) > 0).all()
    per_axis = np.diagonal(I, axis1=1, axis2=2) / np.diag(np.asarray(base.inertia[:]).reshape(3, 3))[None] / (a["mass"] / base.mass)[:, None]
    assert (per_axis >= 0.8 - 1e-12).all() and (per_axis <= 1.2 + 1e-12).all()
    f = a["ext_force_world"]
    mag = np.hypot(f[:, 0], f[:, 1])
    assert (f[:, 2] == 0).all() and (mag <= 30 + 1e-9).all() and mag.max() > 20
    assert (a["ext_torque_body"] == 0).all()
    assert (np.sign(f[:, 0]) > 0).any() and (np.sign(f[:, 0]) < 0).any()      # random directions
    z = pkg.random_go1_plants(10, seed=1)      # default: no disturbance
    assert (z["ext_force_world"] == 0).all()


def test_plant_rule_step_and_planner(tmp_path):
    out = ""
    for src, args in ((SRC, []), (PLAN_SRC, ["--check", "loop"])):
        exe = tmp_path / src.stem
        subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-o", str(exe), str(src)], check=True)
        r = subprocess.run([str(exe), *args], capture_output=True, text=True)
        print(r.stdout)
        assert r.returncode == 0 and "passed: 0 failures" in r.stdout, r.stdout + r.stderr
        out += r.stdout
    assert "10000 valid records equal fill_dev_params' blocks (10000)" in out
    assert "20000 of 20000 zero-disturbance steps equal plant_step" in out and "loop records planner:" in out
