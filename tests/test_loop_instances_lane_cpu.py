"""CPU suite: the lane-kernel ticks of the closed loop with per-robot controller records (qmpc_loop_run_instances* /
qmpc_loop_run_outcomes* under QMPC_INSTANCES_AUTO, include/qmpc.h) without a device.

tests/native/records_plan_host.cpp (--check loop-policy) enumerates plan_loop_instances under either policy over the planner's
whole input space; the ABI's constants and null-handle answers stay as they are."""
import ctypes as C
import subprocess
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
PLAN_SRC = HERE / "native" / "records_plan_host.cpp"
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def lib(pkg):
    import __graft_entry__ as g

    g.build_hip()
    return pkg.load_library()


def test_loop_planner_under_the_policy(tmp_path):
    exe = tmp_path / "records_plan_host"
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-o", str(exe), str(PLAN_SRC)], check=True)
    r = subprocess.run([str(exe), "--check", "loop-policy"], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "loop instance lane planner:" in r.stdout and "passed: 0 failures" in r.stdout


def test_loop_plan_abi_without_a_device(pkg, lib):
    assert (pkg.INSTANCES_WAVE, pkg.INSTANCES_AUTO, pkg.QUERY_INSTANCES_POLICY, pkg.QUERY_LOOP_INSTANCES_PLAN) == (0, 1, 10, 9)
    assert pkg.KERNEL_FAMILY[5] == "lane" and pkg.KERNEL_FAMILY[6] == "lane_handoff" and pkg.KERNEL_FAMILY[2] == "wform_ws"
    v = C.c_int64(-77)
    for arg in (20480, 20480 | (1 << 32), 20480 | (3 << 32)):
        assert lib.qmpc_query(None, pkg.QUERY_LOOP_INSTANCES_PLAN, C.c_int64(arg), C.byref(v)) == pkg.BAD_ARGUMENT and v.value == -77
    assert lib.qmpc_set_instances_policy(None, pkg.INSTANCES_AUTO) == pkg.BAD_ARGUMENT
    assert lib.qmpc_prepare(None, 20480) == pkg.BAD_ARGUMENT
    # the four loop calls that take controller records refuse a null handle before anything else
    assert lib.qmpc_loop_run_instances(None, None, 1, None, 1, None, None, None, None) == pkg.BAD_ARGUMENT
    assert lib.qmpc_loop_run_instances_device(None, None, 1, None, 1, None, None, None, None, None) == pkg.BAD_ARGUMENT
    assert lib.qmpc_loop_run_outcomes(None, None, 1, None, 1, None, None, None, None, None, None) == pkg.BAD_ARGUMENT
    assert lib.qmpc_loop_run_outcomes_device(None, None, 1, None, 1, None, None, None, None, None, None, None) == pkg.BAD_ARGUMENT
