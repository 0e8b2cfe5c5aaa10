"""CPU suite: warm-started closed loops with per-robot controller records (qmpc_set_loop_warm_records, include/qmpc.h) without
a device.

tests/native/records_plan_host.cpp (--check loop-warm) enumerates the loop planner with the opt-in setting over the planner's
whole input space; the ABI: the symbol is exported, a null handle is refused, the header and the binding agree on the query's
number, and the build's unit table carries the two new translation units."""
import ctypes as C
import re
import subprocess
from pathlib import Path

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


def test_planner_with_the_opt_in_flag(tmp_path):
    exe = tmp_path / "records_plan_host"
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-o", str(exe), str(PLAN_SRC)], check=True)
    r = subprocess.run([str(exe), "--check", "loop-warm"], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "loop warm records planner:" in r.stdout and "passed: 0 failures" in r.stdout


def test_abi_without_a_device(pkg, lib):
    assert "qmpc_set_loop_warm_records" in pkg.EXPORTED_SYMBOLS
    nm = subprocess.run(["nm", "-D", "--defined-only", str(REPO / "quaternion-mpc_amd" / "csrc" / "libqmpc_hip.so")], check=True,
                        capture_output=True, text=True).stdout
    assert re.search(r" T qmpc_set_loop_warm_records$", nm, re.M)
    # (the launchers of the two new units are hidden: not part of the C ABI)
    assert "qmpc_wform_inst_warm_launch" not in nm and "qmpc_lane_inst_warm_launch_only" not in nm
    assert lib.qmpc_set_loop_warm_records.argtypes == [C.c_void_p, C.c_int32] and lib.qmpc_set_loop_warm_records.restype == C.c_int32
    for on in (0, 1, 2, -1):
        assert lib.qmpc_set_loop_warm_records(None, on) == pkg.BAD_ARGUMENT
    v = C.c_int64(-77)
    assert lib.qmpc_query(None, pkg.QUERY_LOOP_WARM_RECORDS, C.c_int64(0), C.byref(v)) == pkg.BAD_ARGUMENT and v.value == -77
    # the six entry points the setting concerns refuse a null handle before anything else
    assert lib.qmpc_loop_run_instances(None, None, 1, None, 1, None, None, None, None) == pkg.BAD_ARGUMENT
    assert lib.qmpc_loop_run_instances_device(None, None, 1, None, 1, None, None, None, None, None) == pkg.BAD_ARGUMENT
    assert lib.qmpc_loop_run_outcomes(None, None, 1, None, 1, None, None, None, None, None, None) == pkg.BAD_ARGUMENT
    assert lib.qmpc_loop_run_outcomes_device(None, None, 1, None, 1, None, None, None, None, None, None, None) == pkg.BAD_ARGUMENT
    assert lib.qmpc_loop_run_pushes(None, None, 1, None, 1, None, None, None, None, None, None, None, 1) == pkg.BAD_ARGUMENT
    assert lib.qmpc_loop_run_pushes_device(None, None, 1, None, 1, None, None, None, None, None, None, None, 1, None) == pkg.BAD_ARGUMENT


def test_header_binding_and_unit_table_agree(pkg):
    header = (REPO / "include" / "qmpc.h").read_text()
    m = re.search(r"QMPC_QUERY_LOOP_WARM_RECORDS\s*=\s*(\d+)", header)
    assert m and int(m.group(1)) == pkg.QUERY_LOOP_WARM_RECORDS == 11
    assert re.search(r"qmpc_status\s+qmpc_set_loop_warm_records\(qmpc_handle\*\s*h,\s*int32_t\s+on\);", header)
    # the numbers the setting must not have moved
    assert (pkg.QUERY_INSTANCES_POLICY, pkg.QUERY_LOOP_INSTANCES_PLAN) == (10, 9)
    assert hasattr(pkg.Solver, "set_loop_warm_records") and hasattr(pkg.Solver, "loop_warm_records")
    import __graft_entry__ as g

    units = {n: (deps, flags) for n, deps, flags in g.hip_units()}
    csrc = REPO / "quaternion-mpc_amd" / "csrc"
    for new, twin in (("qmpc_wform_inst_warm", "qmpc_wform_inst_list"), ("qmpc_lane_inst_warm", "qmpc_lane_inst")):
        assert new in units and (csrc / (new + ".hip")).exists()
        assert units[new][1] == units[twin][1] and units[new][0] == units[twin][0]      # the twin's flags and sources
    assert csrc / "qmpc_lane_inst_warm.hip" in units["qmpc_lane"][0] and csrc / "qmpc_lane_inst_warm.hip" not in units["qmpc_wform"][0]
