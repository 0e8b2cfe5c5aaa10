"""CPU suite: the per-robot outcome records of the closed loop (qmpc_loop_run_outcomes*, include/qmpc.h) without a device.

The record's ABI, its host-side initialiser, the call-level argument checks that need no handle, summarize_outcomes, and
tests/native/loop_outcome_host.cpp: loop_outcome_one (csrc/qmpc_loop_math.h, the one source of the metric) over hand-made state
sequences.  The harness is compiled host-only by hipcc, like tests/native/loop_instances_host.cpp."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
SRC = HERE / "native" / "loop_outcome_host.cpp"
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def lib(pkg):
    import __graft_entry__ as g

    g.build_hip()
    return pkg.load_library()


def test_outcome_record_size(lib, pkg):
    assert lib.qmpc_sizeof_loop_outcome() == pkg.LOOP_OUTCOME_DTYPE.itemsize == 128
    assert C.sizeof(pkg.OutcomeParams) == 32
    names = pkg.LOOP_OUTCOME_DTYPE.names      # the field order of struct qmpc_loop_outcome
    assert names[:4] == ("ticks", "down_tick", "min_height", "min_upright") and names[-1] == "reserved"


def test_default_outcome_params(lib, pkg):
    op = pkg.OutcomeParams(7.0, 7.0, 7.0, 7.0)
    lib.qmpc_default_outcome_params(C.byref(op))
    assert (op.down_height, op.down_upright, op.stop_when_down, op.reserved) == (0.15, 0.5, 0.0, 0.0)
    assert pkg.default_outcome_params(lib, stop_when_down=True).stop_when_down == 1.0
    lib.qmpc_default_outcome_params(None)      # a no-op, not a crash


def test_outcome_init_overwrites_every_byte(lib, pkg):
    a = np.frombuffer(np.full(5 * 16, np.nan).tobytes(), dtype=pkg.LOOP_OUTCOME_DTYPE).copy()
    b = np.frombuffer(b"\xa5" * (5 * 128), dtype=pkg.LOOP_OUTCOME_DTYPE).copy()
    for x in (a, b):
        lib.qmpc_loop_outcome_init(x.ctypes.data_as(C.c_void_p), 4)
    assert a[:4].tobytes() == b[:4].tobytes() == pkg.loop_outcomes(4, lib).tobytes()
    assert np.isnan(a[4]["ticks"]) and b[4:].tobytes() == b"\xa5" * 128      # the fifth record is not the call's
    o = a[:4]
    for k in ("ticks", "sum_vel_err_sq", "not_ok_ticks", "rejected_ticks", "iterations_sum"):
        assert (o[k] == 0).all() and not np.signbit(o[k]).any(), k
    assert (o["reserved"] == 0).all() and not np.signbit(o["reserved"]).any()
    assert (o["down_tick"] == -1).all() and (o["first_rejected_tick"] == -1).all()
    assert (o["min_height"] == np.inf).all() and (o["min_upright"] == np.inf).all()
    for k in ("max_height_err", "max_vel_err", "max_ang_vel", "max_force_z", "iterations_max"):
        assert (o[k] == -np.inf).all(), k
    lib.qmpc_loop_outcome_init(None, 3)      # a no-op, not a crash


def test_null_arguments_are_rejected(lib, pkg):
    lp = pkg.default_loop_params(lib)
    op = pkg.default_outcome_params(lib)
    st = np.zeros(2, dtype=pkg.LOOP_STATE_DTYPE)
    oc = pkg.loop_outcomes(2, lib)
    plant = np.zeros(2, dtype=pkg.PLANT_PARAMS_DTYPE)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    fake = C.c_void_p(8)      # never dereferenced: the null checks come first
    for f in (lib.qmpc_loop_run_outcomes, lib.qmpc_loop_run_outcomes_device):
        extra = [None] if f is lib.qmpc_loop_run_outcomes_device else []
        assert f(None, C.byref(lp), 2, vp(st), 5, None, vp(plant), None, None, C.byref(op), vp(oc), *extra) == pkg.BAD_ARGUMENT
        assert f(fake, C.byref(lp), 2, vp(st), 5, None, vp(plant), None, None, None, vp(oc), *extra) == pkg.BAD_ARGUMENT
        assert f(fake, C.byref(lp), 2, vp(st), 5, None, vp(plant), None, None, C.byref(op), None, *extra) == pkg.BAD_ARGUMENT
        assert f(fake, None, 2, vp(st), 5, None, vp(plant), None, None, C.byref(op), vp(oc), *extra) == pkg.BAD_ARGUMENT
        assert f(fake, C.byref(lp), 2, None, 5, None, vp(plant), None, None, C.byref(op), vp(oc), *extra) == pkg.BAD_ARGUMENT
    assert oc.tobytes() == pkg.loop_outcomes(2, lib).tobytes()


def test_summarize_outcomes(lib, pkg):
    o = pkg.loop_outcomes(6, lib)
    o["ticks"][:5] = [40, 40, 12, 14, 12]
    o["down_tick"][2:5] = [18, 20, 18]
    o["min_height"][:5] = [0.29, 0.28, 0.14, 0.13, 0.12]
    o["min_upright"][:5] = [0.99, 0.98, 0.9, 0.4, 0.95]
    o["max_height_err"][:5] = [0.01, 0.02, 0.16, 0.17, 0.18]
    o["max_vel_err"][:5] = [0.1, 0.2, 0.3, 0.4, 0.5]
    o["sum_vel_err_sq"][:5] = [0.4, 1.6, 0.12, 0.14, 0.48]
    o["max_ang_vel"][:5] = [1, 2, 3, 4, 5]
    o["max_force_z"][:5] = [60, 70, 150, 140, 130]
    o["not_ok_ticks"][:5] = [0, 1, 3, 0, 0]
    o["rejected_ticks"][:5] = [0, 0, 2, 0, 0]
    o["iterations_sum"][:5] = [400, 440, 300, 200, 100]
    o["iterations_max"][:5] = [12, 14, 120, 30, 20]
    s = pkg.summarize_outcomes(o)
    assert s["robots"] == 6 and s["evaluated"] == 5 and s["down"] == 3 and s["down_fraction"] == 0.5
    assert s["down_tick_histogram"] == {18: 2, 20: 1} and s["first_down_tick"] == 18 and s["median_down_tick"] == 18.0
    assert s["min_height"] == 0.12 and s["median_min_height"] == 0.14 and s["min_upright"] == 0.4
    assert s["worst_height_err"] == 0.18 and s["median_height_err"] == 0.16
    assert s["worst_vel_err"] == 0.5 and s["median_vel_err"] == 0.3
    assert abs(s["worst_rms_vel_err"] - 0.2) < 1e-15 and abs(s["median_rms_vel_err"] - 0.1) < 1e-15
    assert s["worst_ang_vel"] == 5 and s["worst_force_z"] == 150
    assert s["not_ok_ticks"] == 4 and s["rejected_ticks"] == 2 and s["robots_with_rejected_solves"] == 1
    assert s["mean_iterations"] == 1440 / 118 and s["max_iterations"] == 120
    e = pkg.summarize_outcomes(pkg.loop_outcomes(3, lib))      # nothing accumulated yet: counts only
    assert e == {"robots": 3, "evaluated": 0, "down": 0, "down_fraction": 0.0, "down_tick_histogram": {}}


def test_outcome_metric_on_hand_made_sequences(tmp_path):
    exe = tmp_path / "loop_outcome_host"
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-o", str(exe), str(SRC)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sequence: 3 ticks accumulated, down at tick 3, frozen afterwards" in r.stdout
    assert "down rule: 8 cases" in r.stdout
    assert "200 of 200 two-segment accumulations equal the one-segment record" in r.stdout and "passed: 0 failures" in r.stdout
