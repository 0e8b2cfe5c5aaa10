"""CPU suite: the timed push windows of the closed loop (qmpc_loop_run_pushes*, include/qmpc.h) without a device.

The record's ABI and numpy dtype, the call-level argument checks that need no handle, random_go1_pushes, and
tests/native/loop_push_host.cpp: loop_push_wrench / loop_push_valid (csrc/qmpc_loop_math.h, the one source of the window, combination
and validity rules) and the impulse identities of one plant step under the effective wrench.  The harness is compiled host-only by
hipcc, like tests/native/loop_outcome_host.cpp."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
SRC = HERE / "native" / "loop_push_host.cpp"
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def lib(pkg):
    import __graft_entry__ as g

    g.build_hip()
    return pkg.load_library()


def test_push_record_size_and_layout(lib, pkg):
    dt = pkg.PUSH_PARAMS_DTYPE
    assert lib.qmpc_sizeof_push_params() == dt.itemsize == 64
    assert dt.names == ("start_tick", "ticks", "force_world", "torque_body")      # the field order of struct qmpc_push_params
    assert [dt.fields[n][1] for n in dt.names] == [0, 8, 16, 40]
    assert dt["force_world"].shape == (3,) and dt["torque_body"].shape == (3,)
    assert pkg.MAX_PUSHES == 8
    header = (HERE.parent / "include" / "qmpc.h").read_text()
    assert "#define QMPC_MAX_PUSHES 8" in header


def test_push_params_are_no_push(pkg):
    one = pkg.push_params(5)
    assert one.shape == (5, 1) and one.dtype == pkg.PUSH_PARAMS_DTYPE and one.tobytes() == bytes(5 * 64)
    three = pkg.push_params(4, per_robot=3)
    assert three.shape == (4, 3) and three.tobytes() == bytes(4 * 3 * 64)
    three["start_tick"][2, 1] = 7.0      # robot 2's window 1 is push[2 * 3 + 1]
    assert three.ravel()[2 * 3 + 1]["start_tick"] == 7.0


def test_null_arguments_are_rejected(lib, pkg):
    lp = pkg.default_loop_params(lib)
    op = pkg.default_outcome_params(lib)
    st = np.zeros(2, dtype=pkg.LOOP_STATE_DTYPE)
    oc = pkg.loop_outcomes(2, lib)
    plant = np.zeros(2, dtype=pkg.PLANT_PARAMS_DTYPE)
    push = pkg.push_params(2, 2)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    fake = C.c_void_p(8)      # never dereferenced: the null checks come first
    for f in (lib.qmpc_loop_run_pushes, lib.qmpc_loop_run_pushes_device):
        extra = [None] if f is lib.qmpc_loop_run_pushes_device else []
        for pu, n in ((vp(push), 2), (None, 0), (None, 5)):      # with windows, and through the outcome call (push == NULL)
            assert f(None, C.byref(lp), 2, vp(st), 5, None, vp(plant), None, None, C.byref(op), vp(oc), pu, n, *extra) == pkg.BAD_ARGUMENT
            assert f(fake, C.byref(lp), 2, vp(st), 5, None, vp(plant), None, None, None, vp(oc), pu, n, *extra) == pkg.BAD_ARGUMENT
            assert f(fake, C.byref(lp), 2, vp(st), 5, None, vp(plant), None, None, C.byref(op), None, pu, n, *extra) == pkg.BAD_ARGUMENT
            assert f(fake, None, 2, vp(st), 5, None, vp(plant), None, None, C.byref(op), vp(oc), pu, n, *extra) == pkg.BAD_ARGUMENT
            assert f(fake, C.byref(lp), 2, None, 5, None, vp(plant), None, None, C.byref(op), vp(oc), pu, n, *extra) == pkg.BAD_ARGUMENT
        # a non-NULL push with pushes_per_robot outside 1 .. QMPC_MAX_PUSHES, whatever the handle
        for n in (0, -1, 9):
            assert f(fake, C.byref(lp), 2, vp(st), 5, None, vp(plant), None, None, C.byref(op), vp(oc), vp(push), n, *extra) == pkg.BAD_ARGUMENT
    assert oc.tobytes() == pkg.loop_outcomes(2, lib).tobytes() and push.tobytes() == bytes(4 * 64)


def test_random_go1_pushes(pkg):
    from quaternion_mpc_amd import scenarios

    dt = 0.005
    a = pkg.random_go1_pushes(300, seed=4, per_robot=2, start=(0, 91), ticks=(1, 12), impulse=(2.0, 9.0), dt=dt)
    assert a.shape == (300, 2) and a.dtype == pkg.PUSH_PARAMS_DTYPE
    assert a.tobytes() == pkg.random_go1_pushes(300, seed=4, per_robot=2, start=(0, 91), ticks=(1, 12), impulse=(2.0, 9.0), dt=dt).tobytes()
    assert a.tobytes() != pkg.random_go1_pushes(300, seed=5, per_robot=2, start=(0, 91), ticks=(1, 12), impulse=(2.0, 9.0), dt=dt).tobytes()
    # a shard equals its block of the whole
    shard = pkg.random_go1_pushes(70, seed=4, first=130, per_robot=2, start=(0, 91), ticks=(1, 12), impulse=(2.0, 9.0), dt=dt)
    assert shard.tobytes() == a[130:200].tobytes()
    # integral windows inside their ranges, horizontal forces, no torque
    assert (a["start_tick"] == np.floor(a["start_tick"])).all() and (a["start_tick"] >= 0).all() and (a["start_tick"] <= 90).all()
    assert (a["ticks"] == np.floor(a["ticks"])).all() and (a["ticks"] >= 1).all() and (a["ticks"] <= 11).all()
    assert len(np.unique(a["start_tick"])) > 40 and len(np.unique(a["ticks"])) == 11
    assert (a["force_world"][..., 2] == 0).all() and (a["torque_body"] == 0).all()
    # |F| ticks dt is the impulse drawn: the third uniform of the window's four (the generator's documented order)
    u = scenarios._uniform(0x5EED3000 + 4, np.arange(300, dtype=np.uint64), 8).reshape(300, 2, 4)
    drawn = 2.0 + 7.0 * u[:, :, 2]
    got = np.linalg.norm(a["force_world"], axis=-1) * a["ticks"] * dt
    assert np.abs(got - drawn).max() <= 1e-13 * 9.0
    assert got.min() >= 2.0 - 1e-12 and got.max() <= 9.0 + 1e-12 and got.max() - got.min() > 5.0
    # the direction is spread over the circle
    ang = np.arctan2(a["force_world"][..., 1], a["force_world"][..., 0]).ravel()
    assert np.histogram(ang, bins=8, range=(-np.pi, np.pi))[0].min() > 40
    # a fixed impulse: every window carries it
    b = pkg.random_go1_pushes(50, seed=1, impulse=(6.0, 6.0), ticks=(3, 3), dt=dt)
    assert b.shape == (50, 1) and (b["ticks"] == 3).all()
    assert np.abs(np.linalg.norm(b["force_world"], axis=-1) * 3 * dt - 6.0).max() <= 1e-13 * 6.0


def test_push_rules_and_impulse_identities(tmp_path):
    exe = tmp_path / "loop_push_host"
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-o", str(exe), str(SRC)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "window rule: 14 cases" in r.stdout and "combination rule: 9 cases" in r.stdout
    assert "validity rule: 24 non-finite windows rejected" in r.stdout
    assert "impulse identities: 200 random steps, force and torque" in r.stdout and "passed: 0 failures" in r.stdout
