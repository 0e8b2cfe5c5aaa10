"""CPU suite: the true ground of the closed loop's plant (qmpc_loop_run_ground*, include/qmpc.h) without a device.

The records' ABI and numpy dtypes, the init functions, the call-level argument checks that need no handle, random_go1_grounds, the
agreement of header, binding and unit table, and tests/native/loop_ground_host.cpp: loop_ground_leg / loop_ground_clamp /
loop_ground_valid / loop_ground_tally_one (csrc/qmpc_loop_math.h, the one source of the clamp, validity and counting rules) and the
momentum identity of one plant step under the delivered forces.  The harness is compiled host-only by hipcc, like
tests/native/loop_push_host.cpp."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
SRC = HERE / "native" / "loop_ground_host.cpp"
HIPCC = "/opt/rocm/bin/hipcc"
NEW = ("qmpc_ground_params_init", "qmpc_ground_tally_init", "qmpc_sizeof_ground_params", "qmpc_sizeof_ground_tally",
       "qmpc_loop_run_ground", "qmpc_loop_run_ground_device")


@pytest.fixture(scope="module")
def lib(pkg):
    import __graft_entry__ as g

    g.build_hip()
    return pkg.load_library()


def test_record_sizes_and_layouts(lib, pkg):
    gp, gt = pkg.GROUND_PARAMS_DTYPE, pkg.GROUND_TALLY_DTYPE
    assert lib.qmpc_sizeof_ground_params() == gp.itemsize == 64 and lib.qmpc_sizeof_ground_tally() == gt.itemsize == 32
    assert gp.names == ("mu", "fz_max") and [gp.fields[n][1] for n in gp.names] == [0, 32]      # the field order of the structs
    assert gp["mu"].shape == (4,) and gp["fz_max"].shape == (4,)
    assert gt.names == ("clipped_ticks", "first_clipped_tick", "friction_leg_ticks", "normal_leg_ticks")
    assert [gt.fields[n][1] for n in gt.names] == [0, 8, 16, 24]


def test_init_functions_write_every_byte(lib, pkg):
    for fill in (0x00, 0xFF, 0x5A):
        g = np.frombuffer(bytes([fill]) * (5 * 64), dtype=pkg.GROUND_PARAMS_DTYPE).copy()
        t = np.frombuffer(bytes([fill]) * (5 * 32), dtype=pkg.GROUND_TALLY_DTYPE).copy()
        lib.qmpc_ground_params_init(g.ctypes.data_as(C.c_void_p), 4)
        lib.qmpc_ground_tally_init(t.ctypes.data_as(C.c_void_p), 4)
        assert g[:4].tobytes() == pkg.ground_params(4).tobytes() and t[:4].tobytes() == pkg.ground_tallies(4).tobytes()
        assert g[4:].tobytes() == bytes([fill]) * 64 and t[4:].tobytes() == bytes([fill]) * 32      # ... and none beyond `batch`
    g, t = pkg.ground_params(3), pkg.ground_tallies(3)
    assert g.shape == (3,) and np.isposinf(g["mu"]).all() and np.isposinf(g["fz_max"]).all()
    assert t.shape == (3,) and [t[n].tolist() for n in t.dtype.names] == [[0.0] * 3, [-1.0] * 3, [0.0] * 3, [0.0] * 3]
    lib.qmpc_ground_params_init(None, 4)      # a NULL pointer is ignored
    lib.qmpc_ground_tally_init(None, 4)


def test_null_arguments_are_rejected(lib, pkg):
    lp = pkg.default_loop_params(lib)
    op = pkg.default_outcome_params(lib)
    st = np.zeros(2, dtype=pkg.LOOP_STATE_DTYPE)
    oc = pkg.loop_outcomes(2, lib)
    plant = np.zeros(2, dtype=pkg.PLANT_PARAMS_DTYPE)
    push = pkg.push_params(2, 2)
    gr, ta = pkg.ground_params(2), pkg.ground_tallies(2)
    gr["mu"] = 0.5
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    fake = C.c_void_p(8)      # never dereferenced: the null checks come first
    for f in (lib.qmpc_loop_run_ground, lib.qmpc_loop_run_ground_device):
        extra = [None] if f is lib.qmpc_loop_run_ground_device else []
        # with a ground record, through the push call (ground == NULL), through the outcome call (both NULL)
        for pu, n, g, t in ((vp(push), 2, vp(gr), vp(ta)), (None, 0, vp(gr), None), (vp(push), 2, None, vp(ta)), (None, 5, None, None)):
            assert f(None, C.byref(lp), 2, vp(st), 5, None, vp(plant), None, None, C.byref(op), vp(oc), pu, n, g, t, *extra) == pkg.BAD_ARGUMENT
            assert f(fake, C.byref(lp), 2, vp(st), 5, None, vp(plant), None, None, None, vp(oc), pu, n, g, t, *extra) == pkg.BAD_ARGUMENT
            assert f(fake, C.byref(lp), 2, vp(st), 5, None, vp(plant), None, None, C.byref(op), None, pu, n, g, t, *extra) == pkg.BAD_ARGUMENT
            assert f(fake, None, 2, vp(st), 5, None, vp(plant), None, None, C.byref(op), vp(oc), pu, n, g, t, *extra) == pkg.BAD_ARGUMENT
            assert f(fake, C.byref(lp), 2, None, 5, None, vp(plant), None, None, C.byref(op), vp(oc), pu, n, g, t, *extra) == pkg.BAD_ARGUMENT
        # a non-NULL push with pushes_per_robot outside 1 .. QMPC_MAX_PUSHES, with and without a ground record, whatever the handle
        for n in (0, -1, 9):
            for g in (vp(gr), None):
                assert f(fake, C.byref(lp), 2, vp(st), 5, None, vp(plant), None, None, C.byref(op), vp(oc), vp(push), n, g, vp(ta),
                         *extra) == pkg.BAD_ARGUMENT
    assert oc.tobytes() == pkg.loop_outcomes(2, lib).tobytes() and ta.tobytes() == pkg.ground_tallies(2).tobytes()


def test_random_go1_grounds(pkg):
    from quaternion_mpc_amd import scenarios

    a = pkg.random_go1_grounds(300, seed=4, mu=(0.1, 0.9))
    assert a.shape == (300,) and a.dtype == pkg.GROUND_PARAMS_DTYPE
    assert a.tobytes() == pkg.random_go1_grounds(300, seed=4, mu=(0.1, 0.9)).tobytes()
    assert a.tobytes() != pkg.random_go1_grounds(300, seed=5, mu=(0.1, 0.9)).tobytes()
    # a shard equals its block of the whole
    assert pkg.random_go1_grounds(70, seed=4, first=130, mu=(0.1, 0.9)).tobytes() == a[130:200].tobytes()
    # one mu per robot on its four legs, inside the range and spread over it; no normal limit unless asked for
    assert (a["mu"] == a["mu"][:, :1]).all() and a["mu"].min() >= 0.1 and a["mu"].max() < 0.9
    assert np.histogram(a["mu"][:, 0], bins=4, range=(0.1, 0.9))[0].min() > 40
    assert np.isposinf(a["fz_max"]).all()
    # the draws are the generator's, in the documented order mu, fz_max
    u = scenarios._uniform(0x5EED4000 + 4, np.arange(300, dtype=np.uint64), 2)
    assert np.array_equal(a["mu"][:, 0], 0.1 + (0.9 - 0.1) * u[:, 0])
    b = pkg.random_go1_grounds(300, seed=4, mu=(0.1, 0.9), fz_max=(30.0, 60.0))
    assert np.array_equal(b["mu"], a["mu"]) and (b["fz_max"] == b["fz_max"][:, :1]).all()
    assert np.array_equal(b["fz_max"][:, 0], 30.0 + 30.0 * u[:, 1])
    c = pkg.random_go1_grounds(20, seed=1, mu=(0.3, 0.3))
    assert (c["mu"] == 0.3).all()


def test_header_binding_and_unit_table_agree(lib, pkg):
    header = (REPO / "include" / "qmpc.h").read_text()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(REPO / "quaternion-mpc_amd" / "csrc" / "libqmpc_hip.so")], check=True,
                        capture_output=True, text=True).stdout
    for sym in NEW:
        assert sym in pkg.EXPORTED_SYMBOLS and re.search(r"\b" + sym + r"\(", header) and re.search(r" T " + sym + r"$", nm, re.M), sym
    assert "rec_ground_check_launch" not in nm      # (the launchers of the new units are hidden: not part of the C ABI)
    m = re.search(r"typedef struct qmpc_ground_params \{.*?double mu\[4\];.*?double fz_max\[4\];.*?\} qmpc_ground_params;", header, re.S)
    assert m
    m = re.search(r"typedef struct qmpc_ground_tally \{(.*?)\} qmpc_ground_tally;", header, re.S)
    assert m and re.findall(r"double (\w+);", m.group(1)) == list(pkg.GROUND_TALLY_DTYPE.names)
    # the ground call takes the push call's arguments in their order, then ground and tally (before stream)
    args = lambda name: [a.split()[-1].lstrip("*") for a in re.search(name + r"\((.*?)\);", header, re.S).group(1).split(",")]      # noqa: E731
    assert args("qmpc_loop_run_ground") == args("qmpc_loop_run_pushes") + ["ground", "tally"]
    assert args("qmpc_loop_run_ground_device") == args("qmpc_loop_run_pushes_device")[:-1] + ["d_ground", "d_tally", "stream"]
    assert lib.qmpc_loop_run_ground.argtypes == lib.qmpc_loop_run_pushes.argtypes + [C.c_void_p, C.c_void_p]
    assert lib.qmpc_loop_run_ground_device.argtypes == lib.qmpc_loop_run_pushes_device.argtypes[:-1] + [C.c_void_p] * 3
    for name in ("loop_run_ground", "loop_run_ground_device"):
        assert hasattr(pkg.Solver, name), name
    for name in ("GROUND_PARAMS_DTYPE", "GROUND_TALLY_DTYPE", "ground_params", "ground_tallies", "random_go1_grounds"):
        assert hasattr(pkg, name), name
    import __graft_entry__ as g

    units = {n: (deps, flags) for n, deps, flags in g.hip_units()}
    csrc = REPO / "quaternion-mpc_amd" / "csrc"
    for new in ("qmpc_loop_ground", "qmpc_loop_cground"):
        assert new in units and (csrc / (new + ".hip")).exists()
        assert units[new][1] == units["qmpc_loop_push"][1] and units[new][0] == units["qmpc_loop_push"][0]      # the twin's flags and sources
        # each unit is the shared text once more, not a copy of it
        text = (csrc / (new + ".hip")).read_text()
        assert '#include "qmpc_loop_rec.inc"' in text and "#define QMPC_REC_EXT 3" in text and "__global__" not in text
        assert ("#define QMPC_REC_CONVEX" in text) == (new == "qmpc_loop_cground")
    assert "#define QMPC_REC_EXT 2" in (csrc / "qmpc_loop_crec.hip").read_text()      # ... and the three ConvexMpc calls keep their unit


def test_ground_rules_and_momentum_identity(tmp_path):
    exe = tmp_path / "loop_ground_host"
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-o", str(exe), str(SRC)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "clamp: 18 cases" in r.stdout and "validity: 36 invalid records rejected" in r.stdout
    assert "tally: 4 ticks counted" in r.stdout
    assert "momentum identity: 200 random steps, 400 clamped legs" in r.stdout and "passed: 0 failures" in r.stdout
