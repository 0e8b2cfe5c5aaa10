"""CPU suite: QuatMpc solves with a contact schedule over the horizon (qmpc_solve_schedule*) without a device.

The reference of this feature is the independent problem statement tests/kkt_schedule.py (the oracle has no per-knot contacts):
the points of tests/golden/schedule_fixtures.npz (tests/golden/make_schedule_fixtures.py: its active-set Newton method) pass the
certificate of tests/test_kkt_certificate.py with that file's tolerances; a constant schedule is the plain problem, exactly; the
ABI, the binding and the unit table agree and the call-level refusals that need no handle hold; qmpc_gait_predict gives, bit for
bit, the masks of stepping a copy of the state through the FSM tests/test_loop_gait_cpu.py restates in Python."""
import copy
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import kkt_independent as K
import kkt_schedule as KS
from test_kkt_certificate import TOL_FEASIBILITY, TOL_INDEPENDENT, TOL_STATIONARITY
from test_loop_gait_cpu import DT, FREQS, TABLE, Leg

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
FIX = HERE / "golden" / "schedule_fixtures.npz"
NEW = ("qmpc_solve_schedule", "qmpc_solve_schedule_device", "qmpc_gait_predict")
CASES = (("n10", 10, 8, ("constant", "trot_four_other", "trot_other", "trot_three")), ("n20", 20, 2, ("constant", "trot_four_other")))


@pytest.fixture(scope="module")
def fix():
    return np.load(FIX)


@pytest.fixture(scope="module")
def lib(pkg):
    import __graft_entry__ as g

    g.build_hip()
    return pkg.load_library()


@pytest.fixture(scope="module")
def host():
    import __graft_entry__ as g

    h = C.CDLL(str(g.build_host()))
    h.qh_gait_predict.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_void_p]
    h.qh_gait_predict.restype = None
    return h


def _problem(pkg, N, i, masks):
    rec = pkg.random_go1_trot_states(8, config_id=2)
    par = pkg.default_params(N, pkg.MODE_CONVERGED, pkg.load_library())
    return KS.ScheduleProblem(par, rec[i], masks), par, rec


# ---- the schedules -----------------------------------------------------------------------------------------------------------
def test_schedule_families(pkg):
    rec = pkg.random_go1_trot_states(8, config_id=2)
    assert pkg.SCHEDULE_FAMILIES == CASES[0][3]
    for N in (10, 20):
        fam = pkg.schedule_families(rec, N)
        assert tuple(fam) == pkg.SCHEDULE_FAMILIES
        for name, s in fam.items():
            assert s.dtype == np.uint8 and s.shape == (8, N) and s.flags.c_contiguous and (s >= 1).all() and (s <= 15).all(), name
        m = (rec["contacts"] != 0).astype(int) @ (1 << np.arange(4))
        assert set(m.tolist()) == {9, 6, 15}      # trot records: one diagonal stands, or (state 7) all four legs
        assert (fam["constant"] == m[:, None]).all() and np.array_equal(fam["constant"], pkg.constant_schedule(rec, N))
        o = np.where(m == 15, 9, 15 - m)      # a standing robot starts to trot on FL + RR
        f = fam["trot_four_other"]
        assert (f[:, :3] == m[:, None]).all() and (f[:, 3:5] == 15).all() and (f[:, 5:] == o[:, None]).all()
        f, cut = fam["trot_other"], (2 * N) // 5
        assert (f[:, :cut] == m[:, None]).all() and (f[:, cut:] == o[:, None]).all()
        f = fam["trot_three"]
        assert (f[:, :N // 2] == m[:, None]).all()
        assert all(bin(int(v)).count("1") == min(4, bin(int(mm)).count("1") + 1) and int(v) & int(mm) == int(mm)
                   for row, mm in zip(f[:, N // 2:], m) for v in row)
    assert [int(np.argmax(pkg.schedule_families(rec, 10)[n][0] != m[0])) for n in pkg.SCHEDULE_FAMILIES] == [0, 3, 4, 5]      # 3+2+5, 4+6, 5+5


# ---- the certificate ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_stored_points_pass_the_certificate(pkg, fix, case):
    name, N, n, fams = case
    assert tuple(fix[name + "_families"]) == fams
    rec = pkg.random_go1_trot_states(8, config_id=2)
    par = pkg.default_params(N, pkg.MODE_CONVERGED, pkg.load_library())
    sched = pkg.schedule_families(rec, N)
    for fam in fams:
        U = fix[f"{name}_{fam}_U"]
        assert U.shape == (n, N, 12)
        worst, active = {}, 0
        for i in range(n):
            prob = KS.ScheduleProblem(par, rec[i], sched[fam][i])
            r = prob.kkt(U[i])
            for k, v in r.items():
                worst[k] = max(worst.get(k, v), v)
            active += prob.active_rows(U[i])
            swing = U[i].reshape(N, 4, 3)[prob.conk == 0]
            assert (swing == 0.0).all() and not np.signbit(swing).any()      # exactly +0.0
            assert fix[f"{name}_{fam}_active"][i] == (fix[f"{name}_{fam}_W"][i] >= 0).sum()
        print(name, fam, f"stationarity_nnls {worst['stationarity_nnls']:.2e} violation {worst['violation']:.2e} swing "
              f"{worst['swing_force']:.1e} active rows/instance {active / n:.1f} iterations {fix[f'{name}_{fam}_iterations'].tolist()}")
        assert worst["stationarity_nnls"] <= TOL_STATIONARITY
        assert worst["violation"] <= TOL_FEASIBILITY
        assert worst["swing_force"] == 0.0
        assert active / n >= 1


def test_constant_schedule_is_the_plain_problem_exactly(pkg):
    rng = np.random.default_rng(7)
    for N in (10, 20):
        rec = pkg.random_go1_trot_states(8, config_id=2)
        par = pkg.default_params(N, pkg.MODE_CONVERGED, pkg.load_library())
        sched = pkg.constant_schedule(rec, N)
        for i in (0, 3):
            plain, prob = K.QuatProblem(par, rec[i]), KS.ScheduleProblem(par, rec[i], sched[i])
            for _ in range(2):
                U = rng.normal(0.0, 30.0, (N, 12))
                Jp, gp = plain.value_and_grad(U)
                Js, gs = prob.value_and_grad(U)
                assert Jp == Js and gp.tobytes() == gs.tobytes()


def test_stored_constant_points_are_the_plain_problems_points(pkg, fix):
    """... found by kkt_independent.active_set_newton on QuatProblem (the stored solutions of tests/golden/kkt_fixtures.npz: the
    same eight config-2 states at N = 10)."""
    kf = np.load(HERE / "golden" / "kkt_fixtures.npz")
    U = fix["n10_constant_U"]
    d = np.abs(U - kf["quat_n10_U_independent"][:8]).max()
    print(f"constant schedule vs the plain problem's active-set Newton points: {d:.2e} N")
    assert d <= TOL_INDEPENDENT
    # ... and one of them once more from scratch, with the plain solver itself (the flat view changes nothing: difference 0.0)
    prob, par, rec = _problem(pkg, 10, 0, pkg.constant_schedule(pkg.random_go1_trot_states(8, config_id=2), 10)[0])
    Up, _, _, _ = K.active_set_newton(K.QuatProblem(par, rec[0]))
    print(f"re-solved plain point vs stored constant-schedule point: {np.abs(Up - U[0]).max():.2e} N")
    assert np.abs(Up - U[0]).max() <= TOL_INDEPENDENT


def test_a_schedule_moves_the_first_knot_and_replaces_the_later_ones(fix):
    c, f = fix["n10_constant_U"], fix["n10_trot_other_U"]
    d0 = np.abs(c[:, 0] - f[:, 0]).max(axis=1)
    print("first-knot force, trot -> other against constant [N]:", np.array2string(d0, precision=3))
    assert (d0 > 1e-3).any()
    assert np.abs(c[:, 4:] - f[:, 4:]).max() > 10.0


# ---- ABI -----------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_unit_table_agree(lib, pkg):
    header = (REPO / "include" / "qmpc.h").read_text()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(REPO / "quaternion-mpc_amd" / "csrc" / "libqmpc_hip.so")], check=True,
                        capture_output=True, text=True).stdout
    for sym in NEW:
        assert sym in pkg.EXPORTED_SYMBOLS and re.search(r"\b" + sym + r"\(", header) and re.search(r" T " + sym + r"$", nm, re.M), sym
    assert "qmpc_wform_sched_launch" not in nm and "qmpc_wform_sched_set_lds" not in nm      # hidden: not part of the C ABI
    args = lambda name: [a.split()[-1].lstrip("*") for a in re.search(name + r"\((.*?)\);", header, re.S).group(1).split(",")]      # noqa: E731
    assert args("qmpc_solve_schedule") == ["h", "batch", "in", "iparams", "schedule", "forces_body", "info", "traj_u", "traj_x"]
    assert args("qmpc_solve_schedule_device") == ["h", "batch", "d_in", "d_iparams", "d_schedule", "d_forces_body", "d_info", "d_traj_u",
                                                   "d_traj_x", "stream"]
    assert args("qmpc_gait_predict") == ["lp", "g", "s", "h", "N", "masks"]
    assert len(lib.qmpc_solve_schedule.argtypes) == 9 and len(lib.qmpc_solve_schedule_device.argtypes) == 10
    assert re.search(r"QMPC_QUERY_KERNEL_FOR_SCHEDULE\s*=\s*16\b", header) and pkg.QUERY_KERNEL_FOR_SCHEDULE == 16
    for name in ("solve_schedule", "solve_schedule_device", "kernel_for_schedule"):
        assert hasattr(pkg.Solver, name), name
    for name in ("constant_schedule", "predict_schedule", "schedule_families"):
        assert hasattr(pkg, name), name
    import __graft_entry__ as g

    units = {n: (deps, flags) for n, deps, flags in g.hip_units()}
    csrc = REPO / "quaternion-mpc_amd" / "csrc"
    assert "qmpc_wform_sched" in units and units["qmpc_wform_sched"] == units["qmpc_wform"]      # qmpc_wform's sources and flags
    text = (csrc / "qmpc_wform_sched.hip").read_text()
    assert '#include "qmpc_wform_body.inc"' in text and "#define QMPC_WSCHED 1" in text
    # the flag is set by that unit alone: every other unit compiles the sources without it
    for f in csrc.glob("*.hip"):
        assert ("#define QMPC_WSCHED" in f.read_text()) == (f.name == "qmpc_wform_sched.hip"), f.name
    slots = (csrc / "qmpc_kernel_slots.h").read_text()
    assert "kWformSchedSlots = 3" in slots and "wform_sched_slot" in slots
    hip = (csrc / "qmpc_hip.hip").read_text()
    assert "qmpc_wform_sched_set_lds()" in hip and "plan_schedule(" in (csrc / "qmpc_plan.h").read_text()
    # one source of the predictor: the library and the host shim call loop_gait_predict of qmpc_loop_math.h
    assert len(re.findall(r"\bvoid loop_gait_predict\(", (csrc / "qmpc_loop_math.h").read_text())) == 1
    assert "qmpc_loop::loop_gait_predict(" in hip
    assert "qmpc_loop::loop_gait_predict(" in (REPO / "quaternion-mpc_amd" / "host" / "host_shim.cpp").read_text()


def test_null_arguments_are_rejected(lib, pkg):
    rec = pkg.random_go1_trot_states(2, config_id=2)
    sched = pkg.constant_schedule(rec, 10)
    ip = pkg.instance_params(pkg.default_params(10, pkg.MODE_CONVERGED, lib), 2)
    f = np.zeros((2, 12))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    fake = C.c_void_p(8)      # never dereferenced: the null checks come first
    host_call = lambda h, b, i, s, o: lib.qmpc_solve_schedule(h, b, i, vp(ip), s, o, None, None, None)      # noqa: E731
    dev_call = lambda h, b, i, s, o: lib.qmpc_solve_schedule_device(h, b, i, None, s, o, None, None, None, None)      # noqa: E731
    for call in (host_call, dev_call):
        assert call(None, 2, vp(rec), vp(sched), vp(f)) == pkg.BAD_ARGUMENT
        assert call(fake, -1, vp(rec), vp(sched), vp(f)) == pkg.BAD_ARGUMENT
        assert call(fake, 2, None, vp(sched), vp(f)) == pkg.BAD_ARGUMENT
        assert call(fake, 2, vp(rec), None, vp(f)) == pkg.BAD_ARGUMENT
        assert call(fake, 2, vp(rec), vp(sched), None) == pkg.BAD_ARGUMENT
    assert not f.any()
    # the predictor ignores null pointers and a horizon below one knot
    st = pkg.loop_states(np.zeros((1, 7)))
    lp = pkg.default_loop_params(lib)
    out = np.full(4, 0xAA, dtype=np.uint8)
    lib.qmpc_gait_predict(C.byref(lp), None, None, 0.005, 4, vp(out))
    lib.qmpc_gait_predict(C.byref(lp), None, vp(st), 0.005, 4, None)
    lib.qmpc_gait_predict(None, None, vp(st), 0.005, 4, vp(out))
    lib.qmpc_gait_predict(C.byref(lp), None, vp(st), 0.005, 0, vp(out))
    assert (out == 0xAA).all()
    with pytest.raises(ValueError):
        pkg.Solver.solve_schedule(type("S", (), {"params": pkg.default_params(10, pkg.MODE_CONVERGED, lib)})(), rec, sched[:, :9])


# ---- the predictor ---------------------------------------------------------------------------------------------------------------
def _walked_states(pkg, name, f, phases, rng):
    """`phases` robots of one gait at frequency f, each walked a different number of ticks by the Python FSM (some ticks with an
    early contact, so the legs' accumulators leave the lattice of the plain schedule): the state records and the FSM's legs."""
    fs, sp, ph = TABLE[name]
    st = pkg.loop_states(np.zeros((phases, 7)))
    legs = []
    for b in range(phases):
        L = [Leg(fs[l], sp[l], ph[l]) for l in range(4)]
        early = rng.random((b, 4)) < (0.3 if b % 2 else 0.0)
        for t in range(b):
            for l in range(4):
                L[l].update(f * DT, bool(early[t, l]))
        for l in range(4):
            p, s, idx, prev, start, end = L[l].fields()
            leg = st["leg"][b][l]
            leg["gait_phase"], leg["state"], leg["pattern_index"], leg["prev_pattern_index"] = p, s, idx, prev
            leg["start_time"], leg["end_time"], leg["not_first_call"] = start, end, 1.0
            st["contacts"][b][l] = s
        legs.append(L)
    return st, legs


def _expected(legs, f, h, N):
    out = np.zeros((len(legs), N), dtype=np.uint8)
    for b, L0 in enumerate(legs):
        L = copy.deepcopy(L0)
        out[b, 0] = sum(int(L[l].state) << l for l in range(4))
        for k in range(1, N):
            out[b, k] = sum(int(L[l].update(f * h, False)) << l for l in range(4))
    return out


@pytest.mark.parametrize("name", list(TABLE))
def test_predictor_equals_the_fsm_stepped(pkg, lib, host, name):
    rng = np.random.default_rng(11)
    for f in FREQS:
        st, legs = _walked_states(pkg, name, f, 200, rng)
        g = pkg.gait_params(200, name, gait_freq=f)
        before = st.tobytes()
        for N in (10, 20):
            got = pkg.predict_schedule(None, g, st, DT, N, lib)
            want = _expected(legs, f, DT, N)
            assert got.dtype == np.uint8 and got.shape == (200, N)
            assert got.tobytes() == want.tobytes(), (name, f, N, np.argwhere(got != want)[:4])
            shim = np.zeros_like(got)
            for b in range(200):
                host.qh_gait_predict(g[b:b + 1].ctypes.data, st[b:b + 1].ctypes.data, DT, N, shim[b:b + 1].ctypes.data)
            assert shim.tobytes() == want.tobytes()
        assert st.tobytes() == before      # the state is unchanged
        assert len({r.tobytes() for r in got}) > 3      # the phases really differ


def test_trot_prediction_from_mid_stance_switches_where_the_fsm_switches(pkg, lib):
    lp = pkg.default_loop_params(lib)
    f = lp.gait_freq      # 2.2 Hz: a leg's arc is 0.5 / (2.2 * 0.005) = 45.45 ticks
    fs, sp, ph = TABLE["trot"]
    L = [Leg(fs[l], sp[l], ph[l]) for l in range(4)]
    for _ in range(35):      # mid-stance of the first diagonal: the stance exit is at tick 46 (phase 0.506 >= 0.5), 11 ticks on
        for l in range(4):
            L[l].update(f * DT, False)
    st = pkg.loop_states(np.zeros((1, 7)))
    for l in range(4):
        p, s, idx, prev, start, end = L[l].fields()
        leg = st["leg"][0][l]
        leg["gait_phase"], leg["state"], leg["pattern_index"], leg["prev_pattern_index"], leg["start_time"], leg["end_time"] = p, s, idx, prev, start, end
        st["contacts"][0][l] = s
    got = pkg.predict_schedule(lp, None, st, DT, 20, lib)[0]      # gait None: the reference's trot at lp.gait_freq
    assert got.tolist() == [9] * 11 + [6] * 9
    assert got.tobytes() == _expected([L], f, DT, 20)[0].tobytes()
    assert pkg.predict_schedule(lp, None, st, DT, 10, lib)[0].tolist() == [9] * 10      # N = 10 does not reach the switch
    assert got.tobytes() == pkg.predict_schedule(None, pkg.gait_params(1, "trot", gait_freq=f), st, DT, 20, lib)[0].tobytes()
