"""GPU suite (-m gpu): the record loops on the lane kernels with per-lane parameters (qmpc_lane_inst_kernel.inc; DESIGN.md section
3t) under the knobs that select their other forms.  The other files run these kernels with the default knobs only: lane pairs in
every pass (-34), the sort with the robots that will not solve last.  Here, set before the handle is created:
  QMPC_LANE_PAIR = 0 / 2 / 4   the warm QuatMpc kernel's 32-lane masked form, -33 (the cold rounds' trial pass split) and -32 (the
                               cold rounds split)
  QMPC_LANE_SORT = 0           no sort: the kernels' null-perm path, warm and cold, both models
  QMPC_LANE_SORT_IDLE = 0      the sort's idle_last = 0 argument, both models
The assertion is the byte contract of the other files: uniform records give the states, force trace and contact trace of the plain
loop on the same handle under the same knobs.  65 robots: a full wavefront of 32 (pairs or masked), a second one, a tail of one."""
import pytest

from records_fleet import convex_fleet, quat_fleet, same, walk

pytestmark = pytest.mark.gpu

B, N, T0, T = 65, 10, 3, 6
LANE_KNOBS = {"quat": (("QMPC_LOOP_FUSED", "0"), ("QMPC_LANE_MIN", "1"), ("QMPC_LANE_INST_MIN", "1")),
              "convex": (("QMPC_LOOP_FUSED", "0"), ("QMPC_LANE_MIN", "1"), ("QMPC_LANE_CINST_MIN", "1"))}
CASES = [("quat", True, "QMPC_LANE_PAIR", "0"), ("quat", True, "QMPC_LANE_PAIR", "2"), ("quat", True, "QMPC_LANE_PAIR", "4"),
         ("quat", True, "QMPC_LANE_SORT", "0"), ("quat", True, "QMPC_LANE_SORT_IDLE", "0"),
         ("convex", True, "QMPC_LANE_SORT", "0"), ("convex", True, "QMPC_LANE_SORT_IDLE", "0"),
         ("quat", False, "QMPC_LANE_SORT", "0"), ("convex", False, "QMPC_LANE_SORT", "0")]


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


@pytest.mark.parametrize("model,warm,knob,value", CASES)
def test_uniform_records_equal_the_plain_loop_under_the_knob(pkg, lib, monkeypatch, model, warm, knob, value):
    for k, v in LANE_KNOBS[model] + ((knob, value),):
        monkeypatch.setenv(k, v)
    convex = model == "convex"
    p = (pkg.default_convex_params if convex else pkg.default_params)(N, pkg.MODE_CONVERGED, lib)
    p.ipm_mu0 = 1e-6
    lp, st, cmds = convex_fleet(pkg, lib, B) if convex else quat_fleet(pkg, lib, B, seed=42, trot=True)
    lp.warm_start = 1.0 if warm else 0.0
    s = pkg.Solver(p, B, device=0, lib=lib)
    s.set_instances_policy("auto")
    if convex:
        s.set_convex_records(True)
        s.set_convex_lane_records(True)
        s.set_convex_warm_records(True)
    else:
        s.set_loop_warm_records(True)
    plan, plain = s.loop_instances_plan(B, True, warm), s.loop_instances_plan(B, False, warm)
    print(f"{model} warm={warm} {knob}={value}: records call {plan}, plain loop {plain}")
    assert plan is not None and plan[0] == "per_tick" and plan[1] in ("lane", "lane_handoff")
    assert plain is not None and plain[0] == "per_tick" and plain[1] in ("lane", "lane_handoff")
    ref = walk(lambda x, t, tr: s.loop_run(x, t, lp, trace=tr), st, cmds, T0, T)
    ctrl, plant = pkg.instance_params(p, B), pkg.plant_params(p, B)
    got = walk(lambda x, t, tr: s.loop_run_instances(x, t, lp, ctrl=ctrl, plant=plant, trace=tr), st, cmds, T0, T)
    last = pkg.KERNEL_FAMILY[s.query(pkg.QUERY_LAST_KERNEL)]
    s.close()
    assert last == plan[1]
    # the reference run is a run: every robot reached the last tick and solved, feet swung, forces acted
    assert (ref[0]["tick"] == T0 + T).all() and (ref[0]["status"] == pkg.OK).mean() >= 0.95
    assert (ref[2] == 0).any() and (ref[1] != 0).any()
    assert len(got) == len(ref) == 3
    for name, a, b in zip(("states", "force trace", "contact trace"), ref, got):
        assert same(a, b), name
