"""GPU suite: the closed-loop calls with per-robot records are ONE chain (qmpc_loop_run_outcomes* .. qmpc_loop_run_motors*).

An entry point that is given the records of a lower kind only -- NULL for everything higher -- makes that kind's call
(csrc/qmpc_loop_records.h: loop_recs_normalise): for every kind, every entry point above it returns the bytes of the kind's own
entry point, through host buffers and once through device buffers (the motors call); and the call with all seven kinds of record
equals itself split into two calls.  3 robots (one standing, two walking) for 3 ticks at the default horizon, on a QuatMpc handle
and on a ConvexMpc handle that opted in (set_convex_records), in both launch forms (QMPC_LOOP_FUSED, read by qmpc_create)."""
import numpy as np
import pytest

from test_gpu_loop_actuation import MODELS, _all_same, _binding, _fleet, _mixed, _params, _records, _same, _shoves, _solver
from test_gpu_loop_actuation import lib  # noqa: F401  (the fixture: raises if the HIP extension is missing, no fallback)
from test_gpu_loop_gait import _mixed_gaits

pytestmark = pytest.mark.gpu

B, T = 3, 3
KINDS = ["outcomes", "pushes", "ground", "actuation", "sensing", "gaits", "motors"]      # the entry points above the plain loop
OWN = {"pushes": ("push",), "ground": ("ground",), "actuation": ("act",), "sensing": ("sense",), "gaits": ("gait",), "motors": ("motor",)}
NACC = {"outcomes": 1, "pushes": 1, "ground": 2, "actuation": 3, "sensing": 4, "gaits": 4, "motors": 5}      # accumulators an entry point returns


@pytest.fixture(params=[(m, f) for m in MODELS for f in ("persistent", "per_tick")], ids=lambda p: "-".join(p))
def fleet(request, pkg, lib, monkeypatch):
    """A solver of the model in the launch form, the fleet's states and one record of every kind; rec[name]: what the entry
    points take under that keyword"""
    model, form = request.param
    monkeypatch.setenv("QMPC_LOOP_FUSED", "1" if form == "persistent" else "0")
    p = _params(pkg, lib, model)
    lp, st = _fleet(pkg, lib, B, model=model)
    ctrl, plant = _records(pkg, p, B, "both", model=model)
    act, line = _mixed(pkg, p, lp, B)
    rec = dict(push=_shoves(pkg, lp, B, 40, (0.0, 1.0), (2.0, 1.0)), ground=_binding(pkg, p, B), act=act, lines=line,
               sense=pkg.random_go1_senses(B, seed=3), gait=_mixed_gaits(pkg, lp, B), motor=pkg.random_go1_motors(B, seed=5, scale=(0.15, 0.6)))
    s = _solver(pkg, lib, p, B, model)
    assert s.loop_instances_plan(B, True, False)[0] == form
    yield s, st, rec, dict(lp=lp, ctrl=ctrl, plant=plant, op=pkg.default_outcome_params(lib), trace=True)
    s.close()


def _accepts(entry):
    """the accumulators beyond the outcome records that the entry point takes (its keywords for them)"""
    i = KINDS.index(entry)
    return [n for n, k in (("tallies", "ground"), ("lines", "actuation"), ("seen", "sensing"), ("mtallies", "motors")) if i >= KINDS.index(k)]


def _call(s, entry, kind, st, ticks, rec, common, carry=None):
    """Entry point `entry` with the records of the kinds up to `kind` and None for the higher ones.  The accumulators it takes are
    fresh ones (the delay lines: rec["lines"], given whether or not there is an actuation record) or, with carry, those of an
    earlier call (outcomes, tallies, lines, seen, mtallies).  Returns (states, accumulators, traces)."""
    kw = dict(common)
    for k in KINDS[1:KINDS.index(entry) + 1]:
        for name in OWN[k]:
            kw[name] = rec[name] if KINDS.index(k) <= KINDS.index(kind) else None
    if "lines" in _accepts(entry):
        kw["lines"] = rec["lines"]
    if carry:
        kw.update({n: carry[n] for n in ["outcomes"] + _accepts(entry)})
    r = getattr(s, "loop_run_" + entry)(st, ticks, **kw)
    return r[0], r[1:1 + NACC[entry]], r[1 + NACC[entry]:]


def test_a_higher_entry_point_with_a_lower_kinds_records_is_that_kinds_call(pkg, lib, fleet):
    """Host buffers: states, the accumulators the kind's own entry point returns and both traces are its bytes from every entry
    point above it; the accumulators of the kinds that are absent come back as they were given."""
    s, st, rec, common = fleet
    given = dict(zip(("outcomes", "tallies", "lines", "seen", "mtallies"),
                     (pkg.loop_outcomes(B, lib), pkg.ground_tallies(B), rec["lines"], pkg.sense_seen(B), pkg.motor_tallies(B, lib))))
    wants = []
    for ki, kind in enumerate(KINDS[:-1]):
        want = _call(s, kind, kind, st, T, rec, common)
        wants.append(want[0])
        assert (want[0]["tick"] == T).all()
        for entry in KINDS[ki + 1:]:
            got = _call(s, entry, kind, st, T, rec, common)
            assert _same(got[0], want[0]) and _all_same(got[1][:NACC[kind]], want[1]) and _all_same(got[2], want[2]), (kind, entry)
            for acc, name in list(zip(got[1], given))[NACC[kind]:]:
                assert _same(acc, given[name]), (kind, entry, name)
    # (the kinds differ from one another on this fleet: the chain is not compared on records that do nothing)
    assert all(not _same(a, b) for a, b in zip(wants, wants[1:]))


def test_the_motors_call_on_device_buffers_with_a_lower_kinds_records(pkg, lib, fleet):
    """Device buffers, once per kind: qmpc_loop_run_motors_device with the kind's records and 0 above them writes the bytes of the
    kind's own host-buffer call."""
    import torch

    s, st, rec, common = fleet
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1).copy()).cuda()      # noqa: E731
    fresh = dict(outcomes=pkg.loop_outcomes(B, lib), tallies=pkg.ground_tallies(B), lines=rec["lines"], seen=pkg.sense_seen(B),
                 mtallies=pkg.motor_tallies(B, lib))
    for ki, kind in enumerate(KINDS):
        want = _call(s, kind, kind, st, T, rec, common)
        has = lambda k: ki >= KINDS.index(k)      # noqa: E731,B023
        d = {n: dev(a) for n, a in list(rec.items()) + list(fresh.items()) + [("st", st), ("ctrl", common["ctrl"]), ("plant", common["plant"])]}
        d_tf = torch.full((T, B, 12), 7.0, dtype=torch.float64, device="cuda")
        d_tc = torch.full((T, B, 4), 7.0, dtype=torch.float64, device="cuda")
        ptr = lambda n, k: d[n].data_ptr() if has(k) else 0      # noqa: E731,B023
        torch.cuda.synchronize()
        s.loop_run_motors_device(B, d["st"].data_ptr(), T, d["outcomes"].data_ptr(), ptr("motor", "motors"), ptr("mtallies", "motors"), None,
                                 ptr("gait", "gaits"), ptr("sense", "sensing"), ptr("seen", "sensing"), ptr("act", "actuation"),
                                 ptr("lines", "actuation"), ptr("ground", "ground"), ptr("tallies", "ground"), ptr("push", "pushes"),
                                 rec["push"].shape[1] if has("pushes") else 0, common["lp"], common["op"], d_ctrl=d["ctrl"].data_ptr(),
                                 d_plant=d["plant"].data_ptr(), d_trace_forces=d_tf.data_ptr(), d_trace_contacts=d_tc.data_ptr())
        s.wait()
        out = [d[n].cpu().numpy() for n in ("outcomes", "tallies", "lines", "seen", "mtallies")]
        assert _same(d["st"].cpu().numpy(), want[0]) and _all_same(out[:NACC[kind]], want[1]), kind
        assert _same(d_tf.cpu().numpy(), want[2][0]) and _same(d_tc.cpu().numpy(), want[2][1]), kind
        assert all(_same(o, fresh[n]) for o, n in list(zip(out, fresh))[NACC[kind]:]), kind      # what the call does not have is not touched


def test_all_seven_kinds_equal_the_call_split_in_two(pkg, lib, fleet):
    """The motors call with every kind of record, 3 ticks at once against 1 tick and then 2 from where it stopped."""
    s, st, rec, common = fleet
    want = _call(s, "motors", "motors", st, T, rec, common)
    names = ("outcomes", "tallies", "lines", "seen", "mtallies")
    a = _call(s, "motors", "motors", st, 1, rec, common)
    b = _call(s, "motors", "motors", a[0], T - 1, rec, common, carry=dict(zip(names, a[1])))
    assert _same(b[0], want[0]) and _all_same(b[1], want[1])
    assert all(_same(np.concatenate([x, y]), w) for x, y, w in zip(a[2], b[2], want[2]))
    assert (want[1][4]["peak_tau"].max(axis=1) > 0).all() and not _same(a[0], want[0])
