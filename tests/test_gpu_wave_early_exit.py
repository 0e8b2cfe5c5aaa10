"""GPU suite (-m gpu): the wave kernels' last pass.

A pass of the interior-point loop that ends the solve (converged, or the iteration cap reached) leaves before the
wrenches and expansions at the new iterate are formed.  What the solve reports must not depend on that: the test for
convergence after `iterations_max` passes (the `iterations_max + 1` pass) still runs, and `iterations`, `cost`,
`last_step`, `penalty` and the forces are those of the same iterate.  Both are checked without a tolerance, GPU against
GPU: a solve whose cap equals the number of passes an instance needs is the same solve as an uncapped one.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()   # raises if the HIP extension is missing: no fallback


# 64: everything in LDS, one wave per SIMD; 4096: gains and per-knot blocks in the workspace (the same body)
@pytest.mark.parametrize("batch", [64, 4096])
def test_cap_equal_to_the_passes_needed_changes_nothing(pkg, lib, batch):
    rec = pkg.random_go1_trot_states(batch, config_id=2)
    p = pkg.default_params(10, pkg.MODE_CONVERGED, lib)
    s = pkg.Solver(p, batch, device=0, lib=lib)
    f0, i0 = s.solve(rec)
    assert (i0["status"] == pkg.OK).all()
    n = i0["iterations"]
    cap = int(np.sort(n)[batch // 2])      # a pass count that occurs, from the middle of the batch
    assert (n > cap).any()                 # both sides of the cap are populated
    p.iterations_max = cap
    s.set_params(p)
    f1, i1 = s.solve(rec)
    s.close()
    done = n <= cap
    # converged within the cap, the last of them exactly AT the cap: the same solve, bit for bit
    assert (n[done] == cap).any()
    assert (i1["status"][done] == pkg.OK).all()
    for name in ("iterations", "cost", "max_violation", "last_step", "penalty"):
        assert np.array_equal(i1[name][done], i0[name][done]), name
    assert np.array_equal(f1[done], f0[done])
    # the others stop at the cap with the iterate of that pass
    assert (i1["status"][~done] == pkg.MAX_ITER).all()
    assert (i1["iterations"][~done] == cap).all()
    assert np.isfinite(f1).all()
