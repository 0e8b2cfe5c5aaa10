"""Worker of tests/test_gpu_foothold_sets.py::test_device_closed_loop_on_displaced_footholds: runs the device-resident closed
loop on foothold_sets.loop_states (standing robots whose feet are displaced from the default footholds; drop_ang_vel = 0) and prints a SHA-256 of
the final states and of the force / contact traces.  The launch form is chosen by the environment (QMPC_LOOP_FUSED=0 per-tick
kernels, =1 persistent kernel), read once per process."""
import hashlib
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from conftest import load_pkg  # noqa: E402

import foothold_sets as F  # noqa: E402
import motion_sets as M  # noqa: E402

pkg = load_pkg()
ticks, horizon = int(sys.argv[1]), int(sys.argv[2])
lib = pkg.load_library()
lp = pkg.default_loop_params(lib)
st0 = F.loop_states(pkg, lib, lp)
s = pkg.Solver(M.params(pkg, "default_params", horizon, pkg.MODE_CONVERGED, lib), len(st0), device=0, lib=lib)
st, tf, tc = s.loop_run(st0, ticks, lp, trace=True)
s.close()
assert (st["tick"] == ticks).all()
print("SHA", hashlib.sha256(st.tobytes() + tf.tobytes() + tc.tobytes()).hexdigest())
