"""The fleets the GPU tests of the warm-started record loops walk, and their byte comparison (a helper module beside the tests,
like kkt_independent.py; not a test).  A fleet: the loop parameters with lp.warm_start set, B robots standing at their initial
poses (movement 0) and the commands they walk with afterwards."""
import numpy as np

COMMANDS = [   # joy.{velx, vely, body_height, roll_rate, pitch_rate, yaw_rate}, movement_mode
    [0.0, 0.0, 0.30, 0.0, 0.0, 0.0, 0.0],
    [0.3, 0.0, 0.30, 0.0, 0.0, 0.0, 1.0],
    [0.2, -0.1, 0.28, 0.0, 0.0, 0.3, 1.0],
    [0.0, 0.0, 0.30, 0.1, -0.1, 0.0, 1.0],
    [-0.2, 0.05, 0.32, 0.0, 0.0, -0.2, 1.0],
    [0.0, 0.0, 0.27, 0.0, 0.0, 0.0, 0.0],
]


def quat_fleet(pkg, lib, B, seed=1, trot=False):
    """the fleet of tests/test_gpu_loop_instances.py; trot: every robot walks"""
    lp = pkg.default_loop_params(lib)
    lp.warm_start = 1.0
    rng = np.random.default_rng(seed)
    cmds = np.array([COMMANDS[1 + i % 4] if trot else COMMANDS[i % len(COMMANDS)] for i in range(B)])
    cmds[:, 0] += rng.uniform(-0.1, 0.1, B) * cmds[:, 6]
    stand = cmds.copy(); stand[:, 6] = 0.0
    st = pkg.loop_states(stand, lp, height=0.3, yaw=rng.uniform(-3, 3, B), lib=lib)
    return lp, st, cmds


def convex_fleet(pkg, lib, B, seed=29):
    """the fleet and commands of tests/test_gpu_convex_loop_instance_lane.py"""
    rng = np.random.default_rng(seed)
    lp = pkg.default_loop_params(lib)
    lp.warm_start = 1.0
    cmds = np.zeros((B, 7))
    cmds[:, 0] = 0.6 * rng.uniform(-0.5, 0.5, B); cmds[:, 1] = rng.uniform(-0.2, 0.2, B); cmds[:, 2] = rng.uniform(0.26, 0.32, B)
    cmds[:, 5] = rng.uniform(-0.5, 0.5, B); cmds[:, 6] = (rng.random(B) < 0.9).astype(float)
    cmds[cmds[:, 6] == 0, :2] = 0.0
    cmds[cmds[:, 6] == 0, 5] = 0.0
    stand = cmds.copy(); stand[:, 6] = 0.0
    return lp, pkg.loop_states(stand, lp, height=0.3, yaw=rng.uniform(-3, 3, B), lib=lib), cmds


def walk(run, st, cmds, t0, t):
    """run(states, ticks, trace): t0 ticks standing, then t ticks under the commands' movement modes, traced"""
    st0 = run(st, t0, False)
    st0["movement_mode"] = cmds[:, 6]
    return run(st0, t, True)


def same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()
