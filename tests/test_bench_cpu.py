"""CPU suite: bench.py's launcher path.  `python bench.py --gpus N` without a launcher in the environment re-executes
itself under torch.distributed.run with one rank per GPU (the driver's multi-GPU call may be either form).  Here the
ranks stop after the rendezvous (QMPC_BENCH_DRYRUN, gloo): what is checked is the self-launch, the 127.0.0.1
rendezvous and that exactly one JSON line comes out of rank 0."""
import json
import os
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent


def _run(args, env_extra):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra)
    return subprocess.run([sys.executable, str(REPO / "bench.py"), *args], env=env, capture_output=True, text=True, timeout=300)


def test_plain_invocation_with_gpus_2_launches_two_ranks():
    r = _run(["--gpus", "2", "--steps", "2", "--warmup", "1"], {"QMPC_BENCH_DRYRUN": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out == {"dry_run": True, "n_gpus": 2, "sum_of_ranks": 3.0}


def test_launcher_mismatch_is_an_error():
    """a launcher that set another world size than --gpus says: refuse (exit code 2), do not guess"""
    r = _run(["--gpus", "4"], {"QMPC_BENCH_DRYRUN": "1", "WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 2


def test_steps_below_one_is_an_error():
    """--steps sets the number of timed steps and ms_per_step divides by it: zero steps is refused before any work"""
    r = _run(["--steps", "0"], {})
    assert r.returncode == 2 and "--steps" in r.stderr


def test_dump_outputs_writes_float64_and_samples_above_the_limit(pkg, tmp_path, monkeypatch):
    """--dump-outputs: one float64 array per output; above the size limit the same seeded sample of instances every
    time, rows.npy naming them, and the files together within the limit"""
    import importlib.util

    import numpy as np

    spec = importlib.util.spec_from_file_location("bench_under_test", REPO / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    rng = np.random.default_rng(1)
    forces = rng.standard_normal((1000, 12))
    info = np.zeros(1000, dtype=pkg.INFO_DTYPE)
    info["iterations"] = rng.integers(1, 30, 1000)
    info["cost"] = rng.standard_normal(1000)

    bench.dump_outputs(tmp_path / "all", forces, info)
    names = sorted(p.name for p in (tmp_path / "all").iterdir())
    assert names == sorted(["forces.npy"] + [f"info_{k}.npy" for k in pkg.INFO_DTYPE.names])
    assert np.array_equal(np.load(tmp_path / "all" / "forces.npy"), forces)
    it = np.load(tmp_path / "all" / "info_iterations.npy")
    assert it.dtype == np.float64 and np.array_equal(it, info["iterations"])

    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096 + 100 * (8 * 18 + 8))
    for d in ("a", "b"):
        bench.dump_outputs(tmp_path / d, forces, info)
    rows = np.load(tmp_path / "a" / "rows.npy")
    assert len(rows) == 100 and np.all(np.diff(rows) > 0)
    assert np.array_equal(rows, np.load(tmp_path / "b" / "rows.npy"))
    assert np.array_equal(np.load(tmp_path / "a" / "forces.npy"), forces[rows.astype(int)])
    assert np.array_equal(np.load(tmp_path / "a" / "info_cost.npy"), info["cost"][rows.astype(int)])
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= bench.DUMP_LIMIT_BYTES
