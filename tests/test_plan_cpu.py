"""CPU suite: the kernel planner (quaternion-mpc_amd/csrc/qmpc_plan.h) over its whole input space.

tests/native/plan_host.cpp enumerates every model and mode, the horizons qmpc_create accepts, the knob sets the tests use
and one setting of every other selection knob, the batch sizes around every switch-over and every kind of call, and
prints the plan of each; the table must equal tests/golden/kernel_plans.txt.gz byte for byte, and every plan must name a
kernel of its unit's launch table.  The harness is compiled host-only by hipcc (the layout headers are HIP
source); no device is needed.  Regenerate the table only for an intended change of the choice:
    python tests/test_plan_cpu.py --write"""
import gzip
import subprocess
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
SRC = HERE / "native" / "plan_host.cpp"
GOLDEN = HERE / "golden" / "kernel_plans.txt.gz"
HIPCC = "/opt/rocm/bin/hipcc"


def build(out_dir: Path) -> Path:
    exe = out_dir / "plan_host"
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-o", str(exe), str(SRC)], check=True)
    return exe


def test_plans_match_the_golden_table(tmp_path):
    table = subprocess.run([str(build(tmp_path))], check=True, capture_output=True).stdout
    golden = gzip.decompress(GOLDEN.read_bytes())
    if table != golden:
        got, want = table.decode().splitlines(), golden.decode().splitlines()
        first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        section = next((want[j] for j in range(min(first, len(want) - 1), -1, -1) if want[j].startswith("# ")), "")
        raise AssertionError(f"plan table differs from line {first + 1} ({section}): got {got[first:first + 1]}, "
                             f"want {want[first:first + 1]} ({len(got)} against {len(want)} lines)")


def test_every_plan_names_a_kernel(tmp_path):
    """Every plan of the enumeration (and of the per-instance solve and loop on the same configurations) names a kernel its
    unit instantiates: the launchers' slot of quaternion-mpc_amd/csrc/qmpc_kernel_slots.h exists."""
    r = subprocess.run([str(build(tmp_path)), "--kernels"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    assert " 0 without a kernel" in r.stdout, r.stdout


if __name__ == "__main__" and sys.argv[1:] == ["--write"]:
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        table = subprocess.run([str(build(Path(d)))], check=True, capture_output=True).stdout
    GOLDEN.write_bytes(gzip.compress(table, compresslevel=9, mtime=0))
    print(f"wrote {GOLDEN} ({len(table.splitlines())} lines)")
