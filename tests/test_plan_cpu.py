"""CPU suite: the kernel planners (quaternion-mpc_amd/csrc/qmpc_plan.h) over their whole input space.

tests/native/plan_host.cpp enumerates every model and mode, the horizons qmpc_create accepts, the knob sets the tests use
and one setting of every other selection knob, the batch sizes around every switch-over and every kind of call, and
prints the plan of each; the table must equal tests/golden/kernel_plans.txt.gz byte for byte, and every plan must name a
kernel of its unit's launch table.  tests/native/records_plan_host.cpp does the same for the planners of the calls with
per-instance records (plan_instances, plan_convex_instances, plan_loop_instances) over every setting of a handle and every
fact of a call, against tests/golden/record_plans.txt.gz.  That table was generated from the planner while it still was a
chain of overloads, one per setting, over the whole product of the settings: it carries what the overloads' own tests
asserted pairwise, that a setting changes nothing while it is off.  The harnesses are compiled host-only by hipcc (the
layout headers are HIP source); no device is needed.  Regenerate the tables only for an intended change of the choice:
    python tests/test_plan_cpu.py --write"""
import gzip
import subprocess
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
SRC = HERE / "native" / "plan_host.cpp"
GOLDEN = HERE / "golden" / "kernel_plans.txt.gz"
RECORDS_SRC = HERE / "native" / "records_plan_host.cpp"
RECORDS_GOLDEN = HERE / "golden" / "record_plans.txt.gz"
HIPCC = "/opt/rocm/bin/hipcc"


def build(out_dir: Path, src: Path = SRC) -> Path:
    exe = out_dir / src.stem
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-o", str(exe), str(src)], check=True)
    return exe


def assert_table(exe: Path, golden_file: Path):
    table = subprocess.run([str(exe)], check=True, capture_output=True).stdout
    golden = gzip.decompress(golden_file.read_bytes())
    if table != golden:
        got, want = table.decode().splitlines(), golden.decode().splitlines()
        first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        section = next((want[j] for j in range(min(first, len(want) - 1), -1, -1) if want[j].startswith("# ")), "")
        raise AssertionError(f"plan table differs from line {first + 1} ({section}): got {got[first:first + 1]}, "
                             f"want {want[first:first + 1]} ({len(got)} against {len(want)} lines)")


def test_plans_match_the_golden_table(tmp_path):
    assert_table(build(tmp_path), GOLDEN)


def test_record_plans_match_the_golden_table(tmp_path):
    assert_table(build(tmp_path, RECORDS_SRC), RECORDS_GOLDEN)


def test_every_plan_names_a_kernel(tmp_path):
    """Every plan of the enumerations (and of the per-instance solve and loop on the same configurations) names a kernel its
    unit instantiates: the launchers' slot of quaternion-mpc_amd/csrc/qmpc_kernel_slots.h exists."""
    for src in (SRC, RECORDS_SRC):
        r = subprocess.run([str(build(tmp_path, src)), "--kernels"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr + r.stdout
        assert " 0 without a kernel" in r.stdout, r.stdout


if __name__ == "__main__" and sys.argv[1:] == ["--write"]:
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        for src, golden in ((SRC, GOLDEN), (RECORDS_SRC, RECORDS_GOLDEN)):
            table = subprocess.run([str(build(Path(d), src))], check=True, capture_output=True).stdout
            golden.write_bytes(gzip.compress(table, compresslevel=9, mtime=0))
            print(f"wrote {golden} ({len(table.splitlines())} lines)")
