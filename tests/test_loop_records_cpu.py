"""CPU suite: the one record of a closed-loop call's per-robot arguments (quaternion-mpc_amd/csrc/qmpc_loop_records.h) without a device.

tests/native/loop_records_host.cpp compares loop_recs_normalise -- which call an entry point makes with the arguments it was
given -- with the delegation cascade the fourteen entry points were before, written out there as the oracle: eight entry kinds,
both chains, every presence combination of the pointers, pushes_per_robot 0 / 1 / QMPC_MAX_PUSHES / QMPC_MAX_PUSHES + 1, batch
0 and 2.  Compiled host-only by hipcc like tests/native/loop_motor_host.cpp, once plain and once with AddressSanitizer and
UndefinedBehaviorSanitizer, as a stand-alone program with its own main."""
import re
import subprocess
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
CSRC = REPO / "quaternion-mpc_amd" / "csrc"
SRC = HERE / "native" / "loop_records_host.cpp"
HIPCC = "/opt/rocm/bin/hipcc"


def test_normalise_equals_the_cascade_native(tmp_path):
    """The native program, plain and then with ASan + UBSan: a stand-alone program with its own main, no preloading."""
    text = SRC.read_text()
    assert re.findall(r'#include "([^"]+)"', text) == ["../../quaternion-mpc_amd/csrc/qmpc_loop_records.h"]      # (which includes include/qmpc.h)
    for tag, flags in (("plain", []), ("san", ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"])):
        exe = tmp_path / ("loop_records_host_" + tag)
        subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", *flags, "-o", str(exe), str(SRC)], check=True)
        r = subprocess.run([str(exe)], capture_output=True, text=True)
        print(tag, r.stdout, r.stderr)
        assert r.returncode == 0, r.stdout + r.stderr
        m = re.search(r"normalise against the cascade: (\d+) calls, (\d+) refused; made by kind((?: \d+){8})$", r.stdout, re.M)
        assert m and int(m.group(1)) == 633424 and 0 < int(m.group(2)) < int(m.group(1))
        assert all(int(k) > 0 for k in m.group(3).split())      # every kind of call is made by some case
        assert "passed: 0 failures" in r.stdout
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_the_header_is_plain_cpp_and_the_record_follows_the_abi_order():
    """No HIP header and no HIP call in the header (a host-only program includes it); the record's members stand in the order in
    which the entry points of include/qmpc.h take them, which the aggregate initialisers of qmpc_hip.hip rely on."""
    header = (CSRC / "qmpc_loop_records.h").read_text()
    assert not re.search(r'#include\s*[<"]hip|\bhip[A-Z]\w*\s*\(', header)
    fields = re.search(r"struct loop_recs \{(.*?)\n\};", header, re.S).group(1)
    assert re.findall(r"(\w+);", fields) == ["ctrl", "plant", "trace_forces", "trace_contacts", "op", "outcomes", "push", "per_robot", "ground",
                                             "tally", "act", "line", "sense", "seen", "gait", "geom", "motor", "mtally"]
