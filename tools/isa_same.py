#!/usr/bin/env python3
"""Does every gfx950 function of the library compile to the instructions it had at another revision?

    python tools/isa_same.py [--base REV]        (default HEAD; no GPU needed)

The sources of REV (quaternion-mpc_amd/csrc and include, through `git archive`: no checkout) go to a temporary directory in
their relative layout.  Every translation unit of __graft_entry__.hip_units() is compiled from both trees with the unit's
flags and -S --cuda-device-only, each listing is cut into its functions, and the functions are compared in emission order
after dropping comments and directives (a kernel keeps the .amdhsa_ lines of its descriptor: registers, scratch, kernarg
size) and replacing every mangled name by a placeholder, so that renaming a kernel is no difference.  One row per function,
`same` or `DIFF (n lines)`; the exit status is non-zero on any DIFF or where a unit's function count differs.  The tool only
diffs two listings: it looks for nothing in them."""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
from __graft_entry__ import hip_units  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
MANGLED = re.compile(r"_Z[\w.$]+")


def listing(csrc: Path, name: str, flags, out: Path) -> str:
    if not (csrc / (name + ".hip")).exists():
        return ""      # a unit the revision does not have: no functions, a different count
    subprocess.run([HIPCC, *flags, "-S", "--cuda-device-only", "-o", str(out), str(csrc / (name + ".hip"))], check=True,
                   stderr=subprocess.DEVNULL)
    return out.read_text()


def functions(txt: str):
    """[(symbol, normalised lines)] in emission order"""
    lines = txt.split("\n")
    desc = {}       # kernel symbol -> the lines of its descriptor
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel", txt, re.M | re.S):
        desc[m.group(1)] = [l.strip() for l in m.group(2).split("\n") if l.strip()]
    out, cur, body = [], None, []
    for l in lines:
        m = re.match(r"^\t\.type\t(\S+),@function", l)
        if m:
            cur, body = m.group(1), []
            continue
        if cur is None:
            continue
        if l.startswith(".Lfunc_end"):
            out.append((cur, [MANGLED.sub("<sym>", x) for x in body + desc.get(cur, [])]))
            cur = None
            continue
        l = l.split(";", 1)[0].rstrip()
        if not l.strip() or l.lstrip().startswith(".") and not l.rstrip().endswith(":"):
            continue      # blank, comment or directive (a local label ends with a colon and stays)
        body.append(l.strip())
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--base", default="HEAD", help="the revision to compare the working tree against")
    a = ap.parse_args()
    rev = subprocess.run(["git", "-C", str(REPO), "rev-parse", "--short", a.base], check=True, capture_output=True, text=True).stdout.strip()
    bad = 0
    with tempfile.TemporaryDirectory() as d:
        d = Path(d)
        tar = subprocess.run(["git", "-C", str(REPO), "archive", a.base, "quaternion-mpc_amd/csrc", "include"], check=True, capture_output=True).stdout
        (d / "base").mkdir()
        subprocess.run(["tar", "-x", "-C", str(d / "base")], input=tar, check=True)
        trees = {"base": d / "base" / "quaternion-mpc_amd" / "csrc", "tree": REPO / "quaternion-mpc_amd" / "csrc"}
        units = hip_units()
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
            jobs = {(n, t): ex.submit(listing, c, n, f, d / f"{t}_{n}.s") for n, _, f in units for t, c in trees.items()}
            txt = {k: j.result() for k, j in jobs.items()}
    print(f"device code of the working tree against {rev}: hipcc <unit flags> -S --cuda-device-only, per function, comments and directives dropped, mangled names replaced")
    for n, _, f in units:
        old, new = functions(txt[(n, "base")]), functions(txt[(n, "tree")])
        names = subprocess.run(["c++filt"], input="\n".join(s for s, _ in new), capture_output=True, text=True).stdout.split("\n")
        print(f"---- {n}.hip ({' '.join(f)}): {len(new)} functions" + ("" if len(old) == len(new) else f", {len(old)} at {rev}: DIFF"))
        bad += len(old) != len(new)
        for (_, lo), (_, ln), name in zip(old, new, names):
            name = re.sub(r"\(.*", "", name).replace("void ", "")
            nd = sum(1 for x in difflib.unified_diff(lo, ln, lineterm="", n=0) if x[:1] in "+-" and x[:3] not in ("+++", "---"))
            bad += nd > 0
            print(f"{name} | {len(ln)} lines | " + (f"DIFF ({nd} lines)" if nd else "same"))
    print("all same" if not bad else f"{bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
