"""tools/isa_regions.py on a short hand-written listing: the exec-mask regions, branches, basic blocks and FP64 arithmetic it
counts per loop of the iteration and for the straight-line remainder, and the kernel-wide count of fma / fmac / mul / add."""
import importlib.util
import subprocess
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
TOOL = REPO / "tools" / "isa_regions.py"

# One kernel shaped like the wave kernel: an iteration loop (.LBB1_1) around a loop with MFMA (.LBB1_2), a lane-parallel loop
# (.LBB1_3) with a short-circuit `a && (b || c)` as the compiler lays it out (two nested regions, the inner one skipped when
# no lane is left), a straight-line remainder with an if / else (s_and_saveexec, s_or_saveexec) and a tail (.LBB1_9) that
# starts inside the iteration and is laid out behind its back edge.  A second kernel stands in front of it: the tool must
# pick the kernel by name.
LISTING = """\
	.text
_Z5otherPd:                             ; @_Z5otherPd
	v_mul_f64 v[0:1], v[2:3], v[4:5]
	s_and_saveexec_b64 s[0:1], vcc
	v_add_f64 v[0:1], v[0:1], v[4:5]
	s_endpgm
.Lfunc_end0:
_Z6kernelPd:                            ; @_Z6kernelPd
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	v_mul_f64 v[50:51], v[2:3], v[4:5]
	s_waitcnt lgkmcnt(0)
.LBB1_1:                                ; the iteration
	v_mov_b32_e32 v9, 0
.LBB1_2:                                ; the loop with MFMA
	ds_read_b64 v[0:1], v10
	s_waitcnt lgkmcnt(0)
	v_mfma_f64_16x16x4_f64 v[40:47], v[0:1], v[2:3], v[40:47]
	s_cbranch_scc1 .LBB1_2
; %bb.3:
	v_rcp_f64_e32 v[6:7], v[8:9]
.LBB1_3:                                ; up = a && (b || c), with short-circuit evaluation
	v_cmp_gt_f64_e32 vcc, 0, v[20:21]
	s_and_saveexec_b64 s[2:3], vcc
	s_cbranch_execz .LBB1_6
; %bb.4:
	v_cmp_neq_f64_e32 vcc, 0, v[22:23]
	s_and_saveexec_b64 s[6:7], vcc
; %bb.5:
	v_mul_f64 v[24:25], v[26:27], v[22:23]
	v_fma_f64 v[28:29], v[30:31], v[20:21], v[24:25]
	s_or_b64 exec, exec, s[6:7]
.LBB1_6:
	s_or_b64 exec, exec, s[2:3]
	v_fmac_f64_e32 v[32:33], v[28:29], v[6:7]
	v_max_f64 v[34:35], v[32:33], v[32:33]
	s_cbranch_execnz .LBB1_3
; %bb.7:
	v_cmp_lt_f64_e32 vcc, v[34:35], v[36:37]
	s_and_saveexec_b64 s[2:3], vcc
	s_xor_b64 s[2:3], exec, s[2:3]
	v_add_f64 v[34:35], v[34:35], v[36:37]
	s_or_saveexec_b64 s[2:3], s[2:3]
	s_xor_b64 exec, exec, s[2:3]
	v_mov_b32_e32 v34, 0
	s_or_b64 exec, exec, s[2:3]
.LBB1_9:                                ; the test at the loop's head, and the tail behind the back edge
	v_cmp_lt_f64_e32 vcc, v[20:21], v[24:25]
	s_cbranch_vccnz .LBB1_1
; %bb.10:
	v_add_f64 v[38:39], v[34:35], v[34:35]
	s_branch .LBB1_9
.Lfunc_end1:
	.size	_Z6kernelPd, .Lfunc_end1-_Z6kernelPd
"""


@pytest.fixture(scope="module")
def report():
    spec = importlib.util.spec_from_file_location("isa_regions", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, mod.analyse(LISTING.split("\n"), "_Z6kernel", 1)


def _summary(rep, label):
    return next(r for r in rep["regions"] if label in r["title"])["summary"]


def test_the_kernel_is_chosen_by_name_and_its_regions_are_the_iterations_loops(report):
    _, rep = report
    assert rep["kernel"] == "_Z6kernelPd"
    titles = [r["title"] for r in rep["regions"]]
    assert len(titles) == 3
    assert titles[0].startswith("backward pass, one knot at .LBB1_2")
    assert titles[1].startswith("loop at .LBB1_3")
    assert titles[2].startswith("one iteration outside its loops (at .LBB1_1")


def test_a_short_circuit_expression_is_two_regions_and_three_blocks(report):
    _, rep = report
    s = _summary(rep, ".LBB1_3")
    assert (s["instructions"], s["and_saveexec"], s["other_saveexec"]) == (12, 2, 0)
    assert (s["cbranch_exec"], s["cbranch_other"]) == (2, 0)      # the skip of the inner region and the back edge
    # leaders: the loop's head, what follows the skip, the skip's target .LBB1_6; the inner region is entered by falling
    # through (no branch, no target): it starts no block of its own
    assert s["blocks"] == 3
    assert s["f64_arith"] == 4      # mul, fma, fmac, max
    assert [at for at, _ in s["saveexec_at"]] == [1, 4]


def test_the_loop_with_mfma_is_one_block_with_a_uniform_back_edge(report):
    _, rep = report
    s = _summary(rep, ".LBB1_2")
    assert (s["instructions"], s["and_saveexec"], s["cbranch_exec"], s["cbranch_other"], s["blocks"], s["f64_arith"]) == (4, 0, 0, 1, 1, 1)


def test_the_remainder_holds_the_else_side_and_the_tail_behind_the_back_edge(report):
    _, rep = report
    s = _summary(rep, "outside its loops")
    # v_mov | v_rcp | the if / else (8) | the head's test (2) and the tail (2)
    assert s["instructions"] == 1 + 1 + 8 + 4
    assert (s["and_saveexec"], s["other_saveexec"]) == (1, 1)
    assert (s["cbranch_exec"], s["cbranch_other"]) == (0, 1)      # s_branch of the tail is no conditional branch
    assert s["f64_arith"] == 3      # rcp, the two adds
    # three straight-line pieces; inside the last one .LBB1_9 (a target) and what follows the branch to .LBB1_1
    assert s["blocks"] == 3 + 2


def test_totals_and_the_kernel_wide_arithmetic_count(report):
    _, rep = report
    t = rep["total"]
    assert (t["instructions"], t["and_saveexec"], t["other_saveexec"], t["cbranch_exec"], t["cbranch_other"]) == (30, 3, 1, 2, 2)
    assert (t["blocks"], t["f64_arith"]) == (9, 8)
    # fma / fmac / mul / add of the whole kernel, the prologue's mul included; rcp, max and MFMA are not in it
    assert rep["kernel_fma4"] == 6


def test_a_kernel_without_an_iteration_loop_is_reported_whole(report):
    mod, _ = report
    rep = mod.analyse(LISTING.split("\n"), "_Z5other", 1)
    assert [r["title"].split(" (")[0] for r in rep["regions"]] == ["one kernel outside its loops"]
    s = rep["regions"][0]["summary"]
    assert (s["instructions"], s["and_saveexec"], s["blocks"], s["f64_arith"]) == (4, 1, 1, 2)
    assert rep["kernel_fma4"] == 2


def test_command_line_lists_every_saveexec_unless_summary(tmp_path):
    f = tmp_path / "k.s"
    f.write_text(LISTING)
    out = subprocess.run([sys.executable, str(TOOL), str(f), "_Z6kernel", "1"], check=True, capture_output=True, text=True).stdout
    assert out.count("_saveexec_b64") == 4
    assert ("total: 30 instructions, 8 FP64 arithmetic; s_and_saveexec 3, other saveexec 1; s_cbranch_exec 2, other s_cbranch 2; "
            "9 basic blocks; v_fma/fmac/mul/add_f64 in the whole kernel 6") in out
    brief = subprocess.run([sys.executable, str(TOOL), str(f), "_Z6kernel", "1", "--summary"], check=True, capture_output=True, text=True).stdout
    assert brief.count("_saveexec_b64") == 0 and brief.strip().endswith(out.strip().split("\n")[-1])
