"""tools/isa_waits.py on a short hand-written listing: what it says about every lgkmcnt wait (batch size, distance to the
youngest read it covers, repeat groups), the AGPR move count and the regions it reports."""
import importlib.util
import subprocess
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
TOOL = REPO / "tools" / "isa_waits.py"

# One kernel shaped like the wave kernel: an iteration loop (.LBB0_1) around a loop with MFMA (.LBB0_2), a loop of
# "load, drain" groups (.LBB0_3), a straight-line remainder with one batch of three loads, and a tail (.LBB0_4) that
# starts inside the iteration and is laid out behind its back edge.  A second kernel stands in front of it: the tool
# must pick the kernel by name.
LISTING = """\
	.text
_Z5otherPd:                             ; @_Z5otherPd
	ds_read_b64 v[0:1], v2
	s_waitcnt lgkmcnt(0)
	s_endpgm
.Lfunc_end0:
_Z6kernelPd:                            ; @_Z6kernelPd
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	s_waitcnt lgkmcnt(0)
.LBB1_1:                                ; the iteration
	v_accvgpr_write_b32 a0, v1
	v_accvgpr_write_b32 a1, v2
.LBB1_2:                                ; the loop with MFMA
	ds_read_b64 v[0:1], v10
	v_add_u32_e32 v10, 8, v10
	v_add_u32_e32 v11, 8, v11
	s_waitcnt lgkmcnt(0)
	v_mfma_f64_16x16x4_f64 v[40:47], v[0:1], v[2:3], v[40:47]
	s_cbranch_scc1 .LBB1_2
; %bb.3:
	v_accvgpr_read_b32 v1, a0
.LBB1_3:                                ; load, drain, load, drain
	ds_read2_b64 v[2:5], v12 offset1:1
	s_waitcnt lgkmcnt(0)
	v_add_f64 v[30:31], v[2:3], v[4:5]
	ds_read2_b64 v[2:5], v12 offset0:2 offset1:3
	s_waitcnt lgkmcnt(0)
	v_add_f64 v[32:33], v[2:3], v[4:5]
	ds_read2_b64 v[2:5], v12 offset0:4 offset1:5
	s_waitcnt lgkmcnt(0)
	v_add_f64 v[34:35], v[2:3], v[4:5]
	s_cbranch_execnz .LBB1_3
; %bb.4:
	ds_read_b64 v[20:21], v13
	ds_read_b64 v[22:23], v13 offset:8
	ds_read_b64 v[24:25], v13 offset:16
	v_mov_b32_e32 v9, 0
	s_waitcnt lgkmcnt(1)
	v_add_f64 v[20:21], v[20:21], v[22:23]
	s_waitcnt vmcnt(0) lgkmcnt(0)
	ds_write_b64 v13, v[20:21]
	s_waitcnt lgkmcnt(0)
	s_waitcnt vmcnt(0)
.LBB1_4:                                ; the test at the loop's head, and the tail behind the back edge
	v_cmp_lt_f64_e32 vcc, v[20:21], v[24:25]
	s_cbranch_vccnz .LBB1_1
; %bb.5:
	v_accvgpr_read_b32 v2, a1
	ds_read_b64 v[36:37], v14
	v_nop
	v_nop
	v_nop
	v_nop
	v_nop
	v_nop
	v_nop
	s_waitcnt lgkmcnt(0)
	s_branch .LBB1_4
.Lfunc_end1:
	.size	_Z6kernelPd, .Lfunc_end1-_Z6kernelPd
"""


@pytest.fixture(scope="module")
def report():
    spec = importlib.util.spec_from_file_location("isa_waits", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, mod.analyse(LISTING.split("\n"), "_Z6kernel", 1)


def _region(rep, label):
    return next(r for r in rep["regions"] if label in r["title"])


def test_the_kernel_is_chosen_by_name_and_its_regions_are_the_iterations_loops(report):
    _, rep = report
    assert rep["kernel"] == "_Z6kernelPd"
    titles = [r["title"] for r in rep["regions"]]
    assert len(titles) == 3
    assert titles[0].startswith("backward pass, one knot at .LBB1_2")
    assert titles[1].startswith("loop at .LBB1_3")
    assert titles[2].startswith("one iteration outside its loops (at .LBB1_1")


def test_a_wait_directly_behind_its_load_and_the_repeat_groups(report):
    _, rep = report
    ws = _region(rep, ".LBB1_3")["waits"]
    assert [w["batch"] for w in ws] == [1, 1, 1]
    assert [w["dist"] for w in ws] == [0, 0, 0]
    assert [w["lgkmcnt"] for w in ws] == [0, 0, 0]
    assert [w["repeat"] for w in ws] == [False, True, True]      # the first group has nothing in front of it to repeat
    s = _region(rep, ".LBB1_3")["summary"]
    assert (s["waits"], s["close"], s["adjacent"], s["repeats"]) == (3, 3, 3, 2)


def test_the_distance_counts_the_instructions_between_read_and_wait(report):
    _, rep = report
    (w,) = _region(rep, ".LBB1_2")["waits"]
    assert (w["batch"], w["dist"], w["repeat"]) == (1, 2, False)
    s = _region(rep, ".LBB1_2")["summary"]
    assert (s["instructions"], s["close"], s["adjacent"]) == (6, 1, 0)


def test_a_counted_wait_leaves_the_youngest_loads_in_flight(report):
    _, rep = report
    ws = _region(rep, "outside its loops")["waits"]
    # lgkmcnt(1) behind three reads covers the first two: the second one stands two instructions in front of it (the third
    # read and a move); lgkmcnt(0) then retires the third (wait, add in between); the store's wait covers no read; the
    # tail's read stands seven instructions in front of its wait, which is not close
    assert [(w["lgkmcnt"], w["batch"], w["dist"]) for w in ws] == [(1, 3, 2), (0, 0, 3), (0, 1, None), (0, 1, 7)]
    assert not any(w["repeat"] for w in ws)
    s = _region(rep, "outside its loops")["summary"]
    assert (s["waits"], s["close"], s["adjacent"], s["repeats"]) == (4, 2, 0, 0)


def test_a_counted_wait_that_streams_is_no_repeat(report):
    mod, _ = report
    # one more load out, the oldest one in: every group is the previous group's, but each wait retires the read of the
    # group before -- nothing here could have been issued earlier
    seq = ["ds_read_b64 v[0:1], v9", "ds_read_b64 v[2:3], v9 offset:8", "s_waitcnt lgkmcnt(1)", "v_add_f64 v[10:11], v[0:1], 0"]
    for i in range(3):
        seq += [f"ds_read_b64 v[{4 + 2 * i}:{5 + 2 * i}], v9 offset:{16 + 8 * i}", "s_waitcnt lgkmcnt(1)", "v_add_f64 v[10:11], v[10:11], v[2:3]"]
    ws = mod.waits_of(seq)
    assert [(w["batch"], w["lgkmcnt"], w["dist"]) for w in ws] == [(2, 1, 1), (1, 1, 3), (1, 1, 3), (1, 1, 3)]      # (between: a wait, an add, the new read)
    assert not any(w["repeat"] for w in ws)


def test_agpr_moves_are_counted_per_region_and_in_total(report):
    _, rep = report
    s = _region(rep, "outside its loops")["summary"]
    assert (s["accvgpr_read"], s["accvgpr_write"]) == (2, 2)      # the tail behind the back edge is part of the iteration
    assert all(r["summary"]["accvgpr_read"] == 0 and r["summary"]["accvgpr_write"] == 0 for r in rep["regions"][:2])
    t = rep["total"]
    assert (t["accvgpr_read"], t["accvgpr_write"], t["waits"], t["repeats"]) == (2, 2, 8, 2)
    # the kernel's prologue (s_load and its wait) is outside the iteration: not in any region
    assert t["instructions"] == sum(r["summary"]["instructions"] for r in rep["regions"]) == 6 + 10 + 26


def test_a_kernel_without_an_iteration_loop_is_reported_whole(report):
    mod, _ = report
    rep = mod.analyse(LISTING.split("\n"), "_Z5other", 1)
    assert [r["title"].split(" (")[0] for r in rep["regions"]] == ["one kernel outside its loops"]
    (w,) = rep["regions"][0]["waits"]
    assert (w["batch"], w["dist"]) == (1, 0)


def test_command_line_prints_one_line_per_wait(tmp_path):
    f = tmp_path / "k.s"
    f.write_text(LISTING)
    out = subprocess.run([sys.executable, str(TOOL), str(f), "_Z6kernel", "1"], check=True, capture_output=True, text=True).stdout
    assert out.count("lgkmcnt(") == 8 and out.count("  repeat") == 2
    assert "total: 42 instructions, 8 lgkmcnt waits: 6 at most 6 behind their read (3 directly behind it), 2 repeats; " \
           "v_accvgpr_read 2, v_accvgpr_write 2" in out
    brief = subprocess.run([sys.executable, str(TOOL), str(f), "_Z6kernel", "1", "--summary"], check=True, capture_output=True, text=True).stdout
    assert brief.count("lgkmcnt(") == 0 and brief.strip().endswith(out.strip().split("\n")[-1])
