"""tools/isa_loops.py on a hand-written listing: loops from back edges, classes, the remainder of the iteration."""
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent

LISTING = """
_Z6kernelv:                             ; @_Z6kernelv
	s_load_dwordx2 s[0:1], s[4:5], 0x0
.LBB0_1:                                ; iteration
	v_mul_f64 v[0:1], v[0:1], v[2:3]
	s_waitcnt lgkmcnt(0)
.LBB0_2:                                ; backward knot
	v_mfma_f64_16x16x4_f64 v[8:15], v[0:1], v[2:3], v[8:15]
	s_nop 7
	v_mov_b64_dpp v[4:5], v[0:1] row_newbcast:3 row_mask:0xf bank_mask:0xf bound_ctrl:1
	v_mov_b32_dpp v6, v0 row_shl:6 row_mask:0xf bank_mask:0xf bound_ctrl:1
	v_fmac_f64_dpp v[0:1], v[2:3], v[4:5] row_newbcast:4 row_mask:0xf bank_mask:0xf
	v_cndmask_b32_e64 v7, 0, v6, s[2:3]
	ds_bpermute_b32 v6, v7, v6
	s_cbranch_scc1 .LBB0_2
	v_add_f64 v[0:1], v[0:1], v[2:3]
.LBB0_3:                                ; rollout knot
	v_readlane_b32 s2, v0, 0
	v_readlane_b32 s3, v1, 0
	v_readlane_b32 s6, v0, 1
	v_readlane_b32 s7, v1, 1
	v_readlane_b32 s8, v0, 2
	v_readlane_b32 s9, v1, 2
	v_readlane_b32 s10, v0, 3
	v_readlane_b32 s11, v1, 3
	v_fma_f64 v[0:1], s[2:3], v[2:3], v[0:1]
	ds_read_b64 v[2:3], v6
	s_cbranch_scc1 .LBB0_3
	ds_write_b64 v6, v[0:1]
	s_cbranch_scc1 .LBB0_1
	s_endpgm
.Lfunc_end0:
; NumVgprs: 16
; ScratchSize: 0
"""


def test_loops_and_classes(tmp_path):
    f = tmp_path / "k.s"
    f.write_text(LISTING)
    out = subprocess.run([sys.executable, str(REPO / "tools" / "isa_loops.py"), str(f), "kernel", "1"],
                         check=True, capture_output=True, text=True).stdout
    lines = out.splitlines()
    bw = next(i for i, l in enumerate(lines) if l.startswith("backward pass, one knot (loop at .LBB0_2)"))
    assert "8 instructions, 2 FP64 arithmetic (1 MFMA), 6 other" in lines[bw]
    for cls in ("mfma 1", "f64_arith_dpp 1", "dpp_mov_b64 1", "dpp_mov_b32 1", "v_cndmask 1", "ds_bpermute 1", "s_nop 1", "s_branch 1"):
        assert cls in lines[bw + 1], cls
    ro = next(i for i, l in enumerate(lines) if l.startswith("trial rollout, knot loop body (loop at .LBB0_3"))
    assert "11 instructions, 1 FP64 arithmetic (0 MFMA), 10 other" in lines[ro]
    assert "v_readlane 8" in lines[ro + 1]
    it = next(i for i, l in enumerate(lines) if l.startswith("one iteration outside its loops (loop at .LBB0_1"))
    # v_mul, s_waitcnt | v_add | ds_write, s_cbranch
    assert "5 instructions, 2 FP64 arithmetic (0 MFMA), 3 other" in lines[it]
    assert "ScratchSize: 0" in out and "NumVgprs: 16" in out
