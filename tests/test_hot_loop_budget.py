"""What the two hot loops of round 12 hold as compiled (tools/loop_census.py; CPU only, hipcc cross-compiles).

The matcher's tile loop (match_knn2_fp4_kernel<1, true, 2, 0>, the basic block with the MFMAs) and the solve kernel's
written-out Jacobi visits lost instructions that no source line asked for (a quieting `v_max_f32 vN, vN, vN` per running
maximum) or that one expression serves as well (the two selected quotients of jacobi_pair_9).  A compiler is free to put
either back; this holds the outcome, as tests/test_solve_kernel_resources.py holds the solve kernel's registers."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import loop_census as lc  # noqa: E402

CENSUS = os.path.join(ROOT, "profiles", "r12_loop_census.txt")
SOLVE_VISITS = 28          # jacobi_sweep_8x9_regs: every (i, j), 0 <= i < j < 8, written out once


def test_census_parser():
    asm = """\t.text
_ZN1a9other_kerEv:
\tv_max_f32_e32 v1, v1, v1
\ts_endpgm
.Lfunc_end0:
_ZN1a6my_kerILi1EEEvPf:                 ; @_ZN1a6my_kerILi1EEEvPf
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tv_mov_b32_e32 v2, 0                     ; a comment, with v_max_f32 v9, v9, v9 in it
\ts_cbranch_scc1 .LBB1_3
; %bb.1:
\tv_cndmask_b32_e32 v3, v4, v5, vcc
.LBB1_2:                                ; =>This Inner Loop Header: Depth=1
\tds_read_b128 v[4:7], v2
\tv_mfma_scale_f32_32x32x64_f8f6f4 v[0:15], v[16:23], v[24:31], v[0:15], v40, v41 op_sel_hi:[0,0,0]
\tv_max_f32_e32 v9, v9, v9
\tv_max_f32_e32 v10, v9, v9
\tv_max_f32_e32 v9, v9, v8
\tv_med3_f32 v11, v9, v9, v9
\tv_add_f32_e32 v12, v12, v12
\tv_pk_max_f16 v13, v13, v13
\tglobal_load_dword v14, v[0:1], off
\ts_cbranch_scc0 .LBB1_2
.LBB1_3:
\ts_endpgm
.Lfunc_end1:
\t.size x, 4
"""
    sym, bl = lc.census(None, "my_kerILi1E", asm)
    assert sym == "_ZN1a6my_kerILi1EEEvPf"
    assert [b["label"] for b in bl] == ["entry", "entry+", ".LBB1_2", ".LBB1_3"]
    entry, second, loop, last = bl
    assert (entry["n"], entry["mem"], entry["valu"], entry["salu"], entry["self"]) == (3, 1, 1, 1, 0)
    assert (second["n"], second["cnd"], second["valu"]) == (1, 1, 1)
    # med3 and add are not idempotent: v_add v, v, v doubles, and a median of one register is no max / min form
    assert (loop["n"], loop["lds"], loop["mfma"], loop["mem"], loop["salu"]) == (10, 1, 1, 1, 1)
    assert (loop["valu"], loop["self"], loop["dup"], loop["loop"]) == (6, 2, 1, True)
    assert not entry["loop"] and (last["n"], last["salu"]) == (1, 1)
    t = lc.totals(bl)
    assert (t["n"], t["valu"], t["cnd"]) == (15, 8, 1)
    text = "#### BEFORE\n" + lc.format_census("mine", sym, bl) + "\n#### AFTER\n" + lc.format_census("mine", sym, bl[:2])
    assert lc.parse_totals(text.split("#### AFTER")[0], "mine") == t
    assert lc.parse_totals(text, "mine")["n"] == 4


@pytest.fixture(scope="module")
def matcher_blocks():
    return lc.census("match.hip", "match_knn2_fp4_kernelILi1ELb1ELi2ELi0E")[1]


def test_matcher_tile_loop(matcher_blocks):
    """The tile loop is the one block with MFMAs: 2 tiles x 4 K-steps = 8.  Per trip a lane closes 2 tiles x 16 results: per result
    one fma (the key), one v_med3_f32 and one v_max_f32, 32 of each at most.  The parent's
    loop held 122 vector instructions, 16 of them v_max_f32 of a register with itself (profiles/r12_loop_census.txt, BEFORE);
    the bound is that count less those 16: 106.  It is derived, not read off the code under test."""
    mf = [b for b in matcher_blocks if b["mfma"]]
    assert len(mf) == 1, [(b["label"], b["mfma"]) for b in mf]
    loop = mf[0]
    print(loop)
    with open(CENSUS) as f:
        before = f.read().split("#### AFTER")[0]
    parent = [ln.split() for ln in before.split("== match_knn2_fp4  (")[1].split("\n== ")[0].splitlines()]
    parent = [f for f in parent if len(f) >= 10 and f[0] != "total" and f[1].isdigit() and int(f[6]) > 0]      # f[6]: the mfma column
    assert len(parent) == 1 and int(parent[0][2]) == 122 and int(parent[0][7]) + int(parent[0][8]) == 16, parent
    assert loop["mfma"] == 8
    assert loop["self"] == 0 and loop["dup"] == 0
    assert loop["valu"] <= 122 - 16, loop["valu"]


def test_matcher_has_no_quieting_max_anywhere(matcher_blocks):
    t = lc.totals(matcher_blocks)
    assert t["self"] == 0 and t["dup"] == 0, t


def test_solve_kernel_selects():
    """jacobi_pair_9 selected the first quotient's numerator and denominator between the two signs of beta: two f64 selects,
    four v_cndmask_b32, in each of the 28 written-out visits.  With the one expression for both signs the kernel's symbol holds
    at most the parent's count (the committed census, BEFORE) less 4 x 28."""
    with open(CENSUS) as f:
        before = f.read().split("#### AFTER")[0]
    parent = lc.parse_totals(before, "ransac_solve<false,4>")
    assert parent["cnd"] == 1057, parent        # the file is the record of the parent: it does not move with the code
    _, bl = lc.census("ransac_solve.hip", "ransac_solve_kernelILb0ELi4E")
    t = lc.totals(bl)
    print(t)
    assert t["cnd"] <= parent["cnd"] - 4 * SOLVE_VISITS, (t["cnd"], parent["cnd"])
    assert t["self"] == 0
