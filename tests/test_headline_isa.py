"""Instruction budget of the headline rollout step (PredatorPrey map 10, teams of 4, two hops, carried, full workgroups:
rollout_w_kernel<2, true, true, false, true, 1>).  That kernel runs ONE wave per SIMD, so every vector instruction of its step
loop is ~4 clk of the step; this pins the counts the step was brought down to, on the ISA hipcc emits with the
Makefile's flags.  Needs hipcc, no GPU."""
from tests import isa

HEADLINE = "_ZN2cm16rollout_w_kernelILi2ELb1ELb1ELb0ELb1ELi1EEE"       # <LHOPS 2, PRE, FULLWG, !TAPE, CARRY, SHAPE 1>


def test_headline_step_loop_instruction_budget():
    k = isa.kernel(isa.listing("cm_rollout_w"), HEADLINE)
    n = isa.counts(isa.step_loop(k.lines))
    print("headline step loop:", n)
    # the loop found must be the step: the whole policy tile (288 MFMAs: 264 of 16x16x32, 24 of 16x16x16) sits inside it
    assert n["mfma"] >= 288, n
    assert k.private_segment_fixed_size == 0
    assert k.vgpr_spill_count == 0
    # the resident 128 -> 64 layer (4 tiles x 4 k blocks x 3 products) is read by the MFMAs where it lives, in AGPRs ...
    assert n["mfma_agpr_src"] >= 48, n
    # ... so the copies in front of them are gone (158 before; what remains are ordinary spill reloads)
    assert n["accvgpr_read"] <= 30, n
    # 3 088 before; 2 959 with the copies gone; 2 658 with the split's residual written by v_fma_mixlo_f16 / v_fma_mixhi_f16
    # (no v_cvt_f32_f16 + v_sub_f32 per value, no second v_cvt_pk_f16_f32 per pair)
    assert n["valu"] <= 2658, n
    assert n["cvt_f32_f16"] == 0, n
