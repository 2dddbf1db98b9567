"""LDS reads of the headline rollout step (rollout_w_kernel<2, true, true, false, true, 1>) after the lean policy tile of the map-10
builds: the two small head layers (64 -> 32 -> logits) live in AGPRs beside the 128 -> 64 layer and the MFMAs name
them there (no copies in front), so their 12 ds_read_b128 per step are gone; the register peak is lower (the look-ahead batches of
e2 and of the attention layer are requested at the middle of the layer that runs meanwhile), which is what lets every layer's bias
reads go in front of the fragment batch they used to queue behind without spill copies.  Pins the counts of the step loop this
reached, on the ISA hipcc emits with the Makefile's flags.  Needs hipcc, no GPU."""
from tests import isa

HEADLINE = "_ZN2cm16rollout_w_kernelILi2ELb1ELb1ELb0ELb1ELi1EEE"       # <LHOPS 2, PRE, FULLWG, !TAPE, CARRY, SHAPE 1>
PROBE = "_ZN2cm22rollout_w_probe_kernelE"                              # the same build with the COMMARL_ENV_STOP < 0 clocks


def _loop(prefix):
    k = isa.kernel(isa.listing("cm_rollout_w"), prefix)
    n = isa.counts(isa.step_loop(k.lines))
    print(prefix, n)
    assert k.private_segment_fixed_size == 0
    assert k.vgpr_spill_count == 0
    return n


def test_headline_step_loop_lds_reads():
    n = _loop(HEADLINE)
    assert n["mfma"] >= 288, n                  # the loop found is the step (the whole policy tile sits inside it)
    assert n["ds_read_b128"] <= 167, n          # 179 before: 12 fewer, the fragments of h3 (8) and h4 (4)
    assert n["mfma_agpr_src"] >= 66, n          # 48 before: + 4 x 3 (h3) + 2 x 3 (h4) MFMAs that read their A operand from AGPRs
    assert n["insts"] <= 3391, n                # 3 438 before
    # what the lower register peak left of the spill copies and the padding (21 / 1 / 96 before), and the vector ALU count
    # (2 393 before: + 4, address arithmetic of the moved reads)
    assert n["accvgpr_read"] <= 11, n
    assert n["accvgpr_write"] <= 0, n
    assert n["s_nop"] <= 76, n
    assert n["valu"] <= 2397, n
    assert n["salu"] <= 465, n                  # 502 before
    assert n["readlane"] <= 82, n               # 83 before


def test_probe_entry_lds_reads():
    n = _loop(PROBE)
    assert n["mfma"] >= 288, n
    assert n["ds_read_b128"] <= 167, n
    assert n["mfma_agpr_src"] >= 66, n
