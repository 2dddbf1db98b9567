"""Scalar bookkeeping of the headline rollout step (rollout_w_kernel<2, true, true, false, true, 1>: one wave per SIMD, so every
instruction the wave issues, scalar ones included, is step time - DESIGN.md §5).  What the launcher has decided once per launch
(five actions sampled without a mask, every default output present, buffers below 2^31 bytes, no diagnostics) is folded into
the SHAPE 1 build: no per-step pointer rebuilds, no null tests, no probe sites, the state arrays written by the last step only.
Pins the counts of the step loop that this reached, on the ISA hipcc emits with the Makefile's flags.  Needs hipcc, no GPU."""
from tests import isa

HEADLINE = "_ZN2cm16rollout_w_kernelILi2ELb1ELb1ELb0ELb1ELi1EEE"       # <LHOPS 2, PRE, FULLWG, !TAPE, CARRY, SHAPE 1>
PROBE = "_ZN2cm22rollout_w_probe_kernelE"                              # the same build with the COMMARL_ENV_STOP < 0 clocks


def _tally(loop):
    n = isa.counts(loop)
    n["s_load"] = sum(1 for ln in loop if ln.startswith("s_load_"))
    n["v_lshl_add_u64"] = sum(1 for ln in loop if ln.startswith("v_lshl_add_u64"))
    n["s_memtime"] = sum(1 for ln in loop if ln.startswith("s_memtime"))
    n["s_getpc_b64"] = sum(1 for ln in loop if ln.startswith("s_getpc_b64"))
    return n


def test_headline_step_loop_scalar_budget():
    k = isa.kernel(isa.listing("cm_rollout_w"), HEADLINE)
    n = _tally(isa.step_loop(k.lines))
    print("headline step loop:", n)
    assert n["mfma"] >= 288, n                  # the loop found is the step (the whole policy tile sits inside it)
    assert k.private_segment_fixed_size == 0
    assert k.vgpr_spill_count == 0
    # the diagnostic clocks live in the probe entry only - nowhere in this kernel
    assert n["s_memtime"] == 0 and n["s_getpc_b64"] == 0, n
    assert k.count("s_memtime") == 0 and k.count("s_getpc_b64") == 0
    # strictly below what the step loop held before the launch constants were folded ...
    assert n["salu"] < 1043 and n["readlane"] < 153 and n["s_nop"] < 122, n
    assert n["s_load"] < 36 and n["v_lshl_add_u64"] < 39, n
    # ... and pinned where the fold brought them
    assert n["salu"] <= 502, n                  # 1 043 before
    assert n["readlane"] <= 83, n               # 153 before (reloads of spilled SGPRs)
    assert n["s_nop"] <= 96, n                  # 122 before
    assert n["s_load"] <= 32, n                 # 46 before, counted the same way (36 of them from the kernel-argument block)
    assert n["v_lshl_add_u64"] <= 5, n          # 39 before (64-bit store addresses per lane)


def test_probe_entry_has_the_clocks():
    k = isa.kernel(isa.listing("cm_rollout_w"), PROBE)
    n = _tally(isa.step_loop(k.lines))
    assert n["mfma"] >= 288, n
    assert n["s_memtime"] > 0, n
    assert k.private_segment_fixed_size == 0
    assert k.vgpr_spill_count == 0
