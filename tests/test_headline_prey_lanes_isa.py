"""The prey trials of the map-10 rollout step, one (prey, trial) pair per lane (pp10::step): the step loop of the
headline build (rollout_w_kernel<2, true, true, false, true, 1>) used to hold prey j's four trials one after the other, 37
instructions each, replayed by all 16 lanes of the env's group.  With lane sl on trial sl >> 2 of prey sl & 3 one trial body is
left, plus the combine (three row-shift DPP moves and the selects behind them).  Pins the instruction and VALU counts of the step
loop at what the build reached - were the compiler to serialise the trials again, they would be back at the parent's - and holds
every SHAPE 1 build and the probe entry to no scratch and no spill.  Needs hipcc, no GPU."""
import pytest

from tests import isa

HEADLINE = "_ZN2cm16rollout_w_kernelILi2ELb1ELb1ELb0ELb1ELi1EEE"       # <LHOPS 2, PRE, FULLWG, !TAPE, CARRY, SHAPE 1>
PARENT_INSTS = 3367                                                    # the step loop with the serial trials

SHAPE1 = [
    ("cm_rollout_w", "_ZN2cm22rollout_w_probe_kernelE"),
    ("cm_rollout_w", "_ZN2cm16rollout_w_kernelILi1ELb1ELb1ELb0ELb1ELi1EEE"),
    ("cm_rollout_w", "_ZN2cm16rollout_w_kernelILi1ELb1ELb0ELb0ELb1ELi1EEE"),
    ("cm_rollout_w", HEADLINE),
    ("cm_rollout_w", "_ZN2cm16rollout_w_kernelILi2ELb1ELb0ELb0ELb1ELi1EEE"),
    ("cm_rollout_wm", "_ZN2cm17rollout_wm_kernelILi1ELb1ELb1ELb1ELi1EEE"),
    ("cm_rollout_wm", "_ZN2cm17rollout_wm_kernelILi1ELb1ELb0ELb1ELi1EEE"),
    ("cm_rollout_wm", "_ZN2cm17rollout_wm_kernelILi2ELb1ELb1ELb1ELi1EEE"),
    ("cm_rollout_wm", "_ZN2cm17rollout_wm_kernelILi2ELb1ELb0ELb1ELi1EEE"),
]


def _row_shifts(loop):
    return sum(1 for ln in loop if ln.startswith("v_mov_b32_dpp") and "row_shl:" in ln)


def test_headline_step_loop_holds_one_trial_body():
    k = isa.kernel(isa.listing("cm_rollout_w"), HEADLINE)
    loop = isa.step_loop(k.lines)
    n = isa.counts(loop)
    print("headline step loop:", n, "row-shift DPP moves", _row_shifts(loop))
    assert n["mfma"] >= 288, n                  # the loop found is the step (the whole policy tile sits inside it)
    assert n["insts"] <= PARENT_INSTS - 80, n   # three 37-instruction trial bodies less an allowance for the combine
    assert n["insts"] <= 3278, n                # as built (3 367 before)
    assert n["valu"] <= 2303, n                 # as built (2 382 before)
    assert _row_shifts(loop) == 3               # the codes of lanes j + 4, j + 8 and j + 12


@pytest.mark.parametrize("unit,prefix", SHAPE1)
def test_shape1_builds_have_no_scratch_and_no_spill(unit, prefix):
    k = isa.kernel(isa.listing(unit), prefix)
    loop = isa.step_loop(k.lines)
    print(prefix, isa.counts(loop), "row-shift DPP moves", _row_shifts(loop))
    assert isa.counts(loop)["mfma"] >= 252      # the loop found is the step (a hop is 24 MFMAs of 16x16x32 and 12 of 16x16x16)
    assert k.private_segment_fixed_size == 0
    assert k.vgpr_spill_count == 0
    assert not any(ln.startswith("scratch_") for ln in k.lines)
    assert _row_shifts(loop) == 3               # every SHAPE 1 build shares the step
