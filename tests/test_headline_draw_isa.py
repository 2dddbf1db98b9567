"""Philox work of the map-10 rollout step after the draw stage: the step loop of the headline build
(rollout_w_kernel<2, true, true, false, true, 1>) used to hold two complete Philox4x32-10 calls on its straight-line path - the
sampler's action draw (13 v_mad_u64_u32) and the prey trial words (19) - next to the rare fifth-trial call and the spawn draws of
an auto-reset: 61 v_mad_u64_u32 in all.  One full call (at most 20) under a wave-uniform branch on even steps replaces the two.
The stage must not cost the other SHAPE 1 builds or the probe entry a register: no scratch, no spill, and no more registers than
each had before it.  Needs hipcc, no GPU."""
import pytest

from tests import isa

HEADLINE = "_ZN2cm16rollout_w_kernelILi2ELb1ELb1ELb0ELb1ELi1EEE"       # <LHOPS 2, PRE, FULLWG, !TAPE, CARRY, SHAPE 1>

# (unit, mangled prefix) -> (vgpr_count: VGPRs + AGPRs, sgpr_count) of the build before the draw stage
BEFORE = {
    ("cm_rollout_w", "_ZN2cm22rollout_w_probe_kernelE"): (448, 106),
    ("cm_rollout_w", "_ZN2cm16rollout_w_kernelILi1ELb1ELb1ELb0ELb1ELi1EEE"): (442, 106),
    ("cm_rollout_w", "_ZN2cm16rollout_w_kernelILi1ELb1ELb0ELb0ELb1ELi1EEE"): (442, 106),
    ("cm_rollout_w", HEADLINE): (446, 106),
    ("cm_rollout_w", "_ZN2cm16rollout_w_kernelILi2ELb1ELb0ELb0ELb1ELi1EEE"): (446, 106),
    ("cm_rollout_wm", "_ZN2cm17rollout_wm_kernelILi1ELb1ELb1ELb1ELi1EEE"): (444, 106),
    ("cm_rollout_wm", "_ZN2cm17rollout_wm_kernelILi1ELb1ELb0ELb1ELi1EEE"): (444, 106),
    ("cm_rollout_wm", "_ZN2cm17rollout_wm_kernelILi2ELb1ELb1ELb1ELi1EEE"): (446, 106),
    ("cm_rollout_wm", "_ZN2cm17rollout_wm_kernelILi2ELb1ELb0ELb1ELi1EEE"): (446, 106),
}


def _mads(loop):
    return sum(1 for ln in loop if ln.startswith("v_mad_u64_u32"))


def test_headline_step_loop_philox_multiplies():
    k = isa.kernel(isa.listing("cm_rollout_w"), HEADLINE)
    loop = isa.step_loop(k.lines)
    n = isa.counts(loop)
    print("headline step loop: v_mad_u64_u32", _mads(loop), n)
    assert n["mfma"] >= 288, n                  # the loop found is the step (the whole policy tile sits inside it)
    assert _mads(loop) <= 50                    # 61 before: - 13 - 19 (the two per-step calls) + at most 20 (the shared call)


@pytest.mark.parametrize("unit,prefix", sorted(BEFORE))
def test_shape1_builds_keep_their_registers(unit, prefix):
    k = isa.kernel(isa.listing(unit), prefix)
    loop = isa.step_loop(k.lines)
    regs = (k._meta_int("vgpr_count"), k._meta_int("sgpr_count"))
    print(prefix, "registers", regs, "v_mad_u64_u32", _mads(loop))
    assert isa.counts(loop)["mfma"] >= 252      # the loop found is the step (a hop is 24 MFMAs of 16x16x32 and 12 of 16x16x16)
    assert k.private_segment_fixed_size == 0
    assert k.vgpr_spill_count == 0
    assert not any(ln.startswith("scratch_") for ln in k.lines)
    assert regs[0] <= BEFORE[unit, prefix][0] and regs[1] <= BEFORE[unit, prefix][1], (regs, BEFORE[unit, prefix])
    assert _mads(loop) <= 50                    # every SHAPE 1 build shares the stage
