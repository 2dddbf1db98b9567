"""Static checks of fwd_any_set_kernel (csrc/cm_policy_gm.hip: the run-time-sized Comm-DP forward for a policy set of mixed layer
sizes): it compiles for gfx950 and keeps the rules of cm_policy_g_dev.h - the rebuilt argument block stays in registers (no
private segment, no spill) and LDS is reached by integer offsets (no flat or scratch instruction)."""
from tests import isa


def _kernel():
    ks = isa.kernels(isa.listing("cm_policy_gm"), "fwd_any_set_kernel")
    assert len(ks) == 1, [k.name for k in ks]
    return ks[0]


def test_the_unit_is_part_of_the_library():
    assert "cm_policy_gm" in isa.units()


def test_set_kernel_compiles_with_no_private_segment_and_no_spill():
    k = _kernel()
    print(f"fwd_any_set_kernel: vgpr {k._meta_int('vgpr_count')} sgpr {k._meta_int('sgpr_count')} spills {k.vgpr_spill_count} "
          f"scratch {k.private_segment_fixed_size} static lds {k._meta_int('group_segment_fixed_size')}")
    assert k.private_segment_fixed_size == 0
    assert k.vgpr_spill_count == 0
    assert k._meta_int("group_segment_fixed_size") == 0       # the tile is dynamic, sized by the planner
    assert k.count("v_mfma_f32_16x16x4") > 0                  # the dense layers are the exact-f32 MFMA of the single launch


def test_set_kernel_has_no_flat_or_scratch_instruction():
    k = _kernel()
    assert not k.has_flat_or_scratch, [ln for ln in k.lines if isa.FLAT_OR_SCRATCH.match(ln)][:5]


def test_set_kernel_is_held_to_its_single_policy_twin():
    """What the single launch's policy instantiation satisfies in the same build, the set kernel satisfies too."""
    k = _kernel()
    twins = [t for t in isa.kernels(isa.listing("cm_policy_g"), "fwd_any_kernel") if "Lb0" in t.name]
    assert len(twins) == 1, [t.name for t in twins]
    twin = twins[0]
    assert twin.private_segment_fixed_size == 0 and twin.vgpr_spill_count == 0 and not twin.has_flat_or_scratch
    assert k.private_segment_fixed_size <= twin.private_segment_fixed_size
    assert k.vgpr_spill_count <= twin.vgpr_spill_count
    assert k._meta_int("group_segment_fixed_size") == twin._meta_int("group_segment_fixed_size")
