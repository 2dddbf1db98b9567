"""csrc/cm_value_stats.hip's kernels (with and without each counterfactual) hold the batches of loaded steps and the recurrence in
registers: no private segment, no spilled register.  Needs hipcc, no GPU."""
from tests import isa


def test_no_kernel_of_the_unit_uses_scratch_or_spills():
    ks = isa.kernels(isa.listing("cm_value_stats"))
    names = [k.name for k in ks]
    assert len(ks) == 2 * 2 and all("value_stats_kernel" in n for n in names), names
    for k in ks:
        assert k.private_segment_fixed_size == 0, (k.name, k.private_segment_fixed_size)
        assert k.vgpr_spill_count == 0, (k.name, k.vgpr_spill_count)
        assert not any(ln.startswith("scratch_") for ln in k.lines), k.name
