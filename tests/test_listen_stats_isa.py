"""csrc/cm_listen_stats.hip's kernels (every action count 2 .. 8 x lanes per graph 1 / 2 / 4 / 8 / 64 x load width) hold a row's
values, their logs and the six sums in registers: no private segment, no spilled register.  Needs hipcc, no GPU."""
from tests import isa


def test_no_kernel_of_the_unit_uses_scratch_or_spills():
    ks = isa.kernels(isa.listing("cm_listen_stats"))
    names = [k.name for k in ks]
    assert len(ks) == 7 * 5 * 2 and all("listen_stats_kernel" in n for n in names), names
    for k in ks:
        assert k.private_segment_fixed_size == 0, (k.name, k.private_segment_fixed_size)
        assert k.vgpr_spill_count == 0, (k.name, k.vgpr_spill_count)
        assert not any(ln.startswith("scratch_") for ln in k.lines), k.name
