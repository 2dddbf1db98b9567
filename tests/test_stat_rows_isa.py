"""csrc/cm_stat_rows.hip's kernels - the four reductions every statistics family shares (episode rows, group means, curve sums, curve
means), each instantiated for rows of four int32 and of six doubles - keep their column sums in registers: no private segment, no
spilled register.  Needs hipcc, no GPU."""
from tests import isa

REDUCTIONS = ("episode_rows_kernel", "group_means_kernel", "curve_sums_kernel", "curve_means_kernel")


def test_no_kernel_of_the_unit_uses_scratch_or_spills():
    ks = isa.kernels(isa.listing("cm_stat_rows"))
    names = [k.name for k in ks]
    assert len(ks) == 4 * 2, names
    for r in REDUCTIONS:                                        # one of each row kind: <int32_t, 4> / <4> and <double, 6> / <6>
        mine = sorted(n.split(r)[1][:6] for n in names if r in n)
        assert mine in (["IdLi6E", "IiLi4E"], ["ILi4EE", "ILi6EE"]), (r, names)
    for k in ks:
        assert k.private_segment_fixed_size == 0, (k.name, k.private_segment_fixed_size)
        assert k.vgpr_spill_count == 0, (k.name, k.vgpr_spill_count)
        assert not any(ln.startswith("scratch_") for ln in k.lines), k.name
