"""CPU-side checks of the set forward (cm_policy_forward_multi: the acting forward of every member of a policy set in one launch):
the entry points are part of the C ABI without a version bump, every fwd_h_set_kernel is held to what its single-policy twin
fwd_h_kernel<0, KH, MAXMK, NW> of the same build satisfies, and the planner refuses a bad set on the host."""
import ctypes as C
import os
import re

import pytest

from tests import isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_forward_multi_is_declared_and_exported_at_abi_3():
    from com_marl_amd import _lib
    src = open(os.path.join(ROOT, "include", "commarl.h")).read()
    assert re.search(r"\bint64_t\s+cm_policy_forward_multi_plan\s*\(", src)
    assert re.search(r"\bint\s+cm_policy_forward_multi\s*\(", src)
    for name in ("cm_policy_forward_multi_plan", "cm_policy_forward_multi"):
        assert name in _lib.EXPORTED
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().cm_abi_version() == 3
    # cm_forward_set_wg: two int32; cm_forward_set_member: two int32 + the pack pointer + seven bias pointers
    assert "cm_forward_set_wg" in src and "cm_forward_set_member" in src
    assert C.sizeof(_lib.ForwardSetWg) == 2 * 4
    assert C.sizeof(_lib.ForwardSetMember) == 2 * 4 + 8 * 8


def test_set_kernels_are_held_to_their_single_policy_twins():
    """One fwd_h_set_kernel per (KH, MAXMK, NW) family dispatch_h selects for teams that are not 4.  What each may use is read
    from its twin in the same build: a private segment, VGPR spills, flat / scratch addressing only if the twin has them, and
    the same static LDS (the tile itself is dynamic, sized by the same lds_map on the host)."""
    sets = isa.kernels(isa.listing("cm_policy_hm"), "fwd_h_set_kernel")
    twins = isa.kernels(isa.listing("cm_policy_h"), "fwd_h_kernel")
    # (MAXMK, waves) 0/4 small teams on the VALU, 25/4 teams of 16..31, 15/8 teams of 32..80, 32/8 teams above 80, each for
    # observation dims padded to 32 / 64 / 96
    assert len(sets) == 12, [k.name for k in sets]
    seen = set()
    for k in sets:
        m = re.search(r"fwd_h_set_kernelILi(\d+)ELi(\d+)ELi(\d+)EE", k.name)
        assert m, k.name
        kh, mk, nw = (int(x) for x in m.groups())
        seen.add((kh, mk, nw))
        twin = [t for t in twins if f"fwd_h_kernelILi0ELi{kh}ELi{mk}ELi{nw}EE" in t.name]
        assert len(twin) == 1, (k.name, [t.name for t in twin])
        twin = twin[0]
        print(f"KH={kh} MAXMK={mk} NW={nw}: set vgpr {k._meta_int('vgpr_count')} sgpr {k._meta_int('sgpr_count')} "
              f"spills {k.vgpr_spill_count} scratch {k.private_segment_fixed_size} | twin vgpr {twin._meta_int('vgpr_count')} "
              f"sgpr {twin._meta_int('sgpr_count')} spills {twin.vgpr_spill_count} scratch {twin.private_segment_fixed_size}")
        if twin.private_segment_fixed_size == 0:
            assert k.private_segment_fixed_size == 0, k.name
        assert k.vgpr_spill_count <= twin.vgpr_spill_count, k.name
        if not twin.has_flat_or_scratch:
            assert not k.has_flat_or_scratch, k.name
        assert k._meta_int("group_segment_fixed_size") == twin._meta_int("group_segment_fixed_size"), k.name
    assert seen == {(kh, mk, nw) for kh in (32, 64, 96) for mk, nw in ((0, 4), (25, 4), (15, 8), (32, 8))}


def _members(K, N=24, d=77, pack=0x1000):
    from com_marl_amd import _lib
    ws = (_lib.PolicyWeights * max(K, 1))()
    for w in ws:
        w.d, w.n_agents, w.n_hops, w.enc_hidden, w.emb, w.h1, w.h2, w.h3, w.n_act = d, N, 2, 128, 64, 128, 64, 32, 5
        for name, _ in _lib.PolicyWeights._fields_[10:]:
            setattr(w, name, 0x1000)                    # never dereferenced by the planner
        w.mfma_pack = pack or None
    return ws


def _plan(ws, sizes, K, n_envs, image=None):
    from com_marl_amd import _lib
    n_wg = C.c_int32(-1)
    arr = (C.c_int32 * max(len(sizes), 1))(*sizes)
    need = _lib.lib().cm_policy_forward_multi_plan(ws, arr, K, n_envs, image, 0 if image is None else len(image), C.byref(n_wg))
    if need < 0:
        _lib.check(int(need), "cm_policy_forward_multi_plan")
    return need, n_wg.value


def test_planner_lays_out_the_table_and_refuses_bad_sets_on_the_host():
    from com_marl_amd import _lib
    # N = 24: two envs per workgroup, so groups of 3, 1, 4 take 2 + 1 + 2 workgroups - the ragged ones are not shared
    need, n_wg = _plan(_members(3), [3, 1, 4], 3, 8)
    assert n_wg == 5 and need == 5 * C.sizeof(_lib.ForwardSetWg) + 3 * C.sizeof(_lib.ForwardSetMember)
    image = (C.c_char * need)()
    assert _plan(_members(3), [3, 1, 4], 3, 8, image) == (need, 5)
    wgs = (_lib.ForwardSetWg * 5).from_buffer(image)
    assert [(w.member, w.block) for w in wgs] == [(0, 0), (0, 1), (1, 0), (2, 0), (2, 1)]
    mem = (_lib.ForwardSetMember * 3).from_buffer(image, 5 * C.sizeof(_lib.ForwardSetWg))
    assert [(m.first_env, m.n_envs) for m in mem] == [(0, 3), (3, 1), (4, 4)]
    assert all(m.pack > 0x1000 and m.enc_b1 == 0x1000 for m in mem)         # the f16 section lies behind the f32 one
    # shapes without a set kernel: 0, no table (teams of 4, teams above 80 agents)
    assert _plan(_members(2, N=4, d=21), [16, 16], 2, 32) == (0, 0)
    assert _plan(_members(2, N=96, d=77), [1, 1], 2, 2) == (0, 0)
    for ws, sizes, K, n_envs, text in [
            (_members(0), [], 0, 0, "at least one member"),
            (_members(3), [3, 0, 5], 3, 8, "at least one env"),
            (_members(3), [3, 1, 4], 3, 9, "sum to n_envs"),
            (_members(3, pack=0), [3, 1, 4], 3, 8, "no operand pack")]:
        with pytest.raises(_lib.CommarlError, match=text):
            _plan(ws, sizes, K, n_envs)
    mixed = _members(2)
    mixed[1].n_hops = 1
    with pytest.raises(_lib.CommarlError, match="differ in shape"):
        _plan(mixed, [1, 1], 2, 2)
    with pytest.raises(_lib.CommarlError, match="too small"):
        _plan(_members(3), [3, 1, 4], 3, 8, (C.c_char * (need - 1))())
