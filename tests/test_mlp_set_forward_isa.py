"""CPU-side checks of the row-MLP set forward (cm_mlp_policy_forward_multi: the acting forward of every member of an Obs-DP / CENT
policy set in one launch): the entry points are part of the C ABI without a version bump, mlp_set_kernel is held to what its
single-policy twin mlp_kernel of the same build satisfies (kernel metadata only), and the planner lays the table out and refuses
a bad set on the host."""
import ctypes as C
import os
import re

import pytest

from tests import isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXL = 6                                                # CM_MLP_MAX_LAYERS


def test_mlp_forward_multi_is_declared_and_exported_at_abi_3():
    from com_marl_amd import _lib
    src = open(os.path.join(ROOT, "include", "commarl.h")).read()
    assert re.search(r"\bint64_t\s+cm_mlp_forward_multi_plan\s*\(", src)
    assert re.search(r"\bint\s+cm_mlp_policy_forward_multi\s*\(", src)
    for name in ("cm_mlp_forward_multi_plan", "cm_mlp_policy_forward_multi"):
        assert name in _lib.EXPORTED
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().cm_abi_version() == 3


def test_member_record_has_its_documented_size():
    """cm_mlp_set_member: first row, row count, first env and a pad (four int32), then CM_MLP_MAX_LAYERS bias pointers and as many
    pack pointers - 112 bytes, as the header says."""
    from com_marl_amd import _lib
    src = open(os.path.join(ROOT, "include", "commarl.h")).read()
    assert _lib.MLP_MAX_LAYERS == MAXL and re.search(r"#define\s+CM_MLP_MAX_LAYERS\s+6\b", src)
    assert "cm_mlp_set_member" in src
    assert C.sizeof(_lib.MlpSetMember) == 4 * 4 + 2 * MAXL * 8 == 112
    assert _lib.MlpSetMember.b.offset == 16 and _lib.MlpSetMember.pack.offset == 16 + 8 * MAXL
    assert re.search(r"cm_mlp_set_member\s*\{[^\n]*112 bytes", src)


def test_set_kernel_is_held_to_its_single_policy_twin():
    """What mlp_set_kernel may use is read from mlp_kernel in the same build: a private segment, VGPR spills, flat / scratch
    addressing only if the twin has them, and the same static LDS (the two tiles are dynamic, sized by the same host code)."""
    asm = isa.listing("cm_mlp")
    k, twin = isa.kernels(asm, "mlp_set_kernel"), isa.kernels(asm, "mlp_kernel")
    assert len(k) == 1 and len(twin) == 1, ([x.name for x in k], [x.name for x in twin])
    k, twin = k[0], twin[0]
    print(f"mlp_set_kernel vgpr {k._meta_int('vgpr_count')} sgpr {k._meta_int('sgpr_count')} spills {k.vgpr_spill_count} "
          f"scratch {k.private_segment_fixed_size} | mlp_kernel vgpr {twin._meta_int('vgpr_count')} sgpr {twin._meta_int('sgpr_count')} "
          f"spills {twin.vgpr_spill_count} scratch {twin.private_segment_fixed_size}")
    if twin.private_segment_fixed_size == 0:
        assert k.private_segment_fixed_size == 0
    assert k.vgpr_spill_count <= twin.vgpr_spill_count
    if not twin.has_flat_or_scratch:
        assert not k.has_flat_or_scratch
    assert k._meta_int("group_segment_fixed_size") == twin._meta_int("group_segment_fixed_size")


# ---- the planner: host only, the pointers are never dereferenced ------------------------------------------------------------
def _members(K, N=4, d=21, cent=False, pack=0x100000, A=5):
    """K members of the Obs-DP chain (d -> 32 -> 32 -> 32 -> A per agent row) or the CENT chain (N*d -> 32 -> 32 -> N*A per env
    row); layer l's bias at 0x1000 * (l + 1) + member."""
    from com_marl_amd import _lib
    dims = [32, 32, N * A] if cent else [32, 32, 32, A]
    ws = (_lib.MlpWeights * max(K, 1))()
    for k, w in enumerate(ws):
        w.in_dim, w.n_layers = (N * d if cent else d), len(dims)
        w.tanh_mask, w.relu_mask = (1 << (len(dims) - 1)) - 1, 0
        for l, o in enumerate(dims):
            w.out_dim[l], w.wt[l], w.b[l] = o, 0x800, 0x1000 * (l + 1) + k
        w.mfma_pack = pack or None
    return ws


def _plan(ws, sizes, K, n_envs, groups, N=4, A=5, image=None):
    from com_marl_amd import _lib
    n_wg = C.c_int32(-1)
    arr = (C.c_int32 * max(len(sizes), 1))(*sizes)
    need = _lib.lib().cm_mlp_forward_multi_plan(ws, arr, K, n_envs, groups, A, N, image, 0 if image is None else len(image),
                                                C.byref(n_wg))
    if need < 0:
        _lib.check(int(need), "cm_mlp_forward_multi_plan")
    return need, n_wg.value


def _pack_floats(K, OUT):
    return ((OUT + 15) // 16) * ((K + 15) // 16) * 256


@pytest.mark.parametrize("cent", [False, True], ids=["obsdp", "cent"])
def test_planner_lays_out_the_table(cent):
    from com_marl_amd import _lib
    N, d, sizes = 4, 21, [9, 1, 17]
    groups = N if cent else 1
    rows = [s * N // groups for s in sizes]             # Obs-DP 36 / 4 / 68 agent rows, CENT 9 / 1 / 17 env rows
    blocks = [-(-r // 32) for r in rows]
    assert blocks == ([1, 1, 1] if cent else [2, 1, 3])
    n = sum(blocks)
    ws = _members(3, N, d, cent)
    need, n_wg = _plan(ws, sizes, 3, 27, groups)
    assert n_wg == n and need == n * C.sizeof(_lib.ForwardSetWg) + 3 * C.sizeof(_lib.MlpSetMember)
    image = (C.c_char * need)()
    assert _plan(ws, sizes, 3, 27, groups, image=image) == (need, n)
    wgs = (_lib.ForwardSetWg * n).from_buffer(image)
    assert [(w.member, w.block) for w in wgs] == [(k, b) for k in range(3) for b in range(blocks[k])]
    mem = (_lib.MlpSetMember * 3).from_buffer(image, n * C.sizeof(_lib.ForwardSetWg))
    first_rows = [0, rows[0], rows[0] + rows[1]]
    assert [(m.first_row, m.n_rows, m.first_env) for m in mem] == list(zip(first_rows, rows, [0, 9, 10]))
    # per layer: the member's own bias, and its fragments where cm_mlp_pack puts them
    dims = [ws[0].in_dim] + [ws[0].out_dim[l] for l in range(ws[0].n_layers)]
    offs = [0]
    for l in range(ws[0].n_layers):
        offs.append(offs[-1] + 4 * _pack_floats(dims[l], dims[l + 1]))
    for k, m in enumerate(mem):
        for l in range(MAXL):
            live = l < ws[0].n_layers
            assert (m.b[l] or 0) == (0x1000 * (l + 1) + k if live else 0)
            assert (m.pack[l] or 0) == (0x100000 + offs[l] if live else 0)


def test_planner_answers_no_set_kernel_without_a_pack():
    ws = _members(3)
    ws[1].mfma_pack = None
    assert _plan(ws, [9, 1, 17], 3, 27, 1) == (0, 0)
    assert _plan(_members(3, pack=0), [9, 1, 17], 3, 27, 1) == (0, 0)


def test_planner_refuses_bad_sets_on_the_host():
    from com_marl_amd import _lib
    sizes = [9, 1, 17]
    for ws, sz, K, n_envs, groups, text in [
            (_members(0), [], 0, 0, 1, "at least one member"),
            (_members(3), [9, 0, 18], 3, 27, 1, "at least one env"),
            (_members(3), sizes, 3, 28, 1, "sum to n_envs"),
            (_members(3), sizes, 3, 27, 2, "groups is 1 .* or agents_per_env"),
            (_members(3), sizes, 3, 27, 4, "last layer width != groups \\* n_act"),       # the Obs-DP chain is 5 wide, not 20
            (_members(3, cent=True), sizes, 3, 27, 1, "last layer width != groups \\* n_act")]:
        with pytest.raises(_lib.CommarlError, match=text):
            _plan(ws, sz, K, n_envs, groups)
    for field, value in [("in_dim", 22), ("n_layers", 3), ("tanh_mask", 3), ("relu_mask", 8)]:
        mixed = _members(2)
        setattr(mixed[1], field, value)
        with pytest.raises(_lib.CommarlError, match="differ in shape"):
            _plan(mixed, [1, 1], 2, 2, 1)
    mixed = _members(2)
    mixed[1].out_dim[1] = 48
    with pytest.raises(_lib.CommarlError, match="differ in shape"):
        _plan(mixed, [1, 1], 2, 2, 1)
    need, _ = _plan(_members(3), sizes, 3, 27, 1)
    with pytest.raises(_lib.CommarlError, match="too small"):
        _plan(_members(3), sizes, 3, 27, 1, image=(C.c_char * (need - 1))())
