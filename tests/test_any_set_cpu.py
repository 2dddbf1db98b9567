"""CPU-side checks of the policy-set forward for Comm-DP nets of any - also mixed - layer sizes (cm_policy_forward_any_multi): the
entry points and the table record are part of the C ABI without a version bump, the planner lays the table out, refuses a bad
set and declines what the kernel is not written for on the host, and nets.PolicySet keeps its whole architecture check unless
any_sizes=True is passed."""
import ctypes as C
import os
import re

import pytest

from tests import any_set_members as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_any_set_forward_is_declared_and_exported_at_abi_3():
    from com_marl_amd import _lib
    src = open(os.path.join(ROOT, "include", "commarl.h")).read()
    assert re.search(r"\bint64_t\s+cm_policy_forward_any_multi_plan\s*\(", src)
    assert re.search(r"\bint\s+cm_policy_forward_any_multi\s*\(", src)
    assert re.search(r"typedef\s+struct\s+cm_any_set_member\s*\{", src)
    for name in ("cm_policy_forward_any_multi_plan", "cm_policy_forward_any_multi"):
        assert name in _lib.EXPORTED
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().cm_abi_version() == 3
    # two int32 of the group, 13 of the sizes and strides, one of padding; 8 + 3 + 10 pointers
    assert C.sizeof(_lib.AnySetMember) == 16 * 4 + 21 * 8
    assert _lib.AnySetMember.enc_w.offset == 64


def _members(families, N, d, hops):
    from com_marl_amd import _lib
    return (_lib.NetWeights * max(len(families), 1))(*[M.net_struct(f, N, d, hops) for f in families])


def _plan(ws, sizes, K, n_envs, image=None):
    """-> (bytes | 0, n_wg, lds_bytes); raises what the planner refuses."""
    from com_marl_amd import _lib
    n_wg, lds = C.c_int32(-1), C.c_size_t(12345)
    arr = (C.c_int32 * max(len(sizes), 1))(*sizes)
    need = _lib.lib().cm_policy_forward_any_multi_plan(ws, arr, K, n_envs, image, 0 if image is None else len(image),
                                                       C.byref(n_wg), C.byref(lds))
    if need < 0:
        assert _lib.lib().cm_last_error()
        _lib.check(int(need), "cm_policy_forward_any_multi_plan")
    return need, n_wg.value, lds.value


@pytest.mark.parametrize("N,d,hops", [(5, 21, 1), (4, 21, 2), (24, 77, 2)])
def test_planner_lays_out_the_table_of_a_mixed_set(N, d, hops):
    from com_marl_amd import _lib
    fams = ["m0", "m1", "m2"]
    epb = M.epb_of(N)
    sizes = [2 * epb + 1, 1, 3 * epb + 1]
    blocks = [-(-s // epb) for s in sizes]
    ws = _members(fams, N, d, hops)
    need, n_wg, lds = _plan(ws, sizes, 3, sum(sizes))
    assert n_wg == sum(blocks) == 3 + 1 + 4
    assert need == n_wg * C.sizeof(_lib.ForwardSetWg) + 3 * C.sizeof(_lib.AnySetMember)
    assert lds == max(M.plan(N, d, f)[2] for f in fams) <= M.LDS_LIMIT          # the launch's LDS: the largest member's
    image = (C.c_char * need)()
    assert _plan(ws, sizes, 3, sum(sizes), image) == (need, n_wg, lds)
    wgs = (_lib.ForwardSetWg * n_wg).from_buffer(image)
    assert [(w.member, w.block) for w in wgs] == [(k, b) for k in range(3) for b in range(blocks[k])]    # in member order
    mem = (_lib.AnySetMember * 3).from_buffer(image, n_wg * C.sizeof(_lib.ForwardSetWg))
    assert [(m.first_env, m.n_envs) for m in mem] == [(0, sizes[0]), (sizes[0], 1), (sizes[0] + 1, sizes[2])]
    for m, fam, w in zip(mem, fams, ws):
        f = M.FAMILIES[fam]
        enc, head = f["encoder_hidden_sizes"], f["categorical_mlp_hidden_sizes"]
        assert (m.emb, m.no_residual) == (f["embedding_dim"], 0 if f.get("residual", True) else 1)
        assert (m.n_enc, tuple(m.enc_h)[:m.n_enc]) == (len(enc), enc)
        assert (m.n_head, tuple(m.head_h)[:m.n_head]) == (len(head), head)
        widest = max((f["embedding_dim"],) + enc + head)
        assert (m.SE, m.SW) == (M.pad16(f["embedding_dim"]) + 4, M.pad16(max(widest, d)) + 4) == M.plan(N, d, fam)[:2]
        # the member's own pointers: hidden layers in their slots, the output layers apart, NULL behind the last layer
        assert [m.enc_w[i] for i in range(3)] == [w.enc_wt[i] if i < len(enc) else None for i in range(3)]
        assert [m.enc_b[i] for i in range(3)] == [w.enc_b[i] if i < len(enc) else None for i in range(3)]
        assert (m.enc_wo, m.enc_bo) == (w.enc_wt[len(enc)], w.enc_b[len(enc)])
        assert [m.head_w[i] for i in range(4)] == [w.head_wt[i] if i < len(head) else None for i in range(4)]
        assert [m.head_b[i] for i in range(4)] == [w.head_b[i] if i < len(head) else None for i in range(4)]
        assert (m.head_wo, m.head_bo) == (w.head_wt[len(head)], w.head_b[len(head)])
        assert (m.attn_wt, m.gcn_w, m.gcn_b) == (w.attn_wt, w.gcn_w, w.gcn_b)
    assert mem[1].attn_wt is None and mem[1].gcn_b is None and mem[0].attn_wt and mem[0].gcn_b       # 'dot', no GCN bias


def test_planner_refuses_bad_sets_on_the_host():
    from com_marl_amd import _lib
    N, d, hops = 24, 77, 2
    fams = ["m0", "m1", "m2"]
    good = lambda: _members(fams, N, d, hops)                          # noqa: E731
    need, n_wg, _ = _plan(good(), [3, 1, 4], 3, 8)
    assert need > 0 and n_wg == 5

    def differs(field, value):
        ws = good()
        setattr(ws[2], field, value)
        return ws

    def null(field, slot=None):
        ws = good()
        if slot is None:
            setattr(ws[1], field, None)
        else:
            getattr(ws[1], field)[slot] = None
        return ws

    cases = [(_members([], N, d, hops), [], 0, 0, "at least one member"),
             (good(), [3, 0, 5], 3, 8, "at least one env"),
             (good(), [3, 1, 4], 3, 9, "sum to n_envs"),
             (differs("n_agents", 12), [3, 1, 4], 3, 8, "differ in"),
             (differs("d", 21), [3, 1, 4], 3, 8, "differ in"),
             (differs("n_hops", 1), [3, 1, 4], 3, 8, "differ in"),
             (differs("n_act", 4), [3, 1, 4], 3, 8, "differ in"),
             (null("enc_wt", 0), [3, 1, 4], 3, 8, "null encoder weight"),
             (null("enc_wt", 1), [3, 1, 4], 3, 8, "null encoder weight"),          # m1's encoder output layer
             (null("head_wt", 4), [3, 1, 4], 3, 8, "null head weight"),            # m1's logits layer
             (null("gcn_w"), [3, 1, 4], 3, 8, "null gcn_w")]
    for ws, sizes, K, n_envs, text in cases:
        with pytest.raises(_lib.CommarlError, match=text):
            _plan(ws, sizes, K, n_envs)
    with pytest.raises(_lib.CommarlError, match="too small"):
        _plan(good(), [3, 1, 4], 3, 8, (C.c_char * (need - 1))())
    n_wg = C.c_int32(0)
    assert _lib.lib().cm_policy_forward_any_multi_plan(good(), (C.c_int32 * 3)(3, 1, 4), 3, 8, None, 0, C.byref(n_wg), None) < 0
    assert b"null argument" in _lib.lib().cm_last_error()
    # NULL where the net has no such weight is no refusal: 'dot' attention, no GCN bias, biases of any layer
    ws = good()
    ws[0].attn_wt = ws[0].gcn_b = None
    assert _plan(ws, [3, 1, 4], 3, 8)[0] == need


def test_planner_declines_what_the_kernel_is_not_written_for():
    """0, *n_wg = 0, nothing written: a member outside the bounds of cm_policy_forward_any, or above 160 KB of LDS."""
    N, d, hops = 24, 77, 2
    wide = _members(["m0", "m1", "m2"], N, d, hops)
    wide[1].head_hidden[0] = 129                                       # one more than the widest layer the kernel takes
    image = (C.c_char * 4096)(*([b"\x55"] * 4096))
    assert _plan(wide, [3, 1, 4], 3, 8, image)[:2] == (0, 0)
    assert bytes(image) == b"\x55" * 4096
    no_enc = _members(["m0", "m1", "m2"], N, d, hops)
    no_enc[0].n_enc = 0
    assert _plan(no_enc, [3, 1, 4], 3, 8)[:2] == (0, 0)
    # m2 at N = 72, d = 53: one env per workgroup, 80 rows of 2 x (132 + 132) floats = 168 960 B of planes alone
    assert 80 * 528 * 4 == 168960 > M.LDS_LIMIT
    assert M.plan(72, 53, "m2")[2] > M.LDS_LIMIT
    assert M.plan(72, 53, "m0")[2] == M.plan(72, 53, "m1")[2] == 129088
    need, n_wg, lds = _plan(_members(["m0", "m1", "m2"], 72, 53, 2), [3, 1, 4], 3, 8, image)
    assert (need, n_wg) == (0, 0) and lds == M.plan(72, 53, "m2")[2]
    assert bytes(image) == b"\x55" * 4096
    need, n_wg, lds = _plan(_members(["m0", "m1"], 72, 53, 2), [3, 1], 2, 4)
    assert need > 0 and n_wg == 4 and lds == 129088                    # without m2 the set fits: one env per workgroup


# ---- nets.PolicySet: the check that stays, and what the keyword frees -------------------------------------------------
def _pol(family, N=5, d=21, hops=1, seed=1, **over):
    import torch
    from com_marl_amd import nets
    from tests.any_shapes import spec_of
    torch.manual_seed(seed)
    kw = dict(M.FAMILIES[family], n_gcn_layers=hops)
    kw.update(over)
    return nets.CommCategoricalMLPPolicy(spec_of(N, d), n_agents=N, device="cpu", **kw)


def test_policy_set_without_the_keyword_still_refuses_differing_sizes():
    from com_marl_amd import nets
    for other, field in (("m1", "attention type"), ("m2", "hidden sizes")):
        with pytest.raises(ValueError, match=f"differs from policies.0. in {field}"):
            nets.PolicySet([_pol("m0"), _pol(other)])
        with pytest.raises(ValueError, match=f"differs from policies.0. in {field}"):
            nets.PolicySet([_pol("m0"), _pol(other)], any_sizes=False)
    with pytest.raises(ValueError, match="in residual"):
        nets.PolicySet([_pol("m0"), _pol("m0", residual=False)])
    ps = nets.PolicySet([_pol("m0", seed=1), _pol("m0", seed=2)])
    assert ps.uniform and not ps.any_sizes and ps.set_kernel == "default"


def test_policy_set_with_the_keyword_frees_the_sizes_and_keeps_the_rest():
    from com_marl_amd import nets
    ps = nets.PolicySet([_pol("m0"), _pol("m1"), _pol("m2")], any_sizes=True)
    assert len(ps) == 3 and ps.any_sizes and not ps.uniform and ps.set_kernel == "any"
    assert (ps._n_agents, ps._dec_obs_dim, ps._action_dim, ps.n_gcn_layers, ps.comm) == (5, 21, 5, 1, True)
    for name in ("_embedding_dim", "residual"):                        # what may differ is not handed out from member 0
        with pytest.raises(AttributeError):
            getattr(ps, name)
    # K checkpoints of one non-default shape: uniform, and on the new route only with the keyword
    same = nets.PolicySet([_pol("m0", seed=1), _pol("m0", seed=2)], any_sizes=True)
    assert same.uniform and same.set_kernel == "any"
    # each field the members still share
    for bad, field in ((_pol("m1", N=4), "team size"), (_pol("m1", d=22), "observation dim"), (_pol("m1", hops=2), "hops")):
        with pytest.raises(ValueError, match=f"in {field}"):
            nets.PolicySet([_pol("m0"), bad], any_sizes=True)
    from tests.any_shapes import spec_of
    from com_marl_amd.envs import EnvSpec, _Box, _Discrete
    import numpy as np
    six = nets.CommCategoricalMLPPolicy(EnvSpec(_Box(np.zeros(21 * 5), np.ones(21 * 5)), _Discrete(6)), n_agents=5, n_gcn_layers=1,
                                        device="cpu", **M.FAMILIES["m1"])
    with pytest.raises(ValueError, match="in action dim"):
        nets.PolicySet([_pol("m0"), six], any_sizes=True)
    dec = nets.DecCategoricalMLPPolicy(spec_of(5, 21), n_agents=5, device="cpu")
    with pytest.raises(ValueError, match="in class"):
        nets.PolicySet([_pol("m0"), dec], any_sizes=True)


def test_obs_dp_members_keep_the_whole_check_with_the_keyword():
    from com_marl_amd import nets
    from tests.any_shapes import spec_of
    a = nets.DecCategoricalMLPPolicy(spec_of(5, 21), n_agents=5, device="cpu")
    b = nets.DecCategoricalMLPPolicy(spec_of(5, 21), n_agents=5, hidden_sizes=(64, 32, 16), device="cpu")
    with pytest.raises(ValueError, match="in hidden sizes"):
        nets.PolicySet([a, b], any_sizes=True)
    ps = nets.PolicySet([a, nets.DecCategoricalMLPPolicy(spec_of(5, 21), n_agents=5, device="cpu")], any_sizes=True)
    assert ps.uniform and ps.set_kernel == "default"


def test_default_sized_uniform_set_with_the_keyword_is_the_set_without_it():
    from com_marl_amd import nets
    from tests.any_shapes import spec_of
    mk = lambda: nets.CommCategoricalMLPPolicy(spec_of(5, 21), n_agents=5, n_gcn_layers=1, device="cpu")     # noqa: E731
    ps = nets.PolicySet([mk(), mk()], any_sizes=True)
    assert ps.uniform and ps.set_kernel == "default"
    mixed = nets.PolicySet([mk(), _pol("m0")], any_sizes=True)
    assert not mixed.uniform and mixed.set_kernel == "any"
