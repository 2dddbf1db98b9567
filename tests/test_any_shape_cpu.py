"""Comm-DP nets with non-default layer sizes, the part that needs no GPU: the float64 restatement (tests/f64_commnet.py)
reproduces the three recordings of the reference at such sizes (tools/gen_golden_shapes.py) to 1e-5 of each tensor's scale,
the bound of tests/test_f64_commnet.py; our classes have the recordings' state_dict; the new entry point is declared and
bound; and the ISA of its translation unit has no scratch, no spills and no flat addressing."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import any_shapes as G
from tests import f64_commnet as R
from tests import isa
from tests.test_f64_commnet import TAU, _check, _t

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("shape", ["A", "B"])
def test_restatement_matches_recorded_net_grads(shape):
    s = G.SHAPES[shape]
    z = G.fixture(s["fixture"])
    N = s["N"]
    assert z["adj"].shape[-1] == N and z["obs"].shape[1] == N * s["d"]
    pol, crit = R.params(G.sd_of(z, "pol")), R.params(G.sd_of(z, "crit"))
    assert pol["encoder._layers.1.linear.weight"].shape == (48, 96) and pol["gcn_layers.0.weight"].shape == (32, 32)
    obs, adj, ch, avail = _t(z["obs"]), _t(z["adj"]), _t(z["channels"]), _t(z["avail"])
    worst = {}
    _, probs, attn = R.policy_forward(pol, obs, avail, adj, ch, N)
    _check("probs", probs, z["probs"], worst)
    _check("attn", attn, z["attn"], worst)
    scalar = R.ppo_scalar(probs, torch.as_tensor(z["actions"]), _t(z["weights"]))
    scalar.backward()
    values = R.critic_values(crit, obs, adj, ch, N)
    _check("values", values, z["values"], worst)
    loss = R.critic_nll(values, R.critic_std(crit), _t(z["returns"]))
    loss.backward()
    _check("scalar", scalar, z["scalar"], worst)
    _check("critic_loss", loss, z["critic_loss"], worst)
    n = 0
    for pre, net in (("gpol", pol), ("gcrit", crit)):
        for pname, p in net.items():
            _check(f"{pre}.{pname}", torch.zeros_like(p) if p.grad is None else p.grad, z[f"{pre}.{pname}"], worst)
            n += 1
    assert n == len([f for f in z.files if f.startswith(("gpol.", "gcrit."))]) == 17 + 16
    print(f"{s['fixture']}: {n} gradients, worst ratio {max(worst.values()):.2e} ({max(worst, key=worst.get)})")


def test_restatement_matches_recorded_ppo_step():
    """shapes_ppo_step.npz: the critic's values over every step (the recorded baselines) and its Gaussian NLL (padded steps
    included, comm_base_critic.py:59-89); and the policy loss of the first step, where the ratio is 1 and the centred
    advantages of each path average to 0: -0.1 x the valid steps' mean entropy."""
    z = G.fixture("shapes_ppo_step")
    pol, crit = R.params(G.sd_of(z, "pol0"), requires_grad=False), R.params(G.sd_of(z, "crit0"), requires_grad=False)
    P, T = z["rewards"].shape
    obs, adj, ch = (_t(z[k]).reshape(P * T, -1) for k in ("obs", "dist_adjs", "channels"))
    worst = {}
    with torch.no_grad():
        values = R.critic_values(crit, obs, adj, ch, 4)
        _check("baselines", values.reshape(P, T), z["baselines"], worst)
        _check("critic_loss1", R.critic_nll(values, R.critic_std(crit), _t(z["returns"]).reshape(-1)), z["critic_loss1"], worst)
        _, probs, _ = R.policy_forward(pol, obs, None, adj, ch, 4)
        valid = torch.arange(T)[None, :] < torch.as_tensor(z["valids"])[:, None]
        _check("loss1", -0.1 * R.entropy(probs).reshape(P, T)[valid].mean(), z["loss1"], worst)
    print(f"shapes_ppo_step: worst ratio {max(worst.values()):.2e} ({max(worst, key=worst.get)})")


@pytest.mark.parametrize("shape", ["A", "B"])
def test_state_dict_equals_the_recording(shape):
    pol, crit = G.build(shape, device="cpu")                 # (loads strictly)
    z = G.fixture(G.SHAPES[shape]["fixture"])
    for net, pre in ((pol, "pol"), (crit, "crit")):
        want = G.sd_of(z, pre)
        assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == [(k, tuple(want[k].shape)) for k in want]
    assert not pol._default_shape and not crit._default_shape
    z = G.fixture("shapes_ppo_step")
    if shape == "A":
        assert {k: tuple(v.shape) for k, v in pol.state_dict().items()} == {k: tuple(v.shape) for k, v in G.sd_of(z, "pol0").items()}
        assert {k: tuple(v.shape) for k, v in crit.state_dict().items()} == {k: tuple(v.shape) for k, v in G.sd_of(z, "crit0").items()}


def test_fixture_names_stay_out_of_the_counted_sets():
    names = [f for f in os.listdir(G.GOLDEN) if f.startswith("shapes_")]
    assert sorted(names) == ["shapes_net_grads_co_map20.npz", "shapes_net_grads_pp_map10.npz", "shapes_ppo_step.npz"]
    assert all(os.path.getsize(os.path.join(G.GOLDEN, f)) < 1 << 20 for f in names)


def test_entry_point_is_declared_and_bound():
    from com_marl_amd import _lib as L
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "commarl.h")).read(), flags=re.S)
    assert re.search(r"\bint cm_policy_forward_any\s*\(const cm_net_weights \*w,", src)
    assert "cm_policy_forward_any" in L.EXPORTED
    lib = L.lib()
    assert hasattr(lib, "cm_policy_forward_any") and lib.cm_abi_version() == 3
    # 16 int32 (d, n_agents, n_hops, n_act, no_residual, emb, n_enc, 3 widths, n_head, 4 widths, pad), then 21 pointers
    body = re.search(r"typedef struct cm_net_weights \{(.*?)\} cm_net_weights;", src, re.S).group(1)
    assert len(re.findall(r"\*\s*\w+", body)) == 7 and L.NetWeights.enc_wt.offset == 64
    assert C.sizeof(L.NetWeights) == 16 * 4 + 21 * 8
    assert C.sizeof(L.PolicyWeights) == 10 * 4 + 16 * 8 and C.sizeof(L.CriticWeights) == 8 * 4 + 12 * 8    # pinned sizes kept
    assert lib.cm_policy_forward_any(None, 4, None, None, None, None, 0, 0, 0, None, 0, None, None, None, None) == -1
    # outside the kernel's bounds: 1 ("not for this shape"), nothing launched - no GPU needed to be told so
    w = L.NetWeights()
    w.d, w.n_agents, w.n_hops, w.n_act, w.emb, w.n_enc, w.n_head = 21, 4, 2, 5, 200, 1, 1
    w.enc_hidden[0], w.head_hidden[0] = 64, 64
    dummy = C.c_float()
    assert lib.cm_policy_forward_any(C.byref(w), 4, C.byref(dummy), None, None, None, 0, 0, 0, None, 0, None, None, None, None) == 1
    w.emb, w.n_agents, w.enc_hidden[0] = 128, 80, 128        # fits the bounds, not the 160 KB of LDS
    assert lib.cm_policy_forward_any(C.byref(w), 4, C.byref(dummy), None, None, None, 0, 0, 0, None, 0, None, None, None, None) == 1


def test_route_attribute_and_default_shape():
    from com_marl_amd import nets
    pol = nets.CommCategoricalMLPPolicy(G.spec_of(4, 21), n_agents=4)
    crit = nets.CommBaseCritic(G.spec_of(4, 21), n_agents=4)
    assert pol._default_shape and crit._default_shape and pol._graph_capturable_update and crit._graph_capturable_update
    assert list(pol._pack_tensors())[:4] == ["enc_w1t", "enc_b1", "enc_w2t", "enc_b2"]            # the default pack, as it was
    p2, _ = G.build("C", device="cpu")
    assert not p2._default_shape and p2._general_forward == "auto" and p2._pack_tensors()["attn_wt"] is None
    assert nets.CommBaseCritic(G.spec_of(4, 21), n_agents=4, decoder_hidden_sizes=(48,))._default_shape is False
    p2._general_forward = "layer"                            # a mistyped route is refused, not read as "layers"
    with pytest.raises(ValueError, match="_general_forward"):
        p2._act_device_any(torch.zeros(1, 5 * 21), None, None, None, False, None, None, None, 0, None, None)


def test_any_shape_kernel_isa_has_no_scratch_spills_or_flat_addressing():
    """The run-time-sized forward addresses LDS by integer offsets into one array and unrolls its layer loops over fixed
    argument slots: no private segment, no VGPR spill, no flat / scratch instruction, and its dense layers on the f32 MFMA."""
    ks = isa.kernels(isa.listing("cm_policy_g"))
    assert len(ks) == 1 and "fwd_any_kernel" in ks[0].name
    for k in ks:
        assert k.private_segment_fixed_size == 0, k.name
        assert k.vgpr_spill_count == 0, k.name
        assert not k.has_flat_or_scratch, k.name
        assert k.count("v_mfma_f32_16x16x4_f32") >= 8 and k.count("v_mfma_") == k.count("v_mfma_f32_16x16x4_f32")
        assert k.count("ds_") > 50
