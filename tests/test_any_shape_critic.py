"""The no-grad forward of 'sum' critics whose layer sizes are not the default, on both routes - ONE launch of the run-time-sized
kernel (cm_critic_forward_any, csrc/cm_critic_g.hip) and layer by layer - against the float64 restatement
(tests/f64_commnet.critic_values): values within 1e-5 of the tensor's scale, the project's standing forward bound (TAU of
tests/test_any_shape_forward.py).  Shapes A and B of tests/any_shapes.py at 37 envs (the last workgroup is ragged), and a
third, seeded here: N = 5, d = 21, encoder (40,), embedding 16, decoder (100, 20, 12, 8), 1 hop, 'dot', no residual, no GCN bias
- a width below one MFMA tile, the deepest decoder, a team that does not divide a 16-row tile, the 'dot' branch."""
import ctypes as C

import numpy as np
import pytest

from tests import any_shapes as G
from tests import f64_commnet as R

pytestmark = pytest.mark.gpu
TAU = 1e-5
DEV = "cuda:0"
C_KW = dict(encoder_hidden_sizes=(40,), embedding_dim=16, decoder_hidden_sizes=(100, 20, 12, 8), attention_type="dot",
            residual=False, gcn_bias=False, n_gcn_layers=1)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need the MI355X")
    return torch


def _t64(torch, a):
    return None if a is None else torch.as_tensor(a, dtype=R.F64)


def _ref(torch, crit, obs, adj, ch, N, residual):
    with torch.no_grad():
        c64 = R.params(dict(crit.state_dict()), requires_grad=False)
        return R.critic_values(c64, _t64(torch, obs), _t64(torch, adj), _t64(torch, ch), N, residual, aggregator="sum")


_CASES = {}


def _case(shape, torch):
    """Critic, device inputs and the float64 values of one shape: computed once, shared by the tests, left unchanged."""
    if shape not in _CASES:
        from com_marl_amd import nets
        s = G.SHAPES[shape]
        if shape == "C":
            torch.manual_seed(4321)
            crit = nets.CommBaseCritic(G.spec_of(s["N"], s["d"]), n_agents=s["N"], device=DEV, **C_KW)
            with torch.no_grad():
                for name, p in crit.named_parameters():
                    if name.endswith("bias"):
                        p.uniform_(-0.1, 0.1)
            residual = False
        else:
            _, crit = G.build(shape)
            residual = True
        obs, _, adj, ch = G.inputs(s["N"], s["d"], s["hops"])
        dev = [torch.as_tensor(a).to(DEV) for a in (obs, adj, ch)]
        _CASES[shape] = dict(crit=crit, np=(obs, adj, ch), dev=dev, residual=residual, N=s["N"],
                             values=_ref(torch, crit, obs, adj, ch, s["N"], residual))
    return _CASES[shape]


@pytest.mark.parametrize("route,took", [("auto", "one_launch"), ("layers", "layers")])
@pytest.mark.parametrize("shape", ["A", "B", "C"])
def test_values_match_float64_on_both_routes(shape, route, took, torch_cuda):
    c = _case(shape, torch_cuda)
    crit = c["crit"]
    obs, adj, ch = c["dev"]
    crit._general_forward = route
    try:
        v = crit.values_device(obs, adj, ch)
        assert crit._last_forward == took
        assert tuple(v.shape) == (G.N_ENVS,)
        r = R.ratio(v, c["values"])
        print(f"shape {shape} {route}: values {r:.2e} of scale")
        assert r <= TAU
    finally:
        crit._general_forward = "auto"


def test_negative_control_other_hop_order_fails_the_bound(torch_cuda):
    """The float64 values with the channels of the two hops swapped must FAIL the bound at shape B: the check is not too loose."""
    torch = torch_cuda
    c = _case("B", torch)
    obs, adj, ch = c["np"]
    wrong = _ref(torch, c["crit"], obs, adj, np.ascontiguousarray(ch[:, ::-1]), c["N"], True)
    v = c["crit"].values_device(*c["dev"])
    assert c["crit"]._last_forward == "one_launch"
    r = R.ratio(v, wrong)
    print(f"shape B against the other hop order: {r:.2e} of scale")
    assert r > TAU


@pytest.mark.parametrize("shape", ["A", "C"])
def test_call_forms(shape, torch_cuda):
    torch = torch_cuda
    c = _case(shape, torch)
    crit, N = c["crit"], c["N"]
    obs, adj, ch = c["dev"]
    v = crit.values_device(obs, adj, ch)
    # one env
    v1 = crit.values_device(obs[:1], adj[:1], ch[:1])
    assert crit._last_forward == "one_launch" and tuple(v1.shape) == (1,)
    np.testing.assert_array_equal(v1.cpu().numpy(), v[:1].cpu().numpy())
    # the caller's buffer is returned and filled
    out = torch.full((G.N_ENVS,), float("nan"), device=DEV)
    got = crit.values_device(obs, adj, ch, out=out)
    assert got is out
    np.testing.assert_array_equal(out.cpu().numpy(), v.cpu().numpy())
    # None masks = all-ones masks, bit for bit
    v_none = crit.values_device(obs, None, None)
    v_ones = crit.values_device(obs, torch.ones_like(adj), torch.ones_like(ch))
    np.testing.assert_array_equal(v_none.cpu().numpy(), v_ones.cpu().numpy())
    assert (v_none != v).any()
    # a [P, T] lead shape through forward under no_grad = the flat call, bit for bit
    P, T = 3, 5
    with torch.no_grad():
        vpt = crit.forward(obs[:P * T].reshape(P, T, -1), None, adj[:P * T].reshape(P, T, N, N),
                           ch[:P * T].reshape(P, T, -1, N, N))
    assert crit._last_forward == "one_launch" and tuple(vpt.shape) == (P, T)
    np.testing.assert_array_equal(vpt.reshape(-1).cpu().numpy(), crit.values_device(obs[:P * T], adj[:P * T], ch[:P * T]).cpu().numpy())


def test_sync_weights_refreshes_the_flat_copy(torch_cuda):
    """After an in-place change of every parameter and sync_weights() the kernel reads the new weights."""
    torch = torch_cuda
    _, crit = G.build("A")
    s = G.SHAPES["A"]
    obs, _, adj, ch = G.inputs(s["N"], s["d"], s["hops"])
    dev = [torch.as_tensor(a).to(DEV) for a in (obs, adj, ch)]
    crit.sync_weights()
    v0 = crit.values_device(*dev).clone()
    assert crit._pack is not None
    with torch.no_grad():
        for p in crit.parameters():
            p.mul_(1.25)
    crit.sync_weights()
    assert not crit._pack_stale and crit._pack_sig == tuple((p.data_ptr(), p._version) for p in crit.parameters())
    v1 = crit.values_device(*dev)
    assert crit._last_forward == "one_launch"
    ref = _ref(torch, crit, obs, adj, ch, s["N"], True)
    assert R.ratio(v1, ref) <= TAU
    assert R.ratio(v0, ref) > TAU and (v1 != v0).any()


def test_shape_too_large_for_one_launch_goes_layer_by_layer(torch_cuda):
    """N = 80 with every width 128: the planes of one env need more than 160 KB of LDS.  The entry point answers 1 and leaves
    the buffer alone; values_device answers through the layer path within the same bound."""
    torch = torch_cuda
    from com_marl_amd import _lib as L, nets
    N, d, S = 80, 21, 3
    torch.manual_seed(5)
    crit = nets.CommBaseCritic(G.spec_of(N, d), n_agents=N, encoder_hidden_sizes=(128, 128), embedding_dim=128,
                               decoder_hidden_sizes=(128,), device=DEV)
    obs, _, adj, ch = G.inputs(N, d, 2, S=S)
    dobs, dadj, dch = (torch.as_tensor(a).to(DEV) for a in (obs, adj, ch))
    values = torch.full((S,), -1.0, device=DEV)
    w = crit._net_struct()
    with torch.cuda.device(DEV):
        rc = L.lib().cm_critic_forward_any(C.byref(w), S, L.ptr(dobs), L.ptr(dadj), L.ptr(dch), L.ptr(values), L.current_stream())
    assert rc == 1
    assert (values.cpu().numpy() == -1.0).all()
    v = crit.values_device(dobs, dadj, dch)
    assert crit._last_forward == "layers"
    assert R.ratio(v, _ref(torch, crit, obs, adj, ch, N, True)) <= TAU


def test_direct_and_default_critics_keep_their_routes(torch_cuda):
    torch = torch_cuda
    from com_marl_amd import nets
    obs = torch.rand(5, 84, device=DEV)
    direct = nets.CommBaseCritic(G.spec_of(4, 21), n_agents=4, aggregator_type="direct", device=DEV, **G.SIZES)
    default = nets.CommBaseCritic(G.spec_of(4, 21), n_agents=4, device=DEV)
    assert not direct._default_shape and default._default_shape
    for crit in (direct, default):
        crit.sync_weights()
        v = crit.values_device(obs, None, None)
        assert tuple(v.shape) == (5,) and bool(torch.isfinite(v).all())
        with torch.no_grad():
            crit.forward(obs, None, None, None)
        assert crit._last_forward != "one_launch" and crit._last_forward is None
