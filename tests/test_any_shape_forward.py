"""The acting forward of Comm-DP nets whose layer sizes are not the default (tests/any_shapes.py: shapes A, B, C), on both
routes - ONE launch of the run-time-sized kernel (cm_policy_forward_any) and layer by layer - against the float64
restatement (tests/f64_commnet.py): probabilities and attention within 1e-5 of each tensor's scale (the project's standing
forward bound), greedy = argmax of the kernel's own probabilities, sampled actions = the oracle's inverse-CDF draw on the
kernel's own probabilities, exactly; the critic's values at A and B to the same bound; and a shape too large for one launch."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import any_shapes as G
from tests import f64_commnet as R

pytestmark = pytest.mark.gpu
TAU = 1e-5


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need the MI355X")
    return torch


_CASES = {}


def _case(shape, torch):
    """Nets, device inputs and the float64 answers of one shape: computed once, shared by the tests, left unchanged."""
    if shape not in _CASES:
        s = G.SHAPES[shape]
        pol, crit = G.build(shape)
        obs, avail, adj, ch = G.inputs(s["N"], s["d"], s["hops"])
        t64 = lambda a: torch.as_tensor(a, dtype=R.F64)                              # noqa: E731
        residual = s["pol"].get("residual", True)
        with torch.no_grad():
            p64 = R.params({k: v for k, v in pol.state_dict().items()}, requires_grad=False)
            _, probs, attn = R.policy_forward(p64, t64(obs), t64(avail), t64(adj), t64(ch), s["N"], residual)
            values = None
            if crit is not None:
                c64 = R.params({k: v for k, v in crit.state_dict().items()}, requires_grad=False)
                values = R.critic_values(c64, t64(obs), t64(adj), t64(ch), s["N"])
        dev = [torch.as_tensor(a).to("cuda:0") for a in (obs, avail, adj, ch)]
        _CASES[shape] = dict(pol=pol, crit=crit, dev=dev, probs=probs, attn=attn, values=values)
    return _CASES[shape]


@pytest.mark.parametrize("route,took", [("auto", "one_launch"), ("layers", "layers")])
@pytest.mark.parametrize("shape", sorted(G.SHAPES))
def test_forward_and_sample_match_float64(shape, route, took, torch_cuda):
    torch = torch_cuda
    c = _case(shape, torch)
    pol = c["pol"]
    obs, avail, adj, ch = c["dev"]
    pol._general_forward = route
    try:
        pol.set_rng(seed=77, env_id_offset=1000)
        acts, probs, attn = pol.act_device(obs, avail, adj, ch, policy_step=5)
        assert pol._last_forward == took
        r_p, r_a = R.ratio(probs, c["probs"]), R.ratio(attn, c["attn"])
        print(f"shape {shape} {route}: probs {r_p:.2e} attn {r_a:.2e} of scale")
        assert r_p <= TAU and r_a <= TAU
        p_np = probs.cpu().numpy()
        assert (p_np[avail.cpu().numpy() == 0] == 0).all()
        np.testing.assert_array_equal(acts.cpu().numpy(), O.sample_actions(p_np, 77, 1000, 5))
        # another step, the env id offset of the call, outputs into the caller's buffers
        out_a, out_p = torch.empty_like(acts), torch.empty_like(probs)
        a2, p2, _ = pol.act_device(obs, avail, adj, ch, policy_step=9, env_id_offset=31, out_actions=out_a, out_probs=out_p,
                                   want_attn=False)
        assert a2 is out_a and p2 is out_p
        np.testing.assert_array_equal(p2.cpu().numpy(), p_np)
        np.testing.assert_array_equal(a2.cpu().numpy(), O.sample_actions(p_np, 77, 31, 9))
        assert (a2 != acts).any()
        g, pg, _ = pol.act_device(obs, avail, adj, ch, greedy=True, policy_step=5)
        np.testing.assert_array_equal(g.cpu().numpy(), pg.cpu().numpy().argmax(-1))
        # None masks = all ones
        _, p1, m1 = pol.act_device(obs, None, None, None, want_actions=False, policy_step=0)
        _, p0, m0 = pol.act_device(obs, torch.ones_like(avail), torch.ones_like(adj), torch.ones_like(ch), want_actions=False,
                                   policy_step=0)
        np.testing.assert_array_equal(p1.cpu().numpy(), p0.cpu().numpy())
        np.testing.assert_array_equal(m1.cpu().numpy(), m0.cpu().numpy())
    finally:
        pol._general_forward = "auto"


@pytest.mark.parametrize("shape", ["A", "B"])
def test_critic_values_match_float64(shape, torch_cuda):
    torch = torch_cuda
    c = _case(shape, torch)
    obs, _, adj, ch = c["dev"]
    v = c["crit"].values_device(obs, adj, ch)
    r = R.ratio(v, c["values"])
    print(f"shape {shape}: values {r:.2e} of scale")
    assert r <= TAU
    with torch.no_grad():
        v2 = c["crit"].forward(obs, None, adj, ch)
    np.testing.assert_array_equal(v2.cpu().numpy(), v.cpu().numpy())


def test_evaluate_nograd_returns_the_acting_probabilities(torch_cuda):
    torch = torch_cuda
    c = _case("A", torch)
    obs, _, adj, ch = c["dev"]
    logits, probs = c["pol"].evaluate_nograd(obs, adj, ch)
    assert logits is None
    _, want, _ = c["pol"].act_device(obs, None, adj, ch, want_actions=False, policy_step=0)
    np.testing.assert_array_equal(probs.cpu().numpy(), want.cpu().numpy())


def test_shape_too_large_for_one_launch_goes_layer_by_layer(torch_cuda):
    """N = 80 with every width 128: the planes of one env need more than 160 KB of LDS.  The entry point answers 1 having
    launched nothing, and act_device answers through the layer path within the same bound."""
    torch = torch_cuda
    from com_marl_amd import _lib as L, nets
    N, d, S = 80, 21, 3
    torch.manual_seed(5)
    pol = nets.CommCategoricalMLPPolicy(G.spec_of(N, d), n_agents=N, encoder_hidden_sizes=(128, 128), embedding_dim=128,
                                        categorical_mlp_hidden_sizes=(128,), device="cuda:0")
    obs, avail, adj, ch = G.inputs(N, d, 2, S=S)
    dobs, dav, dadj, dch = (torch.as_tensor(a).to("cuda:0") for a in (obs, avail, adj, ch))
    probs = torch.full((S, N, 5), -1.0, device="cuda:0")
    w = pol._net_struct()
    with torch.cuda.device("cuda:0"):
        rc = L.lib().cm_policy_forward_any(C.byref(w), S, L.ptr(dobs), L.ptr(dav), L.ptr(dadj), L.ptr(dch), 1, 0, 0, None, 0, None,
                                           L.ptr(probs), None, L.current_stream())
    assert rc == 1
    assert (probs.cpu().numpy() == -1.0).all()
    acts, probs, attn = pol.act_device(dobs, dav, dadj, dch, policy_step=2)
    assert pol._last_forward == "layers"
    t64 = lambda a: torch.as_tensor(a, dtype=R.F64)                                  # noqa: E731
    with torch.no_grad():
        p64 = R.params(dict(pol.state_dict()), requires_grad=False)
        _, p_ref, a_ref = R.policy_forward(p64, t64(obs), t64(avail), t64(adj), t64(ch), N)
    assert R.ratio(probs, p_ref) <= TAU and R.ratio(attn, a_ref) <= TAU
    np.testing.assert_array_equal(acts.cpu().numpy(), O.sample_actions(probs.cpu().numpy(), pol.seed, 0, 2))


def test_default_shape_keeps_its_route(torch_cuda):
    """A default-shaped policy never reaches the run-time-sized kernel."""
    from com_marl_amd import nets
    pol = nets.CommCategoricalMLPPolicy(G.spec_of(4, 21), n_agents=4, device="cuda:0")
    assert pol._default_shape
    obs = torch_cuda.rand(5, 84, device="cuda:0")
    pol.act_device(obs, None, None, None, policy_step=0)
    assert pol._last_forward is None
