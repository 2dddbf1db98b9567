"""The training path of Comm-DP nets whose embedding is not 64, now on the any-width graph ops (cm_attention_*_any,
cm_masked_agg_*_any through the any-width family of nets._AttentionSoftmax / _MaskedAggregate): which route nets.graph_op_route
gives and which entry points then run (recorded by the proxy of tests/lib_spy.py around com_marl_amd._lib.lib()), every
parameter gradient of policy and critic at shapes A and C (tests/any_shapes.py) against float64 autograd of
tests/f64_commnet.py - the bound of tests/test_any_shape_training.py:121-123, rtol 1e-4 plus 1e-5 of the tensor's scale -
and bit-identical gradients of two backward passes in deterministic mode."""
import numpy as np
import pytest

from tests import any_shapes as G
from tests import f64_commnet as R
from tests.lib_spy import spy  # noqa: F401  (the fixture: a recording proxy around _lib.lib())
from tests.test_any_shape_critic import C_KW

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need the MI355X")
    return torch


def _nets(shape, torch):
    from com_marl_amd import nets
    s = G.SHAPES[shape]
    pol, crit = G.build(shape)
    if crit is None:                                                         # shape C: a critic of the same trunk, seeded here
        torch.manual_seed(4321)
        crit = nets.CommBaseCritic(G.spec_of(s["N"], s["d"]), n_agents=s["N"], device=DEV, **C_KW)
    return pol, crit


def _any_calls(spy):
    return [c for c in spy.calls if c.endswith("_any")]


def test_graph_op_routes(torch_cuda, spy):
    torch = torch_cuda
    from com_marl_amd import nets
    for N, E in ((4, 32), (24, 32), (5, 16)):
        assert nets.graph_op_route(N, E) == "hip", (N, E)
    assert nets.graph_op_route(200, 32) == "framework"
    # a shape whose planes do not fit: the forward op answers 1 once, the framework path answers, and the answer is kept
    N, E, S = 128, 128, 2
    assert nets.graph_op_route(N, E) == "hip"
    att = nets.AttentionModule(E, "dot").to(DEV)
    e = torch.tanh(torch.randn(S, N, E, device=DEV))
    try:
        m = att(e)
        assert _any_calls(spy) == ["cm_attention_forward_any"]               # asked once: the refusal
        assert nets.graph_op_route(N, E) == "framework"
        want = torch.softmax(e @ e.transpose(-2, -1), -1).cpu().numpy()
        np.testing.assert_allclose(m.cpu().numpy(), want, rtol=1e-5, atol=1e-7)
        spy.calls.clear()
        m2 = att(e)
        out = nets.masked_aggregate(m, None, None, 0, e, None)
        assert not _any_calls(spy), spy.calls                                # not probed again
        np.testing.assert_allclose(m2.cpu().numpy(), want, rtol=1e-5, atol=1e-7)
        assert tuple(out.shape) == (S, N, E)
    finally:
        nets.set_graph_op_route(N, E, None)


def test_width_64_never_asks_for_a_route(torch_cuda, monkeypatch, spy):
    torch = torch_cuda
    from com_marl_amd import nets

    def boom(*a):
        raise AssertionError("graph_op_route consulted for E = 64")
    # AttentionModule and masked_aggregate resolve the name in their own module (nets.graph): a patch on the façade reaches neither
    from com_marl_amd.nets import graph
    assert nets.AttentionModule.__module__ == nets.masked_aggregate.__module__ == graph.__name__
    monkeypatch.setattr(graph, "graph_op_route", boom)
    S, N = 3, 4
    with pytest.raises(AssertionError, match="graph_op_route consulted"):    # the patch is live: a width other than 64 does ask
        nets.AttentionModule(32, "dot").to(DEV)(torch.tanh(torch.randn(S, N, 32, device=DEV)))
    assert spy.calls == []
    e = torch.tanh(torch.randn(S, N, 64, device=DEV))
    m = nets.AttentionModule(64, "dot").to(DEV)(e)
    out = nets.masked_aggregate(m, None, None, 0, e, None)
    assert tuple(out.shape) == (S, N, 64)
    assert spy.calls == ["cm_attention_forward", "cm_masked_agg_forward"]    # and no _any entry point


@pytest.mark.parametrize("shape", ["A", "C"])
def test_parameter_gradients_match_float64(shape, torch_cuda, spy):
    torch = torch_cuda
    s = G.SHAPES[shape]
    N, hops = s["N"], s["hops"]
    residual = s["pol"].get("residual", True)
    pol, crit = _nets(shape, torch)
    obs, avail, adj, ch = G.inputs(N, s["d"], hops)
    S = obs.shape[0]
    dobs, dav, dadj, dch = (torch.as_tensor(a).to(DEV) for a in (obs, avail, adj, ch))
    t64 = lambda a: torch.as_tensor(a, dtype=R.F64)                          # noqa: E731
    g = torch.Generator().manual_seed(11)
    w_p, w_v = torch.randn(S, N, 5, generator=g), torch.randn(S, generator=g)
    spy.calls.clear()

    probs, _ = pol._probs(dobs, dav, dadj, dch)
    pol.zero_grad()
    (probs * w_p.to(DEV)).sum().backward()
    values, _ = crit._values_grad(dobs, dadj, dch)
    crit.zero_grad()
    (values * w_v.to(DEV)).sum().backward()
    # the any-width ops carry these gradients: policy + critic, each backward as often as its forward, no E = 64 entry point
    for op, n in (("cm_attention", 2), ("cm_masked_agg", 2 * hops)):
        assert spy.count(op + "_forward_any") == n and spy.count(op + "_backward_any") == n, (op, spy.calls)
        assert spy.count(op + "_forward") == 0 and spy.count(op + "_backward") == 0, (op, spy.calls)

    p64 = R.params(dict(pol.state_dict()))
    _, probs64, _ = R.policy_forward(p64, t64(obs), t64(avail), t64(adj), t64(ch), N, residual)
    (probs64 * w_p.to(R.F64)).sum().backward()
    c64 = R.params(dict(crit.state_dict()))
    values64 = R.critic_values(c64, t64(obs), t64(adj), t64(ch), N, residual, aggregator="sum")
    (values64 * w_v.to(R.F64)).sum().backward()
    assert R.ratio(probs, probs64) <= 1e-5 and R.ratio(values, values64) <= 1e-5

    worst, n = 0.0, 0
    for pre, net, ref in (("pol", pol, p64), ("crit", crit, c64)):
        for pname, p in net.named_parameters():
            if pname == "baseline_aggregator._init_std":                     # (the values do not depend on the std)
                continue
            want = (torch.zeros_like(ref[pname]) if ref[pname].grad is None else ref[pname].grad).numpy()
            got = np.zeros_like(want) if p.grad is None else p.grad.cpu().numpy()
            scale = max(float(np.abs(want).max()), 1e-6)
            worst = max(worst, float(np.abs(got - want).max()) / scale)
            np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5 * scale, err_msg=f"{pre} {pname}")
            n += 1
    assert n >= 20
    print(f"shape {shape}: {n} gradients, worst deviation / tensor scale {worst:.2e}")
    # negative control: the gradient of the GCN weight with the hops' channels in the other order (A) / without the masks (C)
    # must fail the same bound
    p64b = R.params(dict(pol.state_dict()))
    wrong_ch = t64(np.ascontiguousarray(ch[:, ::-1])) if hops > 1 else None
    _, pb, _ = R.policy_forward(p64b, t64(obs), t64(avail), t64(adj) if hops > 1 else None, wrong_ch, N, residual)
    (pb * w_p.to(R.F64)).sum().backward()
    want = p64b["gcn_layers.0.weight"].grad.numpy()
    got = pol.gcn_layers[0].weight.grad.cpu().numpy()
    assert not np.allclose(got, want, rtol=1e-4, atol=1e-5 * float(np.abs(want).max()))


def test_deterministic_backward_passes_are_bit_identical(torch_cuda):
    torch = torch_cuda
    import com_marl_amd
    s = G.SHAPES["A"]
    pol, crit = _nets("A", torch)
    obs, avail, adj, ch = (torch.as_tensor(a).to(DEV) for a in G.inputs(s["N"], s["d"], s["hops"], S=2300))
    g = torch.Generator().manual_seed(12)
    w_p, w_v = torch.randn(2300, s["N"], 5, generator=g).to(DEV), torch.randn(2300, generator=g).to(DEV)
    com_marl_amd.set_deterministic(True)
    try:
        runs = []
        for _ in range(2):
            pol.zero_grad()
            crit.zero_grad()
            (pol._probs(obs, avail, adj, ch)[0] * w_p).sum().backward()
            (crit._values_grad(obs, adj, ch)[0] * w_v).sum().backward()
            runs.append([p.grad.clone() for net in (pol, crit) for p in net.parameters() if p.grad is not None])
    finally:
        com_marl_amd.set_deterministic(None)
    assert len(runs[0]) == len(runs[1]) >= 20
    for a, b in zip(*runs):
        assert torch.equal(a, b)
