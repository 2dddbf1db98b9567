"""nets._AttentionSoftmax and nets._MaskedAggregate serve both kernel families - E = 64 (cm_attention_*, cm_masked_agg_*) and
any width (their _any forms) - chosen by their `any_width` argument.  One case per family at S = 3, N = 4, two hops:
AttentionModule and masked_aggregate, forward and backward, with and without channels, with and without bias.  Asserted: the
entry points that ran (the proxy of tests/lib_spy.py around com_marl_amd._lib.lib()) and the results against the framework
formula in float64 - softmax(q e^T); tanh of the row-renormalised M.R.C times HW plus b - with the metric, the term scales and
the bound TAU = 1e-5 tests/test_any_width_graph_ops.py applies to the same quantities.  The 'dot' module feeds the embedding in
as query and key, so its gradient is d_q + d_e, held against the sum of their term scales - of the rows and of the tensor, as
that file's "peaked" variant is: with q = e the diagonal score |e_i|^2 (~25 at E = 64) dwarfs the others, the softmax rows are
one-hot to float32 and the softmax backward is a difference of equal terms (float32 framework arithmetic is 1e-2 of max|ref|
off there, 3e-8 of the terms).  The op called on separate q and e (rows ~0.7 peaked) holds d_q and d_e each on its own."""
import pytest
import torch

from tests import f64_commnet as R
from tests.lib_spy import spy  # noqa: F401  (the fixture: a recording proxy around _lib.lib())
from tests.test_any_width_graph_ops import _agg_ref, _attention_inputs
from tests.test_backward_kernels_f64 import TAU, _agg_attn_terms, _attn_ref, _check, _masks, _record

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64 = torch.float64
S, N, HOPS = 3, 4, 2
OPS = ("cm_attention_forward", "cm_attention_backward", "cm_masked_agg_forward", "cm_masked_agg_backward")


def _f(t):
    return None if t is None else t.to(F64)


@pytest.mark.parametrize("E", [64, 32], ids=["E64", "any-width-E32"])
def test_folded_graph_ops_run_their_family_and_match_the_formula(E, spy):
    from com_marl_amd import nets
    any_width = E != 64
    mine = {n + "_any" if any_width else n for n in OPS}
    other = {n if any_width else n + "_any" for n in OPS}
    rows = S * N
    worst = {}
    g = torch.Generator().manual_seed(7 + E)

    # attention: the module ('dot': q is e), then the op on separate q and e
    q, e = (t.to(DEV) for t in _attention_inputs(g, S, N, E, False))
    d_m = torch.randn(S, N, N, generator=g).to(DEV)
    spy.calls.clear()
    x = e.clone().requires_grad_(True)
    m = nets.AttentionModule(E, "dot").to(DEV)(x)
    (d_x,) = torch.autograd.grad(m, (x,), d_m)
    assert spy.calls == [n for n in sorted(mine, reverse=True) if "attention" in n], spy.calls       # forward, then backward
    _check("module", "m", m, torch.softmax(_f(e) @ _f(e).transpose(-2, -1), dim=-1), worst, TAU, rows=rows)
    rq, re, sq, se = _attn_ref(e, e, m.detach(), d_m, None, None)
    _check("module", "d_q + d_e", d_x, rq + re, worst, TAU, rows=rows, row_terms=sq + se, tensor_terms=sq + se)
    ql, el = q.clone().requires_grad_(True), e.clone().requires_grad_(True)
    m = nets._AttentionSoftmax.apply(ql, el, any_width)
    d_q, d_e = torch.autograd.grad(m, (ql, el), d_m)
    _check("op", "m", m, torch.softmax(_f(q) @ _f(e).transpose(-2, -1), dim=-1), worst, TAU, rows=rows)
    rq, re, sq, se = _attn_ref(q, e, m.detach(), d_m, None, None)
    _check("op", "d_q", d_q, rq, worst, TAU, rows=rows, row_terms=sq)
    _check("op", "d_e", d_e, re, worst, TAU, rows=rows, row_terms=se)

    # masked aggregation: (channels and adjacency | neither) x (bias | none)
    attn0 = m.detach()
    adj, ch = (t.to(DEV) for t in _masks(g, S, N, HOPS, False))
    hw0 = (torch.randn(S, N, E, generator=g) * 0.5).to(DEV)
    bias0 = (torch.randn(E, generator=g) * 0.1).to(DEV)
    d_out = torch.randn(S, N, E, generator=g).to(DEV)
    for masks in (True, False):
        for has_bias in (True, False):
            case = f"agg masks={masks} bias={has_bias}"
            hop = 1
            a_adj, a_ch, chan_l = (adj, ch, ch[:, hop]) if masks else (None, None, None)
            attn, hw = attn0.clone().requires_grad_(True), hw0.clone().requires_grad_(True)
            bias = bias0.clone().requires_grad_(True) if has_bias else None
            n0 = len(spy.calls)
            out = nets.masked_aggregate(attn, a_adj, a_ch, hop, hw, bias)
            grads = torch.autograd.grad(out, (attn, hw) + ((bias,) if has_bias else ()), d_out)
            assert spy.calls[n0:] == [n for n in sorted(mine, reverse=True) if "masked_agg" in n], spy.calls[n0:]
            _check(case, "out", out, R.aggregate(_f(attn0), _f(a_adj), _f(chan_l), _f(hw0), _f(bias0) if has_bias else None), worst, TAU)
            ra, rh, rb = _agg_ref(attn0, a_adj, chan_l, hw0, out.detach(), d_out, has_bias)
            ta = _agg_attn_terms(attn0, a_adj, chan_l, hw0, out.detach(), d_out)
            _check(case, "d_attn", grads[0], ra, worst, TAU, rows=rows, row_terms=ta)
            _check(case, "d_hw", grads[1], rh, worst, TAU, rows=rows)
            if has_bias:
                _check(case, "d_bias", grads[2], rb, worst, TAU)
            if masks:                                        # the other hop's channels must fail the same bound
                wrong = R.aggregate(_f(attn0), _f(adj), _f(ch[:, 0]), _f(hw0), _f(bias0) if has_bias else None)
                assert float((_f(out.detach()) - wrong).abs().max()) > TAU * float(wrong.abs().max()), case
    assert spy.names() == mine and not (spy.names() & other), spy.calls
    _record(f"folded graph ops E={E}", worst)
