"""The graph ops for any embedding width (csrc/cm_graph_any.hip), called through the C ABI:

  cm_masked_agg_forward_any / cm_attention_forward_any
  cm_masked_agg_backward_any / _any_det     channels of hop l of L (pointer offset + stride), out_minus NULL or set, bias NULL or set
  cm_attention_backward_any                 d_e_add0 / d_e_add1 each NULL or set

against a float64 reference of the same operation built from tests/f64_commnet.py (R.masked_weights, R.aggregate,
R.attention_scores' products), exactly as tests/test_backward_kernels_f64.py judges the E = 64 kernels: its metric (strict
and applied, see its header for where and why they differ), its bound TAU = 1e-5 of scale, its negative controls.  The
reference takes the kernel's own float32 inputs widened to float64.  Outputs the kernels write are pre-filled with NaN, as
is the slab of the _det twin; d_bias starts at zero.

Cases (N, E, S), the smallest at which each mapping can go wrong: one column; shape A; E no multiple of 16 with N no multiple
of 4; rows of 400 B; shape B; 48 columns; three 16-row tiles with a ragged E; the largest width that must fit; and more
chunks than the grid cap with a ragged tail (N = 5 takes one env per workgroup: 2300 chunks over grids of 2048 / 1024).

LDS at (80, 128): one env per workgroup, row strides NP = 81 and SE = 132; the largest need is the aggregation backward's,
2 x 6480 (A, dA) + 2 x 10560 (HW, dP) + 2 x 80 (row sums) + 256 (bias partials) floats = 137 984 bytes of the 163 840."""
import time

import pytest
import torch

from tests import f64_commnet as R
from tests.test_backward_kernels_f64 import (TAU, _agg_attn_terms, _attn_ref, _check, _masks, _metric, _nan, _record,  # noqa: F401
                                             _reject, _slab)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64 = torch.float64

CASES = [
    (4, 1, 15, "one column"),
    (4, 32, 37, "shape A"),
    (5, 12, 33, "E no multiple of 16, N no multiple of 4"),
    (3, 100, 9, "rows of 400 B"),
    (24, 32, 9, "shape B"),
    (24, 48, 9, "48 columns"),
    (33, 20, 5, "three row tiles, ragged E"),
    (80, 128, 3, "largest width that must fit"),
    (5, 12, 2300, "grid-stride loop: more chunks than the grid cap, ragged tail"),
]
IDS = [f"N{n}-E{e}-S{s}" for n, e, s, _ in CASES]


def _lib():
    from com_marl_amd import _lib as L
    return L


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _cuda(t):
    return None if t is None else t.to(DEV).contiguous()


# ------------------------------------------------------------------------------------------------------------------
# inputs (the builders of tests/test_backward_kernels_f64.py with the width as a parameter)
# ------------------------------------------------------------------------------------------------------------------
def _attention_inputs(g, S, N, E, peaked):
    e = torch.tanh(torch.randn(S, N, E, generator=g))
    wq = torch.randn(E, E, generator=g) * (0.8 if peaked else 0.12 * (64.0 / E) ** 0.5)
    q = e @ wq.T
    if peaked:                                       # scores around +-40: near one-hot softmax rows
        s = q @ e.transpose(-2, -1)
        q = q * (40.0 / s.abs().amax(dim=(-2, -1), keepdim=True).clamp(min=1e-6))
    return q.float(), e.float()


def _agg_inputs(N, E, S, variant, seed):
    """-> dict of device tensors: attn, adj | None, ch [S,L,N,N] | None, hop, hw, bias | None, y (the op's output), minus | None,
    out (= y + minus, what the caller holds), d_out."""
    with_adj, chv, use_minus, has_bias, edge = variant
    g = torch.Generator().manual_seed(seed)
    Lh, hop = chv if chv is not None else (1, 0)
    adj, ch = _masks(g, S, N, Lh, edge == "masked_row")
    q, e = _attention_inputs(g, S, N, E, False)
    attn = torch.softmax(q.to(F64) @ e.to(F64).transpose(-2, -1), dim=-1).float()
    hw = torch.randn(S, N, E, generator=g) * 0.5
    bias = torch.randn(E, generator=g) * 0.1
    if edge == "saturated":                                         # most pre-activations beyond +-5, whatever N averages over
        bias = bias + 6.0 * torch.sign(torch.randn(E, generator=g))
    z = R.masked_weights(attn.to(F64), adj.to(F64) if with_adj else None, ch[:, hop].to(F64) if chv else None) @ hw.to(F64)
    y = torch.tanh(z + bias.to(F64) if has_bias else z).float()
    if edge == "saturated":
        assert float((y.abs() > 0.9999).float().mean()) > 0.2
    d_out = torch.randn(S, N, E, generator=g)
    minus = torch.tanh(torch.randn(S, N, E, generator=g)) if use_minus else None     # E of x = E + H_L
    out = (y + minus) if use_minus else y
    c = dict(attn=_cuda(attn), adj=_cuda(adj if with_adj else None), ch=_cuda(ch if chv else None), hop=hop, L=Lh, hw=_cuda(hw),
             bias=_cuda(bias if has_bias else None), out=_cuda(out), minus=_cuda(minus), d_out=_cuda(d_out))
    c["chan_l"] = c["ch"][:, hop] if chv else None
    c["y"] = (c["out"] - c["minus"]) if use_minus else c["out"]     # the float32 difference the kernel forms
    return c


def _chan_args(c, N, hop=None):
    if c["ch"] is None:
        return None, 0
    hop = c["hop"] if hop is None else hop
    return c["ch"].data_ptr() + 4 * hop * N * N, c["ch"].shape[1] * N * N


def _agg_ref(attn, adj, chan_l, hw, y, d_out, has_bias):
    """d_attn, d_hw, d_bias of out = tanh(A(attn) hw + b) given its saved tanh output y (float64, autograd for the A part)."""
    E = hw.shape[-1]
    a64 = attn.to(F64).requires_grad_(True)
    hw64 = hw.to(F64).requires_grad_(True)
    b64 = torch.zeros(E, dtype=F64, device=attn.device, requires_grad=True)
    z = R.masked_weights(a64, None if adj is None else adj.to(F64), None if chan_l is None else chan_l.to(F64)) @ hw64 + b64
    dz = d_out.to(F64) * (1 - y.to(F64) ** 2)                      # graph_conv_module.py:231 tanh' from the saved output
    da, dh, db = torch.autograd.grad(z, (a64, hw64, b64), dz)
    return da, dh, (db if has_bias else None)


def _agg_bwd_call(S, N, E, c, det):
    L = _lib()
    lib = L.lib()
    d_attn, d_hw = _nan(S, N, N), _nan(S, N, E)
    d_bias = torch.zeros(E, device=DEV) if c["bias"] is not None else None
    chan_ptr, stride = _chan_args(c, N)
    args = (S, N, E, _p(c["attn"]), _p(c["adj"]), chan_ptr, stride, _p(c["hw"]), _p(c["out"]), _p(c["minus"]), _p(c["d_out"]),
            _p(d_attn), _p(d_hw), _p(d_bias))
    if det:
        nb = lib.cm_masked_agg_backward_any_det_ws_bytes(S, N, E)
        slab = _slab(nb)
        rc = lib.cm_masked_agg_backward_any_det(*args, _p(slab), nb, _stream())
    else:
        rc = lib.cm_masked_agg_backward_any(*args, _stream())
    L.check(rc, "cm_masked_agg_backward_any")
    torch.cuda.synchronize()
    return d_attn, d_hw, d_bias


# (with_adj, channels (L, l) | None, out_minus, bias, edge)
AGG_VARIANTS = [
    (True, (2, 1), True, True, "none"),              # with adj, hop 1 of 2 channels, out_minus and bias
    (True, (3, 0), False, True, "masked_row"),       # a fully masked row, hop 0 of 3, no minus
    (False, None, False, True, "saturated"),         # no masks, saturated tanh, with bias
    (True, None, True, False, "none"),               # no bias: the twin has no cross-workgroup sum left
]


# ------------------------------------------------------------------------------------------------------------------
# masked aggregation
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("N,E,S,what", CASES, ids=IDS)
def test_masked_agg_backward_any(N, E, S, what, det):
    t0 = time.time()
    worst = {}
    for vi, variant in enumerate(AGG_VARIANTS):
        case = f"agg N={N} E={E} S={S} {'det' if det else 'atomic'} v{vi} [{what}]"
        c = _agg_inputs(N, E, S, variant, seed=1000 * N + 10 * E + S + vi)
        has_bias = c["bias"] is not None
        ra, rh, rb = _agg_ref(c["attn"], c["adj"], c["chan_l"], c["hw"], c["y"], c["d_out"], has_bias)
        ga, gh, gb = _agg_bwd_call(S, N, E, c, det)
        ta = _agg_attn_terms(c["attn"], c["adj"], c["chan_l"], c["hw"], c["y"], c["d_out"])
        kw_a, kw_h = dict(rows=S * N, row_terms=ta), dict(rows=S * N)      # d_attn rows: cancelling sums
        _check(case, "d_attn", ga, ra, worst, TAU, **kw_a)
        _check(case, "d_hw", gh, rh, worst, TAU, **kw_h)
        if has_bias:
            _check(case, "d_bias", gb, rb, worst, TAU)
        # negative controls: each plausible wrong answer must fail the same tolerance
        wa, wh = ra.clone(), rh.clone()
        wa[-1], wh[-1] = 0, 0
        _reject(case, "without the last env", [(ga, wa, kw_a), (gh, wh, kw_h)], TAU)
        if c["ch"] is not None and c["L"] > 1:
            other = c["hop"] + 1 if c["hop"] + 1 < c["L"] else c["hop"] - 1
            wa2, wh2, _ = _agg_ref(c["attn"], c["adj"], c["ch"][:, other], c["hw"], c["y"], c["d_out"], False)
            _reject(case, f"channels of hop {other}", [(ga, wa2, kw_a), (gh, wh2, kw_h)], TAU)
        if c["minus"] is not None:
            wa3, wh3, _ = _agg_ref(c["attn"], c["adj"], c["chan_l"], c["hw"], c["out"], c["d_out"], False)
            _reject(case, "no out_minus", [(ga, wa3, kw_a), (gh, wh3, kw_h)], TAU)
    _record(f"agg bwd N={N} E={E} S={S} {'det' if det else 'atomic'} ({time.time() - t0:.1f}s)", worst)


@pytest.mark.parametrize("N,E,S,what", CASES, ids=IDS)
def test_masked_agg_forward_any(N, E, S, what):
    L = _lib()
    lib = L.lib()
    worst = {}
    for vi, variant in enumerate(AGG_VARIANTS):
        case = f"agg fwd N={N} E={E} S={S} v{vi} [{what}]"
        c = _agg_inputs(N, E, S, variant, seed=3000 * N + 10 * E + S + vi)
        out = _nan(S, N, E)
        chan_ptr, stride = _chan_args(c, N)
        L.check(lib.cm_masked_agg_forward_any(S, N, E, _p(c["attn"]), _p(c["adj"]), chan_ptr, stride, _p(c["hw"]), _p(c["bias"]), _p(out),
                                              _stream()), "cm_masked_agg_forward_any")
        torch.cuda.synchronize()
        f = lambda t: None if t is None else t.to(F64)                       # noqa: E731
        ref = R.aggregate(f(c["attn"]), f(c["adj"]), f(c["chan_l"]), f(c["hw"]), f(c["bias"]))
        if variant[4] == "masked_row":                                       # agent 0 of env 0 hears nobody: tanh(b)
            want = torch.tanh(f(c["bias"])) if c["bias"] is not None else torch.zeros(E, dtype=F64, device=DEV)
            assert float((ref[0, 0] - want).abs().max()) < 1e-12
        _check(case, "out", out, ref, worst, TAU)
        wrong = ref.clone()
        wrong[-1] = 0
        _reject(case, "without the last env", [(out, wrong, {})], TAU)
        if c["ch"] is not None and c["L"] > 1:
            other = c["hop"] + 1 if c["hop"] + 1 < c["L"] else c["hop"] - 1
            _reject(case, f"channels of hop {other}",
                    [(out, R.aggregate(f(c["attn"]), f(c["adj"]), f(c["ch"][:, other]), f(c["hw"]), f(c["bias"])), {})], TAU)
    _record(f"agg fwd N={N} E={E} S={S}", worst)


@pytest.mark.parametrize("N,E,S", [(4, 32, 37), (24, 32, 9), (5, 12, 2300)])
def test_det_twin_repeats_bit_for_bit(N, E, S):
    c = _agg_inputs(N, E, S, AGG_VARIANTS[0], seed=99 + N)
    a = _agg_bwd_call(S, N, E, c, True)
    b = _agg_bwd_call(S, N, E, c, True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------------------------
ATTN_VARIANTS = [(True, True, "none"), (False, True, "peaked"), (True, False, "none"), (False, False, "none")]


@pytest.mark.parametrize("N,E,S,what", CASES, ids=IDS)
def test_attention_backward_any(N, E, S, what):
    t0 = time.time()
    L = _lib()
    lib = L.lib()
    worst = {}
    for vi, (has0, has1, edge) in enumerate(ATTN_VARIANTS):
        case = f"attn N={N} E={E} S={S} v{vi} [{what}]"
        g = torch.Generator().manual_seed(2000 * N + 10 * E + S + vi)
        q, e = _attention_inputs(g, S, N, E, edge == "peaked")
        m = torch.softmax(q.to(F64) @ e.to(F64).transpose(-2, -1), dim=-1).float()
        if edge == "peaked" and E >= 12:                                     # (one or four columns: rank-deficient scores)
            assert float(m.amax(-1).mean()) > 0.8
        d_m = torch.randn(S, N, N, generator=g)
        add0 = torch.randn(S, N, E, generator=g) * 0.3 if has0 else None
        add1 = torch.randn(S, N, E, generator=g) * 0.3 if has1 else None
        q, e, m, d_m, add0, add1 = map(_cuda, (q, e, m, d_m, add0, add1))
        dq, de = _nan(S, N, E), _nan(S, N, E)
        L.check(lib.cm_attention_backward_any(S, N, E, _p(q), _p(e), _p(m), _p(d_m), _p(add0), _p(add1), _p(dq), _p(de), _stream()),
                "cm_attention_backward_any")
        torch.cuda.synchronize()
        rq, re, sq, se = _attn_ref(q, e, m, d_m, add0, add1)
        kw_q = dict(rows=S * N, row_terms=sq, tensor_terms=sq if edge == "peaked" else None)
        kw_e = dict(rows=S * N, row_terms=se, tensor_terms=se if edge == "peaked" else None)
        _check(case, "d_q", dq, rq, worst, **kw_q)
        _check(case, "d_e", de, re, worst, **kw_e)
        wq, we = rq.clone(), re.clone()
        wq[-1], we[-1] = 0, 0
        _reject(case, "without the last env", [(dq, wq, kw_q), (de, we, kw_e)])
        for nm, a in (("d_e_add0", add0), ("d_e_add1", add1)):
            if a is not None:
                _reject(case, f"missing {nm}", [(de, re - a.to(F64), kw_e)])
    _record(f"attn bwd N={N} E={E} S={S} ({time.time() - t0:.1f}s)", worst)


@pytest.mark.parametrize("N,E,S,what", CASES, ids=IDS)
def test_attention_forward_any(N, E, S, what):
    L = _lib()
    lib = L.lib()
    worst = {}
    case = f"attn fwd N={N} E={E} S={S} [{what}]"
    g = torch.Generator().manual_seed(4000 * N + 10 * E + S)
    q, e = map(_cuda, _attention_inputs(g, S, N, E, False))
    m = _nan(S, N, N)
    L.check(lib.cm_attention_forward_any(S, N, E, _p(q), _p(e), _p(m), _stream()), "cm_attention_forward_any")
    torch.cuda.synchronize()
    ref = torch.softmax(q.to(F64) @ e.to(F64).transpose(-2, -1), dim=-1)      # f64_commnet.attention_scores + softmax
    _check(case, "m", m, ref, worst, TAU, rows=S * N)
    wrong = ref.clone()
    wrong[-1] = 0
    _reject(case, "without the last env", [(m, wrong, dict(rows=S * N))])
    _record(case, worst)


def test_attention_backward_any_refuses_aliasing():
    lib = _lib().lib()
    t = torch.zeros(2, 4, 32, device=DEV)
    m = torch.zeros(2, 4, 4, device=DEV)
    assert lib.cm_attention_backward_any(2, 4, 32, _p(t), _p(t), _p(m), _p(m), _p(t), None, _p(t.clone()), _p(t), _stream()) != 0
    assert lib.cm_attention_backward_any(2, 4, 32, _p(t), _p(t), _p(m), _p(m), None, _p(t), _p(t.clone()), _p(t), _stream()) != 0


# ------------------------------------------------------------------------------------------------------------------
# shapes the kernels do not take
# ------------------------------------------------------------------------------------------------------------------
def test_planes_that_do_not_fit_answer_1_and_write_nothing():
    lib = _lib().lib()
    S, N, E = 2, 128, 128
    attn, hw = torch.rand(S, N, N, device=DEV), torch.rand(S, N, E, device=DEV)
    out, m = _nan(S, N, E), _nan(S, N, N)
    d_attn, d_hw, d_bias = _nan(S, N, N), _nan(S, N, E), torch.zeros(E, device=DEV)
    st = _stream()
    assert lib.cm_masked_agg_forward_any(S, N, E, _p(attn), None, None, 0, _p(hw), None, _p(out), st) == 1
    assert lib.cm_attention_forward_any(S, N, E, _p(hw), _p(hw), _p(m), st) == 1
    assert lib.cm_masked_agg_backward_any(S, N, E, _p(attn), None, None, 0, _p(hw), _p(hw), None, _p(hw), _p(d_attn), _p(d_hw), _p(d_bias),
                                          st) == 1
    assert lib.cm_attention_backward_any(S, N, E, _p(hw), _p(hw), _p(attn), _p(attn), None, None, _p(out), _p(d_hw), st) == 1
    torch.cuda.synchronize()
    for t in (out, m, d_attn, d_hw):
        assert bool(torch.isnan(t).all())
    assert float(d_bias.abs().max()) == 0.0
    for bad in (0, 129):
        assert lib.cm_masked_agg_forward_any(S, 4, bad, _p(attn), None, None, 0, _p(hw), None, _p(out), st) < 0
        assert lib.cm_attention_forward_any(S, 4, bad, _p(hw), _p(hw), _p(m), st) < 0
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(m).all())
