"""The three backward entry points of the fused training path, called through the C ABI with every argument that path
passes (com-marl_amd/nets/comm.py _FusedNetFn.backward), against a float64 reference of the same operation built from
tests/f64_commnet.py (torch float64 on the GPU: it shares no code with the kernels):

  cm_masked_agg_backward_r / _det  channels of hop l of L (pointer offset + stride), out_minus NULL or set, bias_replicas 1 or 32
  cm_attention_backward            d_e_add0 / d_e_add1 each NULL or set
  cm_encoder_backward / _det       dy2 NULL or set; rc = 1 (nothing launched) for d > 64

The reference takes the kernel's own float32 inputs - the saved forward outputs included - widened to float64, so it
restates the operation, not the rounding of an earlier one.  An element a kernel leaves unwritten, or a slab row it reads
before writing, fails (NaN).

Metric: max|got - ref64| <= 1e-5 * max|ref64| for every tensor, and per agent row (each row against its own max|ref64|)
for d_attn, d_hw, d_q, d_e.  Every case prints the worst STRICT ratio (that metric) and the worst APPLIED one.  The applied
metric differs from the strict one only where the strict one was measured to fail for arithmetic reasons, not kernel ones:

  * d_attn per row: d_attn_ij = mask_ij (g_ij - sum_k A_ik g_ik) / rowsum cancels to far below its terms; plain float32
    torch of the same formula misses rows by up to 7e-4 of their own size (the kernels by up to 5.4e-3 at S = 8192).  A
    row's scale is the larger of its max|ref| and the size of its terms, |mask| (|dz| |hw|^T) / rowsum.
  * d_q, d_e per row: the softmax backward ds = m (dm - <dm, m>) cancels likewise (kernels measured up to 2.3e-4 of a
    row); the row scale is the size of (m |dm| + m |<dm, m>|) carried through the same products.  With peaked scores
    (+-40) every row cancels, so there the TENSOR scale takes the same terms (strict miss up to 1.5e-2 at N = 4, S = 1).

Saturated tanh outputs (|y| > 0.9999) are held to the strict metric like the rest: the kernels form tanh' = 1 - y^2 with
one fma, exact to an ulp of the given y.  (Formed as 1 - fl(y * y), it lost up to 2^-24 absolute - ~6e-4 of tanh' where
1 - y^2 = 1e-4 - and missed d_hw / dw2 by up to 5e-4 of a row.)

Each case also asserts that the APPLIED metric REJECTS plausible wrong answers (negative controls): the last env dropped,
the channels of a neighbouring hop, no out_minus, only replica row 0 of the bias, a missing d_e_add* or dy2.  Outputs the
kernels write are pre-filled with NaN, as is the slab of each _det twin; accumulated outputs (d_bias, dw*, db*) start at
zero, as the ABI requires."""
import time

import pytest
import torch

from tests import f64_commnet as R

pytestmark = pytest.mark.gpu

TAU = 1e-5
DEV = "cuda:0"
F64 = torch.float64

# Which kernel a shape reaches (N: team size, S: envs).  Dispatchers: cm_graph_ops.hip masked_agg_backward (behind
# cm_masked_agg_backward_r / _det) and cm_attention_backward; matrix-core choice cm_graph_ops_mfma.hip agg_bwd_m (behind
# agg_bwd_mfma) / attn_bwd_mfma with NT = ceil(N / 16) and MAXNT = 2 (NT <= 2), 5 (NT <= 5), 8.
SHAPES = [
    # N, S, branch
    (4, 1, "quad kernels agg_bwd4 / attn_bwd4 (the N == 4 branches of masked_agg_backward, cm_attention_backward), one env"),
    (4, 15, "quad kernels, one ragged 16-env chunk"),
    (4, 8192, "quad kernels, 512 chunks: last grid of <= 64 workgroups looping (masked_agg_backward's grid choice)"),
    (4, 8193, "quad kernels, 513 chunks: grid 513 (masked_agg_backward's grid choice), ragged tail; the fused path's 32 bias "
              "replicas (nets._FusedNetFn.backward)"),
    (4, 40001, "quad kernels: agg_bwd4 grid capped at 2048 and looping (masked_agg_backward's grid choice), ragged tail"),
    (4, 70001, "quad kernels: attn_bwd4 grid capped at 4096 and looping (cm_attention_backward), ragged tail"),
    (3, 15, "first-generation agg_bwd_kernel / attn_bwd_kernel (N < 8: agg_bwd_mfma, attn_bwd_mfma return 1)"),
    (5, 1001, "first-generation kernels"),
    (6, 257, "first-generation kernels"),
    (8, 37, "matrix-core MAXNT 2 (NT 1), smallest N it takes (agg_bwd_mfma's N < 8 refusal)"),
    (32, 37, "matrix-core MAXNT 2 at its upper boundary (NT 2)"),
    (33, 15, "matrix-core MAXNT 5 at its lower boundary (NT 3)"),
    (80, 9, "matrix-core MAXNT 5 at its upper boundary (NT 5), largest fused team"),
    (81, 9, "matrix-core MAXNT 8 at its lower boundary (NT 6), per-layer team"),
    (128, 5, "matrix-core MAXNT 8 at its upper boundary (NT 8), MAX_KERNEL_AGENTS"),
]


def _lib():
    from com_marl_amd import _lib as L
    return L


def _p(t):
    return None if t is None else t.data_ptr()


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _slab(nb):
    return torch.full((max(1, (int(nb) + 3) // 4),), float("nan"), dtype=torch.float32, device=DEV)


def _metric(got, ref, rows=None, row_terms=None, tensor_terms=None):
    """-> (strict, applied).  strict = max(max|got - ref| / max|ref|, and with `rows` the same per row against the row's own
    max|ref|, floored at 1e-3 of the tensor's); applied = the same, except that a row's scale is max(row max|ref|, row max of
    `row_terms`) and the tensor's max(max|ref|, max `tensor_terms`) where those are given - the size of the terms an element
    is summed from, for the sums measured to cancel (see the header)."""
    g, r = got.detach().to("cpu", F64), ref.detach().to("cpu", F64)
    err = (g - r).abs()
    scale = max(float(r.abs().max()), 1e-6)
    strict = applied = float(err.max()) / scale
    if tensor_terms is not None:
        applied = float(err.max()) / max(scale, float(tensor_terms.detach().to("cpu", F64).max()))
    if rows is not None:
        e_row, r_row = err.reshape(rows, -1).amax(1), r.abs().reshape(rows, -1).amax(1)
        strict = max(strict, float((e_row / r_row.clamp(min=1e-3 * scale)).max()))
        if row_terms is not None:
            r_row = torch.maximum(r_row, row_terms.detach().to("cpu", F64).reshape(rows, -1).amax(1))
        applied = max(applied, float((e_row / r_row.clamp(min=1e-3 * scale)).max()))
    return strict, applied


def _check(case, name, got, ref, worst, tau=TAU, **terms):
    strict, applied = _metric(got, ref, **terms)
    s0, a0 = worst.get(name, (0.0, 0.0))
    worst[name] = (max(s0, strict), max(a0, applied))
    assert applied <= tau, f"{case}: {name} off by {applied:.3g} of its scale (strict {strict:.3g}; tolerance {tau})"


def _reject(case, what, pairs, tau=TAU):
    """Negative control: with the metric and scales `_check` applies, `got` must FAIL against at least one tensor of a
    plausible wrong answer.  pairs: (got, wrong, metric keywords)."""
    r = max(_metric(g, w, **kw)[1] for g, w, kw in pairs)
    assert r > tau, f"{case}: negative control '{what}' passes the tolerance (ratio {r:.3g}): the check is too loose"


def _record(case, worst):
    if not worst:
        return
    ks = max(worst, key=lambda k: worst[k][0])
    ka = max(worst, key=lambda k: worst[k][1])
    print(f"{case}: worst strict ratio {worst[ks][0]:.2e} ({ks}); worst applied ratio {worst[ka][1]:.2e} ({ka})")


# ------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------
def _masks(g, S, N, L, masked_row):
    adj = (torch.rand(S, N, N, generator=g) < 0.7).float()
    adj[:, torch.arange(N), torch.arange(N)] = 1.0
    ch = (torch.rand(S, L, N, N, generator=g) < 0.8).float()
    ch[:, :, torch.arange(N), torch.arange(N)] = 1.0
    if masked_row:                                   # agent 0 of env 0 hears nobody, itself included
        adj[0, 0, :] = 0.0
    return adj, ch


def _attention_inputs(g, S, N, peaked):
    e = torch.tanh(torch.randn(S, N, 64, generator=g))
    wq = torch.randn(64, 64, generator=g) * (0.8 if peaked else 0.12)
    q = e @ wq.T
    if peaked:                                       # scores around +-40: near one-hot softmax rows
        s = q @ e.transpose(-2, -1)
        q = q * (40.0 / s.abs().amax(dim=(-2, -1), keepdim=True).clamp(min=1e-6))
    return q.float(), e.float()


# ------------------------------------------------------------------------------------------------------------------
# masked aggregation backward
# ------------------------------------------------------------------------------------------------------------------
def _agg_ref(attn, adj, chan_l, hw, y, d_out, has_bias):
    """d_attn, d_hw, d_bias of out = tanh(A(attn) hw + b) given its saved tanh output y (float64, autograd for the A part)."""
    a64 = attn.to(F64).requires_grad_(True)
    hw64 = hw.to(F64).requires_grad_(True)
    b64 = torch.zeros(64, dtype=F64, device=attn.device, requires_grad=True)
    z = R.masked_weights(a64, None if adj is None else adj.to(F64), None if chan_l is None else chan_l.to(F64)) @ hw64 + b64
    dz = d_out.to(F64) * (1 - y.to(F64) ** 2)                      # graph_conv_module.py:231 tanh' from the saved output
    da, dh, db = torch.autograd.grad(z, (a64, hw64, b64), dz)
    return da, dh, (db if has_bias else None)


def _agg_attn_terms(attn, adj, chan_l, hw, y, d_out):
    """Term sizes of d_attn_ij = mask_ij (g_ij - sum_k A_ik g_ik) / rowsum, g = dz hw^T: |mask| (|dz| |hw|^T) / rowsum."""
    mask = torch.ones_like(attn, dtype=F64)
    if adj is not None:
        mask = mask * adj.to(F64)
    if chan_l is not None:
        mask = mask * chan_l.to(F64)
    dzs = d_out.to(F64).abs() * (1 - y.to(F64) ** 2).abs()
    rs = (attn.to(F64) * mask).sum(-1, keepdim=True) + 1e-12
    return mask * (dzs @ hw.to(F64).abs().transpose(-2, -1)) / rs


def _agg_call(S, N, attn, adj, chan_all, hop, hw, out, minus, d_out, reps, det, has_bias):
    L = _lib()
    lib = L.lib()
    d_attn, d_hw = _nan(S, N, N), _nan(S, N, 64)
    d_bias = torch.zeros(reps, 64, device=DEV) if has_bias else None
    chan_ptr, stride = None, 0
    if chan_all is not None:
        chan_ptr, stride = chan_all.data_ptr() + 4 * hop * N * N, chan_all.shape[1] * N * N
    st = torch.cuda.current_stream().cuda_stream
    if det:
        nb = lib.cm_masked_agg_backward_det_ws_bytes(S, N, 64)
        slab = _slab(nb)
        rc = lib.cm_masked_agg_backward_det(S, N, 64, _p(attn), _p(adj), chan_ptr, stride, _p(hw), _p(out), _p(minus), _p(d_out),
                                            _p(d_attn), _p(d_hw), _p(d_bias), _p(slab), nb, st)
    else:
        rc = lib.cm_masked_agg_backward_r(S, N, 64, _p(attn), _p(adj), chan_ptr, stride, _p(hw), _p(out), _p(minus), _p(d_out),
                                          _p(d_attn), _p(d_hw), _p(d_bias), reps, st)
    L.check(rc, "cm_masked_agg_backward")
    torch.cuda.synchronize()
    return d_attn, d_hw, d_bias


# (with_adj, channels (L, l) | None, out_minus, bias_replicas, bias, edge)
AGG_VARIANTS = [
    (True, (2, 1), True, 32, True, "none"),          # the fused path's last hop of 2 (nets._FusedNetFn.backward's hop loop)
    (True, (3, 0), False, 1, True, "masked_row"),
    (False, (4, 2), False, 1, True, "saturated"),
    (True, None, True, 32, False, "peaked"),
    (False, None, False, 1, True, "none"),
]


def _agg_case(N, S, variant, det, seed):
    with_adj, chv, use_minus, reps, has_bias, edge = variant
    if det:
        reps = 1                                                    # the _det twin has one bias row (nets._FusedNetFn.backward)
    g = torch.Generator().manual_seed(seed)
    Lh, hop = chv if chv is not None else (1, 0)
    adj, ch = _masks(g, S, N, Lh, edge == "masked_row")
    q, e = _attention_inputs(g, S, N, edge == "peaked")
    attn = torch.softmax(q.to(F64) @ e.to(F64).transpose(-2, -1), dim=-1).float()
    hw = torch.randn(S, N, 64, generator=g) * 0.5
    bias = torch.randn(64, generator=g) * 0.1
    if edge == "saturated":                                         # most pre-activations beyond +-5, whatever N averages over
        bias = bias + 6.0 * torch.sign(torch.randn(64, generator=g))
    z = R.masked_weights(attn.to(F64), adj.to(F64) if with_adj else None, ch[:, hop].to(F64) if chv else None) @ hw.to(F64)
    y = torch.tanh(z + bias.to(F64)).float()
    if edge == "saturated":                                         # rows of |y| > 0.9999 (tanh' ~ 1e-4)
        assert float((y.abs() > 0.9999).float().mean()) > 0.2
    d_out = torch.randn(S, N, 64, generator=g)
    minus = torch.tanh(torch.randn(S, N, 64, generator=g)) if use_minus else None     # E of x = E + H_L
    out = (y + minus) if use_minus else y
    cuda = lambda t: None if t is None else t.to(DEV).contiguous()       # noqa: E731
    attn_d, adj_d, ch_d, hw_d, out_d, minus_d, dout_d = map(cuda, (attn, adj if with_adj else None, ch if chv else None, hw, out,
                                                                     minus, d_out))
    y_d = (out_d - minus_d) if use_minus else out_d                 # the float32 difference the kernel forms
    chan_l = ch_d[:, hop] if chv else None
    ref = _agg_ref(attn_d, adj_d, chan_l, hw_d, y_d, dout_d, has_bias)
    got = _agg_call(S, N, attn_d, adj_d, ch_d, hop, hw_d, out_d, minus_d, dout_d, reps, det, has_bias)
    return dict(ref=ref, got=got, attn=attn_d, adj=adj_d, ch=ch_d, hop=hop, L=Lh, hw=hw_d, out=out_d, minus=minus_d,
                d_out=dout_d, reps=reps, has_bias=has_bias)


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("N,S,branch", SHAPES, ids=[f"N{n}-S{s}" for n, s, _ in SHAPES])
def test_masked_agg_backward(N, S, branch, det):
    t0 = time.time()
    worst = {}
    variants = AGG_VARIANTS if S * N <= 40000 else AGG_VARIANTS[:2]          # (the large batches: the fused path's two shapes)
    for vi, variant in enumerate(variants):
        case = f"agg N={N} S={S} {'det' if det else 'atomic'} v{vi} [{branch}]"
        c = _agg_case(N, S, variant, det, seed=1000 * N + S + vi)
        (ra, rh, rb), (ga, gh, gb) = c["ref"], c["got"]
        tau = TAU
        y = (c["out"] - c["minus"]) if c["minus"] is not None else c["out"]
        ta = _agg_attn_terms(c["attn"], c["adj"], None if c["ch"] is None else c["ch"][:, c["hop"]], c["hw"], y, c["d_out"])
        kw_a, kw_h = dict(rows=S * N, row_terms=ta), dict(rows=S * N)      # d_attn rows: cancelling sums (header)
        _check(case, "d_attn", ga, ra, worst, tau, **kw_a)
        _check(case, "d_hw", gh, rh, worst, tau, **kw_h)
        if c["has_bias"]:
            _check(case, "d_bias", gb.sum(0), rb, worst, tau)
        # negative controls: each plausible wrong answer must fail the same tolerance
        wa, wh = ra.clone(), rh.clone()
        wa[-1], wh[-1] = 0, 0                                               # the last env left out
        _reject(case, "without the last env", [(ga, wa, kw_a), (gh, wh, kw_h)], tau)
        if c["ch"] is not None and c["L"] > 1:
            other = c["hop"] + 1 if c["hop"] + 1 < c["L"] else c["hop"] - 1
            y = (c["out"] - c["minus"]) if c["minus"] is not None else c["out"]
            wa2, wh2, _ = _agg_ref(c["attn"], c["adj"], c["ch"][:, other], c["hw"], y, c["d_out"], False)
            _reject(case, f"channels of hop {other}", [(ga, wa2, kw_a), (gh, wh2, kw_h)], tau)
        if c["minus"] is not None:
            wa3, wh3, _ = _agg_ref(c["attn"], c["adj"], None if c["ch"] is None else c["ch"][:, c["hop"]], c["hw"], c["out"],
                                   c["d_out"], False)
            _reject(case, "no out_minus", [(ga, wa3, kw_a), (gh, wh3, kw_h)], tau)
        if c["has_bias"] and c["reps"] > 1 and N == 4 and S > 16:     # (the quad kernel spreads; the others add into row 0)
            assert int((gb.abs().sum(1) > 0).sum()) > 1, f"{case}: the bias gradient was not spread over replicas"
            _reject(case, "only replica row 0 of the bias", [(gb[0], rb, {})], tau)
    _record(f"agg N={N} S={S} {'det' if det else 'atomic'} ({time.time() - t0:.1f}s)", worst)


def test_masked_agg_backward_replicas_elsewhere_sum_to_the_bias():
    """bias_replicas = 32 off the quad kernels (N = 24: matrix core; N = 5: first generation): whatever rows they use, the
    rows sum to the reference."""
    for N, S in ((24, 9), (5, 33)):
        c = _agg_case(N, S, AGG_VARIANTS[0], False, seed=7 + N)
        _check(f"agg reps32 N={N}", "d_bias", c["got"][2].sum(0), c["ref"][2], {})


def test_masked_agg_backward_refuses_bad_arguments():
    L = _lib()
    lib = L.lib()
    S, N = 3, 4
    t = lambda *s: torch.zeros(*s, device=DEV)                              # noqa: E731
    a, h = t(S, N, N), t(S, N, 64)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.cm_masked_agg_backward_r(S, N, 64, _p(a), None, None, 0, _p(h), _p(h), None, _p(h), _p(a), _p(h), None, 0, st) != 0
    assert lib.cm_masked_agg_backward_r(S, N, 32, _p(a), None, None, 0, _p(h), _p(h), None, _p(h), _p(a), _p(h), None, 1, st) != 0


# ------------------------------------------------------------------------------------------------------------------
# attention backward
# ------------------------------------------------------------------------------------------------------------------
def _attn_ref(q, e, m, d_m, add0, add1):
    """d_q, d_e of m = softmax_j(q_i . e_j) (f64_commnet.attention_scores + softmax) given the saved m, plus the addends."""
    q64, e64 = q.to(F64).requires_grad_(True), e.to(F64).requires_grad_(True)
    s = q64 @ e64.transpose(-2, -1)
    m64 = m.to(F64)
    # softmax backward from the saved probabilities: ds = m * (dm - <dm, m>)
    dm = d_m.to(F64)
    ds = m64 * (dm - (dm * m64).sum(-1, keepdim=True))
    dq, de = torch.autograd.grad(s, (q64, e64), ds)
    # per-row sizes of the terms that cancel in ds (softmax backward): |m dm| + m |<dm, m>|, carried through the same products
    dsa = m64 * dm.abs() + m64 * (dm * m64).sum(-1, keepdim=True).abs()
    sq = dsa @ e64.detach().abs()
    se = dsa.transpose(-2, -1) @ q64.detach().abs()
    for a in (add0, add1):
        if a is not None:
            de = de + a.to(F64)
            se = se + a.to(F64).abs()
    return dq, de, sq, se


ATTN_VARIANTS = [(True, True, "none"), (False, True, "peaked"), (True, False, "none"), (False, False, "none")]


@pytest.mark.parametrize("N,S,branch", SHAPES, ids=[f"N{n}-S{s}" for n, s, _ in SHAPES])
def test_attention_backward(N, S, branch):
    t0 = time.time()
    L = _lib()
    lib = L.lib()
    worst = {}
    st = torch.cuda.current_stream().cuda_stream
    variants = ATTN_VARIANTS if S * N <= 40000 else ATTN_VARIANTS[:2]
    for vi, (has0, has1, edge) in enumerate(variants):
        case = f"attn N={N} S={S} v{vi} [{branch}]"
        g = torch.Generator().manual_seed(2000 * N + S + vi)
        q, e = _attention_inputs(g, S, N, edge == "peaked")
        m = torch.softmax(q.to(F64) @ e.to(F64).transpose(-2, -1), dim=-1).float()
        if edge == "peaked":
            assert float(m.amax(-1).mean()) > 0.8
        d_m = torch.randn(S, N, N, generator=g)
        add0 = torch.randn(S, N, 64, generator=g) * 0.3 if has0 else None
        add1 = torch.randn(S, N, 64, generator=g) * 0.3 if has1 else None
        cuda = lambda t: None if t is None else t.to(DEV).contiguous()       # noqa: E731
        q, e, m, d_m, add0, add1 = map(cuda, (q, e, m, d_m, add0, add1))
        dq, de = _nan(S, N, 64), _nan(S, N, 64)
        L.check(lib.cm_attention_backward(S, N, 64, _p(q), _p(e), _p(m), _p(d_m), _p(add0), _p(add1), _p(dq), _p(de), st),
                "cm_attention_backward")
        torch.cuda.synchronize()
        rq, re, sq, se = _attn_ref(q, e, m, d_m, add0, add1)
        # rows: the softmax backward cancels (header); peaked rows (one score far above the rest) cancel the whole tensor
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
    _record(f"attn N={N} S={S} ({time.time() - t0:.1f}s)", worst)


def test_attention_backward_refuses_aliasing():
    L = _lib()
    lib = L.lib()
    t = torch.zeros(2, 4, 64, device=DEV)
    m = torch.zeros(2, 4, 4, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.cm_attention_backward(2, 4, 64, _p(t), _p(t), _p(m), _p(m), _p(t), None, _p(t.clone()), _p(t), st) != 0


# ------------------------------------------------------------------------------------------------------------------
# encoder backward
# ------------------------------------------------------------------------------------------------------------------
def _enc_ref(obs, a1, e, w2, dy, dy2):
    """obs -> a1 = tanh(W1 obs + b1) -> e = tanh(W2 a1 + b2) (f64_commnet.encoder), backward from the saved a1 / e."""
    o, a, y, w = (t.to(F64) for t in (obs, a1, e, w2))
    dz2 = dy.to(F64) + (dy2.to(F64) if dy2 is not None else 0)
    dz2 = dz2 * (1 - y ** 2)
    dz1 = (dz2 @ w) * (1 - a ** 2)
    return dz2.T @ a, dz2.sum(0), dz1.T @ o, dz1.sum(0)


ENC_SHAPES = [
    # R (agent rows), d, what
    (1, 21, "one row, d <= 32 instantiation (cm_linear_bwd.hip:571)"),
    (60, 53, "d 33..64 instantiation (cm_linear_bwd.hip:572)"),
    (32772, 64, "d = 64, 8193 envs of 4: ragged tail"),
    (280004, 21, "70001 envs of 4: looping grid"),
    (1024, 64, "saturated tanh rows"),
]


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("Rr,d,what", ENC_SHAPES, ids=[f"R{r}-d{d}" for r, d, _ in ENC_SHAPES])
def test_encoder_backward(Rr, d, what, det):
    t0 = time.time()
    L = _lib()
    lib = L.lib()
    worst = {}
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(Rr + d)
    sat = what.startswith("saturated")
    for use_dy2 in (True, False):
        case = f"enc R={Rr} d={d} {'det' if det else 'atomic'} dy2={use_dy2} [{what}]"
        obs = torch.rand(Rr, d, generator=g) * 2 - 1
        w1, b1 = torch.randn(128, d, generator=g) / d ** 0.5, torch.randn(128, generator=g) * 0.1
        w2, b2 = torch.randn(64, 128, generator=g) / (128 ** 0.5), torch.randn(64, generator=g) * 0.1
        if sat:                                                              # most pre-activations beyond +-5
            b2 = b2 + 6.0 * torch.sign(torch.randn(64, generator=g))
        a1 = torch.tanh(obs.to(F64) @ w1.to(F64).T + b1.to(F64)).float()
        e = torch.tanh(a1.to(F64) @ w2.to(F64).T + b2.to(F64)).float()
        if sat:
            assert float((e.abs() > 0.9999).float().mean()) > 0.2
        dy = torch.randn(Rr, 64, generator=g)
        dy2 = torch.randn(Rr, 64, generator=g) * 0.5 if use_dy2 else None
        cuda = lambda t: None if t is None else t.to(DEV).contiguous()       # noqa: E731
        obs, a1, e, w2, dy, dy2 = map(cuda, (obs, a1, e, w2, dy, dy2))
        dw2, db2, dw1, db1 = (torch.zeros(*s, device=DEV) for s in ((64, 128), (64,), (128, d), (128,)))
        if det:
            nb = lib.cm_encoder_backward_det_ws_bytes(Rr, d)
            rc = lib.cm_encoder_backward_det(Rr, d, _p(obs), _p(a1), _p(e), _p(w2), _p(dy), _p(dy2), _p(dw2), _p(db2), _p(dw1), _p(db1),
                                             _p(_slab(nb)), nb, st)
        else:
            rc = lib.cm_encoder_backward(Rr, d, _p(obs), _p(a1), _p(e), _p(w2), _p(dy), _p(dy2), _p(dw2), _p(db2), _p(dw1), _p(db1), st)
        L.check(rc, "cm_encoder_backward")
        torch.cuda.synchronize()
        ref = _enc_ref(obs, a1, e, w2, dy, dy2)
        for nm, got, r in zip(("dw2", "db2", "dw1", "db1"), (dw2, db2, dw1, db1), ref):
            _check(case, nm, got, r, worst, TAU)
        wref = _enc_ref(obs[:-1], a1[:-1], e[:-1], w2, dy[:-1], None if dy2 is None else dy2[:-1]) if Rr > 1 else \
            tuple(torch.zeros_like(r) for r in ref)
        _reject(case, "without the last row", [(g_, w_, {}) for g_, w_ in zip((dw2, db2, dw1, db1), wref)], TAU)
        if dy2 is not None:
            wref2 = _enc_ref(obs, a1, e, w2, dy, None)
            _reject(case, "missing dy2", [(dw2, wref2[0], {})], TAU)
    _record(f"enc R={Rr} d={d} {'det' if det else 'atomic'} ({time.time() - t0:.1f}s)", worst)


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("d", [65, 77])
def test_encoder_backward_declines_wide_observations(d, det):
    """d > 64 is not covered by the one-pass chain: rc = 1 and nothing written (the caller runs two cm_linear_act_backward)."""
    lib = _lib().lib()
    Rr = 64
    t = lambda *s: torch.zeros(*s, device=DEV)                              # noqa: E731
    obs, a1, e, w2, dy = t(Rr, d), t(Rr, 128), t(Rr, 64), t(64, 128), t(Rr, 64)
    outs = [_nan(64, 128), _nan(64), _nan(128, d), _nan(128)]
    st = torch.cuda.current_stream().cuda_stream
    if det:
        nb = lib.cm_encoder_backward_det_ws_bytes(Rr, d)
        rc = lib.cm_encoder_backward_det(Rr, d, _p(obs), _p(a1), _p(e), _p(w2), _p(dy), None, *map(_p, outs), _p(_slab(nb)), nb, st)
    else:
        rc = lib.cm_encoder_backward(Rr, d, _p(obs), _p(a1), _p(e), _p(w2), _p(dy), None, *map(_p, outs), st)
    torch.cuda.synchronize()
    assert rc == 1
    assert all(bool(torch.isnan(o).all()) for o in outs)
