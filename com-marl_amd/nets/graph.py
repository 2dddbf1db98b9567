"""The graph ops of the Comm-DP trunk under autograd: the attention softmax (``AttentionModule`` over ``_AttentionSoftmax``:
cm_attention_forward / _backward) and the adjacency-masked aggregation of a hop (``masked_aggregate`` over ``_MaskedAggregate``:
cm_masked_agg_forward / _backward, csrc/cm_graph_ops.hip), each one HIP kernel each way for E = 64 and, for other embedding widths,
their _any forms (csrc/cm_graph_any.hip); ``GraphConvolutionModule`` holds a hop's weight and bias.  ``graph_op_route`` /
``set_graph_op_route`` say and pin which path a width other than 64 takes; the table behind them (``_GRAPH_ROUTE``) lives here
with its only readers and writers.

Reference: com_marl/torch/modules/attention_module.py, graph_conv_module.py, comm_base_net.py:101-103.
"""
import math

import torch
from torch import nn

from .. import _lib as L
from .layers import HipLinear


MAX_KERNEL_AGENTS = 128      # team size up to which the N x N HIP kernels hold one env's matrix in LDS


class _NotCovered(Exception):
    """A *_any graph op answered 1: the planes of this (N, E) do not fit a workgroup's LDS - the framework path runs instead."""


# (N, E) -> "hip" | "framework" for embeddings other than 64: what the forward ops answered (asked once per shape), or what
# set_graph_op_route pinned
_GRAPH_ROUTE = {}


def graph_op_route(N, E):
    """Which path attention and masked aggregation take for a team of N and an embedding width E other than 64: "hip" (the
    cm_*_any kernels of csrc/cm_graph_any.hip, forward and backward) or "framework" (batched GEMMs, autograd's backward).
    Teams above MAX_KERNEL_AGENTS and widths outside 1..128 are "framework"; so is a shape whose planes the forward op found
    not to fit 160 KB of LDS (it answers 1 once, the answer is kept).  E = 64 has its own kernels and never asks."""
    if N > MAX_KERNEL_AGENTS or not 1 <= E <= 128:
        return "framework"
    return _GRAPH_ROUTE.get((N, E), "hip")


def set_graph_op_route(N, E, route):
    """Pin graph_op_route(N, E) to "hip" or "framework" (None: forget the pin) - for measurements and tests."""
    if route is None:
        _GRAPH_ROUTE.pop((N, E), None)
        return
    if route not in ("hip", "framework"):
        raise ValueError(f"route must be 'hip', 'framework' or None, not {route!r}")
    _GRAPH_ROUTE[(N, E)] = route


def _graph_forward(name, any_width, N, E, *args, device):
    """The forward of a graph op: `name` (E = 64), or `name`_any, whose answer 1 sends the shape to the framework path."""
    if not any_width:
        L.run(name, *args, device=device)
    elif not L.run(name + "_any", *args, device=device, maybe=True):
        _GRAPH_ROUTE[(N, E)] = "framework"
        raise _NotCovered(name + "_any")


def _hop_channels(chan_all, hop, N):
    """(pointer | None, per-sample stride in floats) of hop `hop`'s N x N planes in channels [S,L,N,N] (contiguous f32)."""
    if chan_all is None:
        return None, 0
    return chan_all.data_ptr() + 4 * hop * N * N, chan_all.shape[1] * N * N


class _AttentionSoftmax(torch.autograd.Function):
    """M = softmax_j(q_i . e_j) per sample, one HIP kernel each way instead of three batched N x N GEMMs: cm_attention_forward /
    _backward for E = 64, with `any_width` their _any forms (widths 1..128; _NotCovered where the forward answers 1)."""

    @staticmethod
    def forward(ctx, q, e, any_width=False):
        S, N, E = e.shape
        q, e = q.contiguous(), e.contiguous()
        m = torch.empty(S, N, N, dtype=e.dtype, device=e.device)
        _graph_forward("cm_attention_forward", any_width, N, E, S, N, E, L.ptr(q), L.ptr(e), L.ptr(m), device=e.device)
        ctx.save_for_backward(q, e, m)
        ctx.any_width = any_width
        return m

    @staticmethod
    def backward(ctx, d_m):
        q, e, m = ctx.saved_tensors
        S, N, E = e.shape
        d_m = d_m.contiguous()
        d_q, d_e = torch.empty_like(q), torch.empty_like(e)
        L.run("cm_attention_backward_any" if ctx.any_width else "cm_attention_backward", S, N, E, L.ptr(q), L.ptr(e), L.ptr(m),
              L.ptr(d_m), None, None, L.ptr(d_q), L.ptr(d_e), device=e.device)
        return d_q, d_e, None


class AttentionModule(nn.Module):
    """attention_module.py:17-51: 'general' softmax_j((q W^T) . k_j) with the learned ``linear_in``, or 'dot'
    softmax_j(q . k_j) with no parameter at all (:38-41).  ('diff' creates a parameter in the reference's constructor but its
    forward has no branch for it - it cannot run there either.)"""

    def __init__(self, dimensions, attention_type="general"):
        super().__init__()
        if attention_type not in ("general", "dot"):
            raise NotImplementedError("attention_type must be 'general' or 'dot' ('diff' has no forward branch in the reference, "
                                      "attention_module.py:36-49)")
        self.attention_type = attention_type
        if attention_type == "general":
            self.linear_in = HipLinear(dimensions, dimensions, bias=False)
        self._dim = dimensions

    def forward(self, query):
        q = self.linear_in(query) if self.attention_type == "general" else query
        if query.is_cuda and query.dim() == 3 and query.shape[-1] == 64 and query.shape[-2] <= MAX_KERNEL_AGENTS:
            return _AttentionSoftmax.apply(q, query)             # fused HIP op (cm_attention_forward/backward)
        if (query.is_cuda and query.dim() == 3 and query.dtype == torch.float32
                and graph_op_route(query.shape[-2], query.shape[-1]) == "hip"):
            try:
                return _AttentionSoftmax.apply(q, query, True)   # embeddings other than 64 (--embedding_dim): cm_attention_*_any
            except _NotCovered:
                pass
        # teams above 128 agents (maps >= 50), and widths whose planes do not fit the LDS: library GEMMs, autograd backward
        return torch.softmax(torch.matmul(q, query.transpose(-2, -1)), dim=-1)


class GraphConvolutionModule(nn.Module):
    """graph_conv_module.py:24-72: weight [in,out] ~ U(+-1/sqrt(out)), bias likewise."""

    def __init__(self, in_features, out_features, bias=True, id=None):
        super().__init__()
        self.in_features, self.out_features, self.id = in_features, out_features, id
        self.weight = nn.Parameter(torch.empty(in_features, out_features))
        self.bias = nn.Parameter(torch.empty(out_features)) if bias else None
        stdv = 1.0 / math.sqrt(out_features)
        with torch.no_grad():
            self.weight.uniform_(-stdv, stdv)
            if self.bias is not None:
                self.bias.uniform_(-stdv, stdv)


class _MaskedAggregate(torch.autograd.Function):
    """out = tanh(A.(HW) + b), A = M*R*C row-renormalised (comm_base_net.py:101-103, graph_conv_module.py:63-70) as one HIP
    kernel each way: cm_masked_agg_forward / _backward for E = 64, with `any_width` their _any forms (widths 1..128;
    _NotCovered where the forward answers 1).  Either backward has its _det twin."""

    @staticmethod
    def forward(ctx, attn, dist_adj, chan_all, hop, hw, bias, any_width=False):
        S, N, E = hw.shape
        attn, hw = attn.contiguous(), hw.contiguous()
        out = torch.empty_like(hw)
        _graph_forward("cm_masked_agg_forward", any_width, N, E, S, N, E, L.ptr(attn), L.ptr(dist_adj),
                       *_hop_channels(chan_all, hop, N), L.ptr(hw), L.ptr(bias), L.ptr(out), device=hw.device)
        ctx.save_for_backward(attn, dist_adj, chan_all, hw, out)
        ctx.hop, ctx.has_bias, ctx.any_width = hop, bias is not None, any_width
        return out

    @staticmethod
    def backward(ctx, d_out):
        attn, dist_adj, chan_all, hw, out = ctx.saved_tensors
        S, N, E = hw.shape
        d_out = d_out.contiguous()
        d_attn, d_hw = torch.empty_like(attn), torch.empty_like(hw)
        d_bias = torch.zeros(E, dtype=hw.dtype, device=hw.device) if ctx.has_bias else None
        L.launch("cm_masked_agg_backward_any" if ctx.any_width else "cm_masked_agg_backward",
                 (S, N, E, L.ptr(attn), L.ptr(dist_adj), *_hop_channels(chan_all, ctx.hop, N), L.ptr(hw), L.ptr(out), None,
                  L.ptr(d_out), L.ptr(d_attn), L.ptr(d_hw), L.ptr(d_bias)), (S, N, E), device=hw.device)
        return d_attn, None, None, None, d_hw, d_bias, None


def masked_aggregate(attn, dist_adj, channels, hop, hw, bias):
    """attn [S,N,N], dist_adj [S,N,N] or None (= ones), channels [S,L,N,N] or None, hw [S,N,E]."""
    if not hw.is_cuda:
        raise L.CommarlError("masked_aggregate is a HIP op: tensors must live on the MI355X (no CPU fallback)")
    if (hw.shape[2] != 64 and hw.dim() == 3 and hw.dtype == torch.float32 and attn.dtype == torch.float32
            and graph_op_route(hw.shape[1], hw.shape[2]) == "hip"):
        try:                                     # embeddings other than 64 (--embedding_dim): cm_masked_agg_*_any
            return _MaskedAggregate.apply(attn, dist_adj if dist_adj is None else dist_adj.contiguous(),
                                          channels if channels is None else channels.contiguous(), hop, hw, bias, True)
        except _NotCovered:
            pass
    if hw.shape[1] > MAX_KERNEL_AGENTS or hw.shape[2] != 64:
        # teams above 128 agents (PP map 50: N = 200), and widths other than 64 whose planes do not fit: the N x N tile of one env
        # no longer fits a workgroup's LDS - the same arithmetic (comm_base_net.py:101-103, graph_conv_module.py:63-70) on the
        # framework's batched GEMM, still on the GPU, autograd doing the backward
        A = attn
        if dist_adj is not None:
            A = A * dist_adj
        if channels is not None:
            A = A * channels[:, hop]
        A = A / (A.sum(dim=-1, keepdim=True) + 1e-12)
        out = torch.matmul(A, hw)
        return torch.tanh(out + bias if bias is not None else out)
    return _MaskedAggregate.apply(attn, dist_adj, channels, hop, hw, bias)
