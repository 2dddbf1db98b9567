"""Comm-DP policy and critic: same classes, ctor kwargs, parameter names and numerics as the
reference, two execution paths:

  * rollout / no-grad : ONE fused HIP launch per batch of env states through the C ABI
    (``cm_policy_forward`` / ``cm_critic_forward``, csrc/cm_policy.hip);
  * PPO update (autograd): dense per-agent GEMMs on PyTorch-ROCm (rocBLAS / MFMA), the
    adjacency-masked aggregation as the custom HIP op ``masked_aggregate``
    (``cm_masked_agg_forward/backward``, csrc/cm_graph_ops.hip).

Reference: com_marl/torch/modules/comm_base_net.py, attention_module.py, graph_conv_module.py,
mlp_encoder_module.py, categorical_mlp_module.py, gaussian_mlp_module.py,
policies/comm_categorical_mlp_policy.py, baselines/comm_base_critic.py,
garage/torch/modules/multi_headed_mlp_module.py.
"""
import ctypes as C
import math
import os
from collections import OrderedDict

import numpy as np
import torch
from torch import nn
from torch.distributions import Categorical, Normal

from . import _lib as L
from . import deterministic as _det


MAX_KERNEL_AGENTS = 128      # team size up to which the N x N HIP kernels hold one env's matrix in LDS
MAX_FUSED_AGENTS = 80        # ... and up to which the one-launch forward (rollout and training) does (cm_policy_h_dev.h LDS map)
MAX_FUSED_OBS = 80           # per-agent observation size up to which the matrix-core pack, hence the training forward, exists

# ---------------------------------------------------------------------------------------------
# building blocks with the reference's state_dict names
# ---------------------------------------------------------------------------------------------
class _Tanh(nn.Module):
    def forward(self, x):
        return torch.tanh(x)


class _ReLU(nn.Module):
    def forward(self, x):
        return torch.relu(x)


ACT_NONE, ACT_TANH, ACT_RELU = 0, 1, 2       # activation codes of cm_linear_act_* (include/commarl.h)


def hidden_act_code(hidden_nonlinearity):
    """The reference runners' ``hidden_nonlinearity`` (F.relu if --hidden_nonlinearity relu else torch.tanh,
    exp_runners/*/runner_*_{obsDP,cent}.py) -> ACT_TANH / ACT_RELU.  Anything else raises: there is no silent fallback."""
    f = hidden_nonlinearity
    if f is torch.tanh or f is torch.nn.functional.tanh or isinstance(f, nn.Tanh):
        return ACT_TANH
    if f is torch.relu or f is torch.nn.functional.relu or isinstance(f, nn.ReLU):
        return ACT_RELU
    raise NotImplementedError(f"hidden_nonlinearity={f!r} is not supported: use torch.tanh, torch.relu, F.tanh, F.relu, "
                              "nn.Tanh() or nn.ReLU()")


class MLPModule(nn.Module):
    """garage MultiHeadedMLPModule with one head (multi_headed_mlp_module.py:54-149):
    ``_layers.{i}.linear`` (+ hidden activation: ``hidden_act`` 1 = tanh, 2 = ReLU) then ``_output_layers.0.linear``
    (+ optional tanh).  Init order mirrors the reference: nn.Linear default init, then xavier_uniform_ / zeros_."""

    def __init__(self, input_dim, output_dim, hidden_sizes, output_tanh=False, hidden_act=ACT_TANH):
        super().__init__()
        if hidden_act not in (ACT_TANH, ACT_RELU):
            raise NotImplementedError(f"hidden_act must be {ACT_TANH} (tanh) or {ACT_RELU} (ReLU)")
        self._hidden_act = hidden_act
        self._layers = nn.ModuleList()
        prev = input_dim
        for size in hidden_sizes:
            lin = HipLinear(prev, size)
            nn.init.xavier_uniform_(lin.weight)
            nn.init.zeros_(lin.bias)
            act = _Tanh() if hidden_act == ACT_TANH else _ReLU()
            self._layers.append(nn.Sequential(OrderedDict(linear=lin, non_linearity=act)))
            prev = size
        lin = HipLinear(prev, output_dim)
        nn.init.xavier_uniform_(lin.weight)
        nn.init.zeros_(lin.bias)
        mods = OrderedDict(linear=lin)
        if output_tanh:
            mods["non_linearity"] = _Tanh()
        self._output_layers = nn.ModuleList([nn.Sequential(mods)])

    def forward(self, x):
        for layer in self._layers:
            x = hip_linear(x, layer.linear, act=self._hidden_act)         # Sequential(linear, activation) as one fused op
        out = self._output_layers[0]
        return hip_linear(x, out.linear, act=1 if len(out) > 1 else 0)


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


def _wgrad(a2d, b2d, want_colsum):
    """c[p][q] = sum_r a[r][p] b[r][q] (+ column sums of a) on the MFMA weight-gradient kernel."""
    R, P = a2d.shape
    Q = b2d.shape[1]
    c = torch.zeros(P, Q, dtype=torch.float32, device=a2d.device)
    cs = torch.zeros(P, dtype=torch.float32, device=a2d.device) if want_colsum else None
    L.launch("cm_linear_wgrad", (R, P, Q, L.ptr(a2d), L.ptr(b2d), L.ptr(c), L.ptr(cs)), (R, P, Q), device=a2d.device)
    return c, cs


def _linear_act_backward(R, K, O, x2, w, layout, dy2, dy_add, y, dx, dw, db, act=None):
    """cm_linear_act_backward (y given = tanh layer), or with ``act`` (0 / 1 / 2) cm_linear_act_backward_ex (their slab twins
    in deterministic mode), on w's device."""
    name = "cm_linear_act_backward" if act is None else "cm_linear_act_backward_ex"
    args = (R, K, O, L.ptr(x2), L.ptr(w), layout, L.ptr(dy2), L.ptr(dy_add), L.ptr(y)) + (() if act is None else (int(act),))
    L.launch(name, args + (L.ptr(dx), L.ptr(dw), L.ptr(db)), (R, K, O), device=w.device)


class _LinearFn(torch.autograd.Function):
    """y = x W^T + b with the weight / bias gradients on cm_linear_wgrad: over ~1e6 agent rows the library
    GEMM for dW = dY^T X (tiny output, million-deep reduction) ran at ~10 TFLOP/s and dominated the update."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return torch.nn.functional.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dx = dy.matmul(weight) if ctx.needs_input_grad[0] else None
        dy2 = dy.reshape(-1, dy.shape[-1]).contiguous()
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        dw, db = _wgrad(dy2, x2, ctx.has_bias)
        return dx, dw, db


class _MatmulWFn(torch.autograd.Function):
    """z = h W (GraphConvolutionModule, weight [in,out]) with dW on cm_linear_wgrad."""

    @staticmethod
    def forward(ctx, h, weight):
        ctx.save_for_backward(h, weight)
        return torch.matmul(h, weight)

    @staticmethod
    def backward(ctx, dz):
        h, weight = ctx.saved_tensors
        dh = dz.matmul(weight.t()) if ctx.needs_input_grad[0] else None
        dw, _ = _wgrad(h.reshape(-1, h.shape[-1]).contiguous(), dz.reshape(-1, dz.shape[-1]).contiguous(), False)
        return dh, dw


class _LinearActFn(torch.autograd.Function):
    """y = act(x W^T + b) (layout 0, nn.Linear) or act(x W) (layout 1, GraphConvolution weight) as ONE kernel each way
    (csrc/cm_linear.hip): forward reads x and writes y; backward reads dy, y, x and writes dx while the weight and
    bias gradients accumulate in registers - instead of torch's GEMM, tanh, tanh', input-gradient GEMM and
    weight-gradient GEMM, each a full HBM pass over the [rows, 64..128] activations of ~1e6 agent rows."""

    @staticmethod
    def forward(ctx, x, weight, bias, act, layout):
        K = x.shape[-1]
        O = weight.shape[0] if layout == 0 else weight.shape[1]
        x2 = x.reshape(-1, K).contiguous()
        w = weight.contiguous()
        y = torch.empty(x2.shape[0], O, dtype=torch.float32, device=x.device)
        L.run("cm_linear_act_forward", x2.shape[0], K, O, L.ptr(x2), L.ptr(w), layout, L.cptr(bias), int(act), L.ptr(y),
              device=x.device)
        ctx.save_for_backward(x2, w, y if act else None)
        ctx.meta = (tuple(x.shape), K, O, int(act), layout, bias is not None)
        return y.reshape(*x.shape[:-1], O)

    @staticmethod
    def backward(ctx, dy):
        x2, w, y = ctx.saved_tensors
        shape, K, O, act, layout, has_bias = ctx.meta
        dy2 = dy.reshape(-1, O).contiguous()
        dx = torch.empty_like(x2) if ctx.needs_input_grad[0] else None
        dw = torch.zeros_like(w)
        db = torch.zeros(O, dtype=torch.float32, device=w.device) if has_bias else None
        # ReLU names its activation (cm_linear_act_backward_ex); tanh / identity keep the entry points they always used
        _linear_act_backward(x2.shape[0], K, O, x2, w, layout, dy2, None, y, dx, dw, db, act=act if act == ACT_RELU else None)
        return (None if dx is None else dx.reshape(shape)), dw, db, None, None


def _fused_ok(x, weight):
    return (x.is_cuda and x.dtype == torch.float32 and torch.is_grad_enabled() and weight.requires_grad
            and max(weight.shape) <= 128)


def hip_linear(x, lin, act=ACT_NONE):
    """nn.Linear followed by act (0 none, 1 tanh, 2 ReLU); on the GPU with autograd on it is the fused one-pass kernel pair."""
    if _fused_ok(x, lin.weight):
        return _LinearActFn.apply(x, lin.weight, lin.bias, act, 0)
    if x.is_cuda and torch.is_grad_enabled() and lin.weight.requires_grad and max(lin.weight.shape) <= 128:
        y = _LinearFn.apply(x, lin.weight, lin.bias)
    else:
        y = torch.nn.functional.linear(x, lin.weight, lin.bias)
    if act == ACT_RELU:
        return torch.relu(y)
    return torch.tanh(y) if act else y


class HipLinear(nn.Linear):
    """nn.Linear (same parameters / state_dict) whose training backward runs on cm_linear_wgrad."""

    def forward(self, x):
        return hip_linear(x, self)


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


# ---------------------------------------------------------------------------------------------
# whole-network training forward (every team size <= 128): ONE fused launch that stores what the backward needs, and a hand-written
# backward chain over the C-ABI kernels - no per-layer forward kernels, no gradient-accumulation adds from autograd
# ---------------------------------------------------------------------------------------------
class _ZeroPool:
    """The weight / bias gradients of one backward pass as views of ONE zero-filled buffer (one fill launch instead of one per
    tensor; the kernels accumulate into them with float atomics, so they must start at zero).  Views are 16-byte aligned."""

    def __init__(self, params, device, extra=0):
        total = sum((p.numel() + 3) & ~3 for p in params) + extra
        self.buf = torch.zeros(total, dtype=torch.float32, device=device)
        self.off = 0

    def take(self, shape):
        n = 1
        for d in shape:
            n *= int(d)
        if self.off + n > self.buf.numel():                        # (not reached: sized from the net's parameter list)
            return torch.zeros(*shape, dtype=torch.float32, device=self.buf.device)
        v = self.buf[self.off:self.off + n].view(*shape)
        self.off += (n + 3) & ~3
        return v


def _lin_bwd(x2, w, layout, dy2, y2, want_dx, has_bias, dy_add=None, pool=None):
    """cm_linear_act_backward on 2-D contiguous tensors -> (dx | None, dw, db | None); dy_add: a second gradient into the
    layer's output, summed inside the kernel; pool: a _ZeroPool the weight / bias gradients are taken from."""
    R, K = x2.shape
    O = dy2.shape[1]
    dx = torch.empty_like(x2) if want_dx else None
    dw = pool.take(w.shape) if pool is not None else torch.zeros_like(w)
    db = (pool.take((O,)) if pool is not None else torch.zeros(O, dtype=torch.float32, device=w.device)) if has_bias else None
    _linear_act_backward(R, K, O, x2, w, layout, dy2, dy_add, y2, dx, dw, db)
    return dx, dw, db


def _fused_shape_ok(net, obs):
    """Shapes with a saved-forward instantiation (cm_*_forward_saved) and a backward chain."""
    # teams above 80 agents exceed the f16-split forward's LDS budget (its activation planes + the N x N score matrix):
    # they keep the per-layer path.  Observations above 80 features have no matrix-core operand pack (kpad_of,
    # cm_policy_mfma_dev.h: cm_*_pack_bytes() == 0), without which the saved forward launches nothing
    return (obs.is_cuda and 1 <= net._n_agents <= MAX_FUSED_AGENTS and 1 <= len(net.gcn_layers) <= 4
            and net._dec_obs_dim <= MAX_FUSED_OBS and len(net.encoder._layers) == 1 and net._default_shape
            and os.environ.get("COMMARL_FUSED_TRAIN", "1") != "0" and os.environ.get("COMMARL_POLICY_KERNEL", "")[:1] not in ("f", "v"))


def _fused_train_ok(net, obs):
    return torch.is_grad_enabled() and _fused_shape_ok(net, obs)


def _fwd_wave_ok(N, S):
    """Teams of 4, large batches: the wave-owned kernel of the rollout as training forward (cm_*_forward_saved_wave: a
    persistent workgroup per CU, activations in registers: 0.97 -> 0.5 ms at 1.1 M agent rows).  Small (launch-bound)
    batches keep the f16-split kernel.  Decided on every call."""
    return (N == 4 and S >= int(os.environ.get("COMMARL_TRAIN_FWD_WAVE_MIN", "16384"))
            and (os.environ.get("COMMARL_POLICY_KERNEL") or "w")[0] not in "hfv")


def _forward_saved(name, wave, *args, device):
    """`name` (cm_policy_forward_saved / cm_critic_forward_saved) on the current stream, preceded by its _wave form when
    `wave`: the wave kernel's return of 1 (shape not covered) falls back to `name`, whose return of 1 raises."""
    if wave and L.run(name + "_wave", *args, device=device, maybe=True):
        return
    if not L.run(name, *args, device=device, maybe=True):
        raise L.CommarlError(f"{name}: no saved-forward instantiation for this shape (callers check _fused_shape_ok)")


class _FusedNetFn(torch.autograd.Function):
    """CommBaseNet trunk + head as ONE forward launch (cm_policy_forward_saved / cm_critic_forward_saved: the rollout
    kernel with stores of every activation the backward needs) and a hand-written backward chain:
    head layers <- residual <- L x (masked aggregation <- H.Wg) <- attention softmax <- linear_in <- encoder, each link one
    C-ABI kernel (cm_linear_act_backward, cm_masked_agg_backward, cm_attention_backward).  Returns logits [S,N,A]
    (policy) or per-agent values [S,N] (critic); the attention matrix comes back as a non-differentiable second output
    (the reference detaches nothing here, but no loss term reads it)."""

    @staticmethod
    def forward(ctx, net, obs, adj, ch, *params):
        N, Lh, d = net._n_agents, len(net.gcn_layers), net._dec_obs_dim
        S = obs.shape[0]
        R = S * N
        dev = obs.device
        policy = net._is_policy
        z = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)   # noqa: E731
        obs2 = obs.reshape(R, d).contiguous()
        t = dict(a1=z(R, 128), e=z(R, 64), q=z(R, 64), hw=[z(R, 64) for _ in range(Lh)], h=[z(R, 64) for _ in range(Lh)])
        if policy:
            A = net._action_dim
            t.update(x1=z(R, 128), x2=z(R, 64), x3=z(R, 32), out=z(R, A))
        else:
            t.update(x1=z(R, 64), out=z(R))
        attn = z(S, N, N)
        sv = L.FwdSaves()
        sv.a1, sv.e, sv.q, sv.x1, sv.out = (t[k].data_ptr() for k in ("a1", "e", "q", "x1", "out"))
        if policy:
            sv.x2, sv.x3 = t["x2"].data_ptr(), t["x3"].data_ptr()
        for l in range(Lh):
            sv.hw[l], sv.h[l] = t["hw"][l].data_ptr(), t["h"][l].data_ptr()
        adj_c = None if adj is None else adj.contiguous()
        ch_c = None if ch is None else ch.contiguous()
        net._train_fwd = True                          # the weight pack refreshes the f16-split section only (_WeightPack._packed)
        # ... and the CM_PACK_WAVE section with it when the wave-owned kernel runs (its fragments)
        wave = net._train_fwd_wave = _fwd_wave_ok(N, S)
        vals = () if policy else (z(S),)               # the critic's entry point also writes the summed values
        try:
            w = net._weights_struct()
            _forward_saved("cm_policy_forward_saved" if policy else "cm_critic_forward_saved", wave, C.byref(w), S, L.ptr(obs2),
                           L.ptr(adj_c), L.ptr(ch_c), L.ptr(attn), *map(L.ptr, vals), C.byref(sv), device=dev)
        finally:
            net._train_fwd = net._train_fwd_wave = False
        ctx.net, ctx.t, ctx.obs2, ctx.adj, ctx.ch, ctx.attn, ctx.policy = net, t, obs2, adj_c, ch_c, attn, policy
        ctx.names = [n for n, _ in net.named_parameters()]
        ctx.mark_non_differentiable(attn)
        out = t["out"].view(S, N, -1) if policy else t["out"].view(S, N)
        return out, attn

    @staticmethod
    def backward(ctx, d_out, _d_attn):
        net, t, obs2, adj, ch, attn = ctx.net, ctx.t, ctx.obs2, ctx.adj, ctx.ch, ctx.attn
        N, Lh = net._n_agents, len(net.gcn_layers)
        R = obs2.shape[0]
        S = R // N
        P = dict(net.named_parameters())
        g = {}
        pool = _ZeroPool(list(P.values()), obs2.device, extra=31 * 64 * len(net.gcn_layers))   # (+ the bias-gradient replicas below)
        det = _det()
        if ctx.policy:
            hd = net.categorical_output_layer
            lins = [l.linear for l in hd._layers] + [hd._output_layers[0].linear]
            pre = ["categorical_output_layer._layers.%d.linear" % i for i in range(3)] + ["categorical_output_layer._output_layers.0.linear"]
            acts = [t["h"][Lh - 1], t["x1"], t["x2"], t["x3"]]          # inputs of the four head layers
            d = d_out.reshape(R, -1).contiguous()
            for i in (3, 2, 1, 0):                                       # y of layer i = input of layer i + 1 (tanh), none for the logits
                d, g[pre[i] + ".weight"], g[pre[i] + ".bias"] = _lin_bwd(acts[i], lins[i].weight, 0, d, None if i == 3 else acts[i + 1],
                                                                          True, True, pool=pool)
        else:
            mm = net.baseline_aggregator._mean_module
            l1, l2 = mm._layers[0].linear, mm._output_layers[0].linear
            pre = "baseline_aggregator._mean_module."
            d = d_out.reshape(R, 1).contiguous()
            d, g[pre + "_output_layers.0.linear.weight"], g[pre + "_output_layers.0.linear.bias"] = _lin_bwd(t["x1"], l2.weight, 0, d, None, True, True, pool=pool)
            d, g[pre + "_layers.0.linear.weight"], g[pre + "_layers.0.linear.bias"] = _lin_bwd(t["h"][Lh - 1], l1.weight, 0, d, t["x1"], True, True, pool=pool)
        # d = gradient wrt the trunk output x = E + H_L (or H_L)
        e, q = t["e"], t["q"]
        d_res = d if net.residual else None                              # residual: the same gradient flows into E
        dH, d_attn, dhin0 = d, None, None
        for l in reversed(range(Lh)):
            gl = net.gcn_layers[l]
            minus = e if (l == Lh - 1 and net.residual) else None       # saved x = E + H_L: the hop's tanh output is x - E
            da, dhw = torch.empty_like(attn), torch.empty_like(e)
            # large batches of teams of 4: the bias gradient over 32 rows summed afterwards (cm_masked_agg_backward_r)
            reps = 32 if (N == 4 and S > 16 * 512 and not det) else 1
            dgb = pool.take((reps, 64)) if gl.bias is not None else None
            # (deterministic mode: one bias row, merged in a fixed order)
            L.launch("cm_masked_agg_backward_r", (S, N, 64, L.ptr(attn), L.ptr(adj), *_hop_channels(ch, l, N), L.ptr(t["hw"][l]),
                                                  L.ptr(t["h"][l]), L.ptr(minus), L.ptr(dH), L.ptr(da), L.ptr(dhw), L.ptr(dgb), reps),
                     (S, N, 64), device=obs2.device)
            if dgb is not None:
                dgb = dgb.sum(0) if reps > 1 else dgb[0]
            d_attn = da if d_attn is None else d_attn.add_(da)
            hin = t["h"][l - 1] if l > 0 else e
            dhin, g["gcn_layers.%d.weight" % l], _ = _lin_bwd(hin, gl.weight, 1, dhw, None, True, False, pool=pool)
            if gl.bias is not None:
                g["gcn_layers.%d.bias" % l] = dgb
            if l > 0:
                dH = dhin
            else:
                dhin0 = dhin
        # gradient wrt E = residual term + hop 0's input gradient + attention key side (summed by the attention kernel)
        # + linear_in's input gradient (summed by the encoder layer's backward): no accumulation passes
        if Lh == 0:
            raise L.CommarlError("fused training path needs at least one hop")
        dq, dE = torch.empty_like(q), torch.empty_like(e)
        L.run("cm_attention_backward", S, N, 64, L.ptr(q), L.ptr(e), L.ptr(attn), L.ptr(d_attn), L.ptr(d_res), L.ptr(dhin0),
              L.ptr(dq), L.ptr(dE), device=obs2.device)
        if net.attention_layer.attention_type == "general":
            deq, g["attention_layer.linear_in.weight"], _ = _lin_bwd(e, net.attention_layer.linear_in.weight, 0, dq, None, True, False, pool=pool)
        else:
            deq = dq                                                     # 'dot': Q is E itself
        enc1, enc2 = net.encoder._layers[0].linear, net.encoder._output_layers[0].linear
        # both encoder layers in one pass (the gradient wrt the hidden layer never leaves the workgroup); wide observations
        # (d > 64) take the two layers one by one
        dw2, db2 = pool.take(enc2.weight.shape), pool.take(enc2.bias.shape)
        dw1, db1 = pool.take(enc1.weight.shape), pool.take(enc1.bias.shape)
        if not L.launch("cm_encoder_backward", (R, obs2.shape[1], L.ptr(obs2), L.ptr(t["a1"]), L.ptr(e), L.ptr(enc2.weight), L.ptr(dE),
                                                L.ptr(deq), L.ptr(dw2), L.ptr(db2), L.ptr(dw1), L.ptr(db1)), (R, obs2.shape[1]),
                        device=obs2.device, maybe=True):
            da1, dw2, db2 = _lin_bwd(t["a1"], enc2.weight, 0, dE, e, True, True, dy_add=deq)     # (dw2 .. db1 taken above stay zero, unused)
            _, dw1, db1 = _lin_bwd(obs2, enc1.weight, 0, da1, t["a1"], False, True)
        g["encoder._output_layers.0.linear.weight"], g["encoder._output_layers.0.linear.bias"] = dw2, db2
        g["encoder._layers.0.linear.weight"], g["encoder._layers.0.linear.bias"] = dw1, db1
        ctx.t = None                                                     # free the saved activations
        return (None, None, None, None) + tuple(g.get(n) for n in ctx.names)


@torch.no_grad()
def _fused_logits_nograd(net, obs, adj, ch, want_probs=False):
    """Policy logits [S,N,A] + attention from the saved-forward kernel with every store but the logits (and, on
    request, the action probabilities) switched off: loss / KL evaluations over the full batch, no activations kept.
    -> (logits, attn) or, with want_probs, (logits, probs)."""
    N, d, A = net._n_agents, net._dec_obs_dim, net._action_dim
    S = obs.shape[0]
    obs2 = obs.reshape(S * N, d).contiguous()
    out = torch.empty(S * N, A, dtype=torch.float32, device=obs.device)
    attn = torch.empty(S, N, N, dtype=torch.float32, device=obs.device)
    sv = L.FwdSaves()
    sv.out = out.data_ptr()
    probs = torch.empty(S, N, A, dtype=torch.float32, device=obs.device) if want_probs else None
    if want_probs:
        sv.probs = probs.data_ptr()
    adj_c = None if adj is None else adj.contiguous()
    ch_c = None if ch is None else ch.contiguous()
    w = net._weights_struct()                                # (no-grad user: every section of the pack is current)
    # large batches of teams of 4: the same kernel the training forward takes (both sides of the PPO ratio from one arithmetic)
    _forward_saved("cm_policy_forward_saved", _fwd_wave_ok(N, S), C.byref(w), S, L.ptr(obs2), L.ptr(adj_c), L.ptr(ch_c),
                   L.ptr(attn), C.byref(sv), device=obs.device)
    return (out.view(S, N, A), probs) if want_probs else (out.view(S, N, A), attn)


# ---------------------------------------------------------------------------------------------
# trunk
# ---------------------------------------------------------------------------------------------
def _as_dev(x, device):
    if x is None:
        return None
    if not torch.is_tensor(x):
        x = torch.as_tensor(np.asarray(x), dtype=torch.float32)
    return x.to(device=device, dtype=torch.float32)


class _Stacked(list):
    """Equal-shape parameters that the flat weight copy stores back to back (what torch.stack would give, without its launch)."""

    def numel(self):
        return sum(t.numel() for t in self)


class _WeightPack:
    """Flat device copy of a net's (transposed) weights for the fused C-ABI kernels; subclasses list the
    tensors in ``_pack_tensors()``."""
    _pack_sig, _pack, _pack_stale, _train_fwd, _train_fwd_wave, _pack_fresh = None, None, False, False, False, 0

    def _pack_tensors(self):
        raise NotImplementedError

    def _packed(self):
        """Flat contiguous device copy of the (transposed) weights.  Allocated once; when a parameter
        changed (optimizer step / load_state_dict) the SAME buffer is rewritten in place, so device
        pointers - and any hipGraph that captured them - stay valid."""
        sig = tuple((p.data_ptr(), p._version) for p in self.parameters())
        # a training forward (_FusedNetFn sets _train_fwd around its launch) reads the f16-split fragments only: between two optimiser steps just that section is
        # refreshed (cm_*_pack_sections); the rest goes stale and is packed - with the range check - by the next no-grad user
        # (sync_weights() before a rollout, evaluate_nograd, act_device)
        need = (L.PACK_F16 | (L.PACK_WAVE if self._train_fwd_wave else 0)) if self._train_fwd else L.PACK_ALL
        if sig == self._pack_sig and not (need & 7 & ~self._pack_fresh):     # every section this user reads is current
            return self._pack[1]
        with torch.no_grad():
            ts = self._pack_tensors()
            if self._pack is None or self._pack[0].device != next(self.parameters()).device:
                offs, off = {}, 0
                for k, v in ts.items():
                    if v is None:
                        offs[k] = None
                        continue
                    offs[k] = (off, v.numel())
                    off += (v.numel() + 3) & ~3                 # keep every tensor 16-byte aligned
                buf = torch.zeros(off, dtype=torch.float32, device=next(self.parameters()).device)
                base = buf.data_ptr()
                ptrs = {k: (None if o is None else base + 4 * o[0]) for k, o in offs.items()}
                self._pack = (buf, ptrs, offs)
            buf, ptrs, offs = self._pack
            self._flat_copy(ts, buf, offs)
            same = sig == self._pack_sig
            self._pack_sig = None                               # a refused pack (cm_*_pack: weight outside the f16 range) is retried
            self._after_pack(self._pack[1], need)
            self._pack_fresh = (need & 7) | (self._pack_fresh if same else 0)
            self._pack_sig, self._pack_stale = sig, self._pack_fresh != 7
        return self._pack[1]

    def _flat_copy(self, ts, buf, offs):
        """Every tensor of `ts` into its slot of the flat buffer.  On the GPU: ONE launch (cm_multi_copy_t) for all the plain
        parameters and transposed weight views (`weight.t()`: the source is the parameter itself, the kernel transposes; a
        _Stacked group entry by entry); anything else through the framework's copy."""
        plain = []
        for k, v in ts.items():
            if v is None:
                continue
            o, n = offs[k]
            if isinstance(v, _Stacked):                      # the stack's members one after the other
                parts, po = [], o
                for t in v:
                    parts.append((t, po, t.numel()))
                    po += t.numel()
            else:
                parts = [(v, o, n)]
            for v, o, n in parts:
                self._flat_copy_one(v, buf[o:o + n], n, plain, buf)
        if plain:
            m = len(plain)
            src = (C.c_void_p * m)(*[t[0] for t in plain])
            dstp = (C.c_void_p * m)(*[t[1] for t in plain])
            rows = (C.c_int32 * m)(*[t[2] for t in plain])
            cols = (C.c_int32 * m)(*[t[3] for t in plain])
            tr = (C.c_int32 * m)(*[t[4] for t in plain])
            L.run("cm_multi_copy_t", m, src, dstp, rows, cols, tr, device=buf.device)

    @staticmethod
    def _flat_copy_one(v, dst, n, plain, buf):
        base = v._base if (v.dim() == 2 and v._base is not None and not v.is_contiguous()) else None
        if (buf.is_cuda and v.dtype == torch.float32 and v.dim() <= 2 and len(plain) < 40
                and (v.is_contiguous() or (base is not None and base.is_contiguous() and base.dim() == 2
                                           and base.shape == v.shape[::-1] and v.data_ptr() == base.data_ptr()))):
            if v.is_contiguous():
                plain.append((v.data_ptr(), dst.data_ptr(), 1, n, 0))
            else:                                            # v = base.t(): dst[c][r] = base[r][c]
                plain.append((base.data_ptr(), dst.data_ptr(), base.shape[0], base.shape[1], 1))
        else:
            dst.copy_(v.detach().to(torch.float32).reshape(-1))

    def _after_pack(self, ptrs, sections=15):
        """Hook: derived device-side layouts (the matrix-core operand pack) are rebuilt here."""

    def sync_weights(self):
        """Refresh the fused kernels' weight pack (call after an optimizer step, outside graphs)."""
        self._packed()

    def grad_norm(self):
        return float(np.sqrt(np.sum([p.grad.norm(2).item() ** 2 for p in self.parameters() if p.grad is not None])))

    def reset(self, dones=None):
        return

    @property
    def recurrent(self):
        return False


class CommBaseNet(_WeightPack, nn.Module):
    """comm_base_net.py:11-111."""
    _graph_capturable_update = True      # algos._UpdateGraphs: forward, loss and backward of these nets wait for nothing on the host

    def __init__(self, env_spec, n_agents, encoder_hidden_sizes=(128,), embedding_dim=64, attention_type="general",
                 n_gcn_layers=2, gcn_bias=True, state_include_actions=False, name="comm_base", residual=True,
                 device="cpu"):
        super().__init__()
        self.residual, self.device, self._n_agents, self.name = residual, device, n_agents, name
        self.comm = True
        self.centralized = True
        self.step = 0
        self.eps = 1e-12
        self._cent_obs_dim = env_spec.observation_space.flat_dim
        self._dec_obs_dim = int(self._cent_obs_dim / n_agents)
        self._action_dim = env_spec.action_space.n
        self._embedding_dim = embedding_dim
        self.n_gcn_layers = n_gcn_layers
        if state_include_actions:
            self._dec_obs_dim += self._action_dim
        self.encoder = MLPModule(self._dec_obs_dim, embedding_dim, encoder_hidden_sizes, output_tanh=True)
        self.attention_layer = AttentionModule(embedding_dim, attention_type)
        self.gcn_layers = nn.ModuleList([GraphConvolutionModule(embedding_dim, embedding_dim, bias=gcn_bias, id=i)
                                         for i in range(n_gcn_layers)])
        self._enc_hidden = tuple(encoder_hidden_sizes)

    # -- helpers --------------------------------------------------------------------------------
    def _flatten(self, obs_n, dist_adj, channels):
        """Reference reshapes (comm_categorical_mlp_policy.py:56-71): obs [...,N*d] -> [S,N,d],
        dist_adj [...,N*N]|[...,N,N] -> [S,N,N], channels [...,L*N,N]|[...,L,N,N] -> [S,L,N,N]."""
        N, Lh = self._n_agents, len(self.gcn_layers)
        lead = obs_n.shape[:-1] if obs_n.shape[-1] == N * self._dec_obs_dim else obs_n.shape[:-2]
        S = int(np.prod(lead)) if len(lead) else 1
        obs = obs_n.reshape(S, N, self._dec_obs_dim)
        adj = None if dist_adj is None else dist_adj.reshape(S, N, N)
        ch = None if channels is None else channels.reshape(S, Lh, N, N)
        return lead, S, obs, adj, ch

    def trunk(self, obs, adj, ch):
        """obs [S,N,d] -> (E, H_L, M) with autograd (CommBaseNet.forward :80-108)."""
        if not obs.is_cuda:
            raise L.CommarlError("policy / critic tensors must live on the MI355X (device cuda:k); there is no CPU path")
        E = self.encoder(obs)
        M = self.attention_layer(E)
        H = E
        for l, g in enumerate(self.gcn_layers):
            if _fused_ok(H, g.weight):
                hw = _LinearActFn.apply(H, g.weight, None, 0, 1)        # H.Wg, weight [in,out]
            else:
                hw = _MatmulWFn.apply(H, g.weight) if (H.is_cuda and torch.is_grad_enabled()) else torch.matmul(H, g.weight)
            H = masked_aggregate(M, adj, ch, l, hw, g.bias)
        return E, H, M

    # -- weight pack for the fused C-ABI forward -----------------------------------------------
    @property
    def _default_shape(self):
        """The reference's default layer sizes (env_uitils.py:84,140,182-192: 128 | 64 | head): the shape cm_policy_forward,
        cm_critic_forward, the rollout kernels and the fused training forward are built for.  Every other shape
        (--encoder_hidden_sizes, --embedding_dim, --categorical_mlp_hidden_sizes) runs on cm_policy_forward_any or layer by layer."""
        return self._enc_hidden == (128,) and self._embedding_dim == 64 and self._head_hidden() == self._HEAD_DEFAULT

    _is_policy = False                   # which saved forward and head _FusedNetFn runs (the policy class says True)

    def _gcn_tensors(self):
        """The hops' weights [in,out] and biases, each stacked hop by hop (None: no hop / no bias)."""
        gs = self.gcn_layers
        return OrderedDict(gcn_w=_Stacked(g.weight for g in gs) if len(gs) else None,
                           gcn_b=_Stacked(g.bias for g in gs) if len(gs) and gs[0].bias is not None else None)

    def _any_tensors(self):
        """The flat weight copy of a net of any layer sizes (cm_net_weights): every linear weight transposed [in,out], layer by layer."""
        t = OrderedDict()
        for pre, mlp in (("enc", self.encoder), ("head", self._head_mlp())):
            for i, lin in enumerate([l.linear for l in mlp._layers] + [mlp._output_layers[0].linear]):
                t[f"{pre}_w{i}t"] = lin.weight.t()
                t[f"{pre}_b{i}"] = lin.bias
        # 'dot': Q = E, no weight at all (NULL)
        t["attn_wt"] = self.attention_layer.linear_in.weight.t() if self.attention_layer.attention_type == "general" else None
        t.update(self._gcn_tensors())
        return t

    def _net_struct(self):
        """cm_net_weights of this net over its flat weight copy (any layer sizes): the policy's head is its categorical MLP, the
        'sum' critic's its decoder (one output column).  None outside the layer counts of cm_*_forward_any."""
        head, mlp = tuple(self._head_hidden()), self._head_mlp()
        if not (1 <= len(self._enc_hidden) <= 3 and 1 <= len(head) <= 4):
            return None                                          # more layers than the kernel is written for: layer by layer
        p = self._packed()
        w = L.NetWeights()
        w.d, w.n_agents, w.n_hops = self._dec_obs_dim, self._n_agents, len(self.gcn_layers)
        w.n_act = mlp._output_layers[0].linear.out_features
        w.no_residual, w.emb = 0 if self.residual else 1, self._embedding_dim
        w.n_enc, w.n_head = len(self._enc_hidden), len(head)
        for i, h in enumerate(self._enc_hidden):
            w.enc_hidden[i] = h
        for i, h in enumerate(head):
            w.head_hidden[i] = h
        for i in range(w.n_enc + 1):
            w.enc_wt[i], w.enc_b[i] = p[f"enc_w{i}t"], p[f"enc_b{i}"]
        for i in range(w.n_head + 1):
            w.head_wt[i], w.head_b[i] = p[f"head_w{i}t"], p[f"head_b{i}"]
        w.attn_wt, w.gcn_w, w.gcn_b = p["attn_wt"], p["gcn_w"], p["gcn_b"]
        return w

    def _trunk_tensors(self):
        enc = self.encoder
        if len(enc._layers) != 1:
            raise L.CommarlError("fused forward is built for one encoder hidden layer (the runners' default)")
        t = OrderedDict()
        t["enc_w1t"] = enc._layers[0].linear.weight.t()
        t["enc_b1"] = enc._layers[0].linear.bias
        t["enc_w2t"] = enc._output_layers[0].linear.weight.t()
        t["enc_b2"] = enc._output_layers[0].linear.bias
        if self.attention_layer.attention_type == "general":
            t["attn_wt"] = self.attention_layer.linear_in.weight.t()
        else:                                   # 'dot': Q = E, i.e. the fused kernels' linear_in is the identity (a constant)
            t["attn_wt"] = torch.eye(self._embedding_dim, dtype=torch.float32, device=next(self.parameters()).device)
        t.update(self._gcn_tensors())
        return t

    def _head_tensors(self):
        raise NotImplementedError

    def _pack_tensors(self):
        if not self._default_shape:
            return self._any_tensors()
        ts = self._trunk_tensors()
        ts.update(self._head_tensors())
        return ts

    def _after_pack(self, ptrs, sections=15):
        """(Re)build the matrix-core operand pack (cm_policy_pack / cm_critic_pack; `sections`: which parts) in its own
        persistent buffer: same address for the life of the net, so captured hipGraphs keep reading fresh weights."""
        dev = next(self.parameters()).device
        if dev.type != "cuda" or not self._default_shape:    # (cm_policy_forward_any reads the plain [in,out] weights)
            return
        w = self._struct_from(ptrs)
        size_fn, pack_fn = self._mfma_fns
        if self._mfma is None or self._mfma.device != dev:
            nbytes = getattr(L.lib(), size_fn)(C.byref(w))
            self._mfma = torch.zeros(nbytes // 4, dtype=torch.float32, device=dev) if nbytes else None
        if self._mfma is not None:
            L.run(pack_fn, C.byref(w), L.ptr(self._mfma), int(sections), device=dev)

    def _weights_struct(self):
        """The net's cm_policy_weights / cm_critic_weights over its current flat weight copy and operand pack."""
        w = self._struct_from(self._packed())
        w.mfma_pack = None if self._mfma is None else self._mfma.data_ptr()
        return w

    def _general_route(self, launch):
        """Which no-grad forward a net of non-default layer sizes takes, recorded in _last_forward.  launch(w) starts the
        one-launch kernel (cm_policy_forward_any / cm_critic_forward_any) over w = _net_struct() and says whether it ran.
        -> True ("one_launch"), or False ("layers": the caller runs layer by layer) where the route is pinned (_general_forward =
        "layers"), the net has more layers than the kernel is written for (no struct) or the kernel answered "not for this
        shape" (1: a workgroup's LDS need above 160 KB)."""
        if self._general_forward not in ("auto", "layers"):
            raise ValueError(f"_general_forward must be 'auto' or 'layers', not {self._general_forward!r}")
        w = self._net_struct() if self._general_forward == "auto" else None
        done = w is not None and launch(w)
        self._last_forward = "one_launch" if done else "layers"
        return done


class _Acting:
    """What the acting forwards (act_device) of the Comm-DP policy and the row-MLP policies share: the sampler's Philox stream,
    the policy-step counter and the output buffers."""

    def set_rng(self, seed, env_id_offset=0):
        """Philox stream of the action sampler: counter (env id, policy step, site 7, agent)."""
        self.seed, self.env_id_offset = int(seed), int(env_id_offset)

    def _next_step(self):
        """This policy's own step counter (what act_device uses when it is given no policy_step), which then advances."""
        self._policy_step += 1
        return self._policy_step - 1

    def _act_outputs(self, S, dev, want_actions, want_probs, want_attn, out_actions, out_probs, out_attn):
        """(actions int32 [S,N], probs [S,N,A], attn [S,N,N]) on `dev`: the caller's buffer, else a new one where wanted, else None."""
        if dev.type != "cuda":
            raise L.CommarlError("the rollout forward is a HIP kernel: inputs must be CUDA tensors (no CPU fallback)")
        N = self._n_agents
        if out_actions is None and want_actions:
            out_actions = torch.empty(S, N, dtype=torch.int32, device=dev)
        if out_probs is None and want_probs:
            out_probs = torch.empty(S, N, self._action_dim, dtype=torch.float32, device=dev)
        if out_attn is None and want_attn:
            out_attn = torch.empty(S, N, N, dtype=torch.float32, device=dev)
        return out_actions, out_probs, out_attn


# ---------------------------------------------------------------------------------------------
# policy
# ---------------------------------------------------------------------------------------------
class CommCategoricalMLPPolicy(_Acting, CommBaseNet):
    """comm_categorical_mlp_policy.py:8-141 (same ctor kwargs as runner_pp_commDP.py:49-61)."""

    def __init__(self, env_spec, n_agents, encoder_hidden_sizes=(128,), embedding_dim=64, attention_type="general",
                 n_gcn_layers=2, residual=True, gcn_bias=True, categorical_mlp_hidden_sizes=(128, 64, 32),
                 name="comm_categorical_mlp_policy", device="cpu"):
        super().__init__(env_spec=env_spec, n_agents=n_agents, encoder_hidden_sizes=encoder_hidden_sizes,
                         embedding_dim=embedding_dim, attention_type=attention_type, n_gcn_layers=n_gcn_layers,
                         gcn_bias=gcn_bias, name=name, device=device)
        self.residual = residual
        self._head_sizes = tuple(categorical_mlp_hidden_sizes)
        self.categorical_output_layer = MLPModule(embedding_dim, self._action_dim, categorical_mlp_hidden_sizes)
        self.seed, self.env_id_offset, self._policy_step = 1, 0, 0
        # layer sizes other than the default: which acting forward act_device takes - "auto": one launch (cm_policy_forward_any)
        # where it fits, else layer by layer; "layers": always layer by layer.  _last_forward says which one the last call took.
        self._general_forward, self._last_forward = "auto", None
        if not self._default_shape:
            # the per-layer training path (the any-width graph ops where the embedding is not 64, autograd's own adds everywhere) has not been
            # run under the update's hipGraphs: every non-default net steps eagerly, as teams above 80 agents do
            self._graph_capturable_update = False
        self.to(device)

    _HEAD_DEFAULT = (128, 64, 32)
    _is_policy = True

    def _head_hidden(self):
        return self._head_sizes

    def _head_mlp(self):
        return self.categorical_output_layer

    # -- autograd path (PPO update) --------------------------------------------------------------
    def _logits_flat(self, obs, adj, ch):
        """Raw head outputs [S,N,A] and attention [S,N,N] of flattened inputs: the fused training forward when it has an
        instantiation, under no_grad the same kernel storing only the logits, else the per-layer path."""
        fused_shape = len(self.categorical_output_layer._layers) == 3
        if _fused_train_ok(self, obs) and fused_shape:
            return _FusedNetFn.apply(self, obs, adj, ch, *self.parameters())          # one forward launch + hand-written backward
        if not torch.is_grad_enabled() and fused_shape and _fused_shape_ok(self, obs):
            return _fused_logits_nograd(self, obs, adj, ch)
        E, H, M = self.trunk(obs, adj, ch)
        x = E + H if self.residual else H
        return self.categorical_output_layer(x), M

    @torch.no_grad()
    def evaluate_nograd(self, obs_n, dist_adj, channels):
        """One no-grad forward over a batch -> (logits [...,N,A] or None, probs [...,N,A]): both from ONE launch when
        the fused training forward has an instantiation (the probabilities are the ones act_device returns, bit for bit),
        else the probabilities from act_device and no logits."""
        lead, S, obs, adj, ch = self._flatten(obs_n, dist_adj, channels)
        N = self._n_agents
        if _fused_shape_ok(self, obs) and len(self.categorical_output_layer._layers) == 3:
            logits, probs = _fused_logits_nograd(self, obs, adj, ch, want_probs=True)
            return logits.reshape(*lead, N, -1), probs.reshape(*lead, N, -1)
        _, probs, _ = self.act_device(obs.reshape(S, -1), None, adj, ch, want_actions=False, want_attn=False, policy_step=0)
        return None, probs.reshape(*lead, N, -1)

    def _logits(self, obs_n, dist_adj, channels):
        lead, S, obs, adj, ch = self._flatten(obs_n, dist_adj, channels)
        logits, _ = self._logits_flat(obs, adj, ch)
        return logits.reshape(*lead, self._n_agents, -1)

    def _probs(self, obs_n, avail_actions_n, dist_adj, channels):
        lead, S, obs, adj, ch = self._flatten(obs_n, dist_adj, channels)
        logits, M = self._logits_flat(obs, adj, ch)
        probs = torch.softmax(logits, dim=-1)
        if avail_actions_n is not None:
            probs = probs * avail_actions_n.reshape(S, self._n_agents, -1)
        probs = probs / probs.sum(dim=-1, keepdim=True)
        N = self._n_agents
        return probs.reshape(*lead, N, -1), M.reshape(*lead, N, N)

    def forward(self, obs_n, avail_actions_n, dist_adj, channels, get_actions=False):
        """-> (Categorical over [..., N, A], attention [..., N, N]).  get_actions=True takes
        numpy inputs and runs the fused no-grad kernel (reference :56-62,81-96)."""
        dev = next(self.parameters()).device
        if get_actions:
            obs_n, avail_actions_n = _as_dev(obs_n, dev), _as_dev(avail_actions_n, dev)
            dist_adj, channels = _as_dev(dist_adj, dev), _as_dev(channels, dev)
            _, probs, attn = self.act_device(obs_n, avail_actions_n, dist_adj, channels, want_actions=False)
            return Categorical(probs=probs.cpu()), attn.cpu()
        probs, attn = self._probs(obs_n, avail_actions_n, dist_adj, channels)
        return Categorical(probs=probs), attn

    def entropy(self, observations, avail_actions, dist_adj, channels):
        dists_n, _ = self.forward(observations, avail_actions, dist_adj, channels)
        return dists_n.entropy().mean(axis=-1)                       # :121-126

    def log_likelihood(self, observations, avail_actions, dist_adj, channels, actions):
        dists_n, _ = self.forward(observations, avail_actions, dist_adj, channels)
        return dists_n.log_prob(actions).sum(axis=-1)                # :128-137

    # -- fused rollout path ----------------------------------------------------------------------
    def _head_tensors(self):
        h = self.categorical_output_layer
        if len(h._layers) != 3:
            raise L.CommarlError("fused forward is built for the 3-hidden-layer categorical head (runner default)")
        t = OrderedDict()
        for i in range(3):
            t[f"hd_w{i + 1}t"] = h._layers[i].linear.weight.t()
            t[f"hd_b{i + 1}"] = h._layers[i].linear.bias
        t["hd_w4t"] = h._output_layers[0].linear.weight.t()
        t["hd_b4"] = h._output_layers[0].linear.bias
        return t

    def _struct_from(self, p):
        w = L.PolicyWeights()
        w.d, w.n_agents, w.n_hops = self._dec_obs_dim, self._n_agents, len(self.gcn_layers)
        w.enc_hidden, w.emb = self._enc_hidden[0], self._embedding_dim
        w.h1, w.h2, w.h3 = self._head_sizes
        w.n_act = self._action_dim
        w.no_residual = 0 if self.residual else 1
        for k, v in p.items():
            setattr(w, k, v)
        return w

    _mfma, _mfma_fns = None, ("cm_policy_pack_bytes", "cm_policy_pack_sections")

    @torch.no_grad()
    def act_device(self, obs, avail, dist_adj, channels, greedy=False, want_actions=True, want_probs=True,
                   want_attn=True, out_actions=None, out_probs=None, out_attn=None, policy_step=None, step_base=None,
                   env_id_offset=None):
        """Fused forward on device tensors: obs [S,N*d]|[S,N,d]; avail/dist_adj/channels may be None
        (= all ones).  Returns (actions int32 [S,N], probs [S,N,A], attn [S,N,N]) as CUDA tensors."""
        S = obs.numel() // (self._n_agents * self._dec_obs_dim)
        actions, probs, attn = self._act_outputs(S, obs.device, want_actions, want_probs, want_attn, out_actions, out_probs, out_attn)
        if policy_step is None:
            policy_step = self._next_step()
        rest = (obs.contiguous(), avail, dist_adj, channels, greedy, actions, probs, attn, policy_step, step_base, env_id_offset)
        if not self._default_shape:
            return self._act_device_any(*rest)
        if self._n_agents > MAX_FUSED_AGENTS:
            return self._act_device_layers(*rest)
        self._forward_launch("cm_policy_forward", self._weights_struct(), *rest)
        return actions, probs, attn

    def _forward_launch(self, name, w, obs, avail, dist_adj, channels, greedy, actions, probs, attn, policy_step, step_base,
                        env_id_offset, maybe=False):
        """cm_policy_forward / cm_policy_forward_any (`name`) over the weights struct `w`: forward + sample of S env states in one
        launch -> as L.run answers.  The call is written out instead of going through L.run: this is the per-step launch of an
        eager rollout, where the helper's extra Python frame showed (+1 us on 34 us per step)."""
        S = obs.numel() // (self._n_agents * self._dec_obs_dim)
        with torch.cuda.device(obs.device):
            rc = getattr(L.lib(), name)(
                C.byref(w), S, L.ptr(obs), L.cptr(avail), L.cptr(dist_adj), L.cptr(channels), self.seed,
                self.env_id_offset if env_id_offset is None else int(env_id_offset), policy_step & 0xFFFFFFFF,
                L.ptr(step_base), int(greedy), L.ptr(actions), L.ptr(probs), L.ptr(attn), L.current_stream())
        if maybe and rc == 1:
            return False
        L.check(rc, name)
        return True

    def _act_device_any(self, obs, avail, dist_adj, channels, greedy, actions, probs, attn, policy_step, step_base, env_id_offset):
        """Layer sizes other than the default: forward + sample in ONE launch of the run-time-sized kernel
        (cm_policy_forward_any, csrc/cm_policy_g.hip); where it answers "not for this shape" (1: a workgroup's LDS need above
        160 KB, more layers than it is written for) or the route is pinned (_general_forward = "layers"), layer by layer."""
        rest = (obs, avail, dist_adj, channels, greedy, actions, probs, attn, policy_step, step_base, env_id_offset)
        if self._general_route(lambda w: self._forward_launch("cm_policy_forward_any", w, *rest, maybe=True)):
            return actions, probs, attn
        return self._act_device_layers(*rest)

    def _act_device_layers(self, obs, avail, dist_adj, channels, greedy, actions, probs, attn, policy_step, step_base, env_id_offset):
        """Teams above 80 agents (PP map 40: N = 128; CO map 40: N = 96): one env's activation planes plus its N x N score matrix
        exceed a workgroup's 160 KB of LDS, so the forward runs layer by layer - encoder on the library GEMM, attention softmax
        and masked aggregation on their own HIP kernels (the training path's, up to 128 agents) - and the head + softmax x avail
        + Philox sample as ONE launch of the row-MLP kernel (cm_mlp_policy_forward) over x = E + H_L.  Same Philox site as the
        fused kernel: the sampled action is the oracle's inverse-CDF draw on the returned probabilities.  Also the route of nets
        with non-default layer sizes that cm_policy_forward_any does not take (_act_device_any)."""
        N, A, d = self._n_agents, self._action_dim, self._dec_obs_dim
        S = obs.numel() // (N * d)
        Lh = len(self.gcn_layers)
        E, H, M = self.trunk(obs.reshape(S, N, d), None if dist_adj is None else dist_adj.reshape(S, N, N),
                             None if channels is None else channels.reshape(S, Lh, N, N))
        x = (E + H if self.residual else H).reshape(S, N * self._embedding_dim).contiguous()
        hs = getattr(self, "_head_sampler_obj", None)
        if hs is None:
            hs = self.__dict__["_head_sampler_obj"] = _HeadSampler(self)       # (not a submodule: no new state_dict entries)
        hs.seed, hs.env_id_offset = self.seed, self.env_id_offset
        a_out, p_out, _ = hs.act_device(x, avail, greedy=greedy, want_actions=actions is not None, want_probs=True,
                                        out_actions=actions, out_probs=probs, policy_step=policy_step, step_base=step_base,
                                        env_id_offset=env_id_offset)
        if attn is not None:
            attn.copy_(M.reshape(attn.shape))
        return a_out, p_out, attn

    def _rollout_call(self, name, env_batch, head, obs, after_obs, dist_adj, channels, step_out, before_out, after_out, greedy,
                      out_actions, out_probs, out_attn, policy_step, step_base, env_id_offset):
        """One call of the cm_rollout_* family: what they share (handle, weights, slot pointers, sampler counters, outputs),
        with the entry point's own arguments spliced in where its signature has them.  False when the library answers
        "not for this shape" (1), having done nothing."""
        if not self._default_shape:                          # the rollout kernels are built for the default layer sizes
            return False
        w = self._weights_struct()
        return L.run(name, env_batch._h, C.byref(w), *head, L.ptr(obs), *after_obs, L.ptr(dist_adj), L.ptr(channels), self.seed,
                     self.env_id_offset if env_id_offset is None else int(env_id_offset), policy_step & 0xFFFFFFFF,
                     L.ptr(step_base), int(greedy), L.ptr(out_actions), L.ptr(out_probs), L.ptr(out_attn), *before_out,
                     C.byref(step_out), *after_out, device=obs.device, maybe=True)

    @torch.no_grad()
    def step_fused(self, env_batch, obs, dist_adj, channels, step_out, greedy=False, out_actions=None, out_probs=None,
                   out_attn=None, policy_step=0, step_base=None, env_id_offset=None, tape=None):
        """One sampler iteration in ONE launch (cm_rollout_step): this policy's forward + sample on `obs`, then the env
        step of `env_batch` on the sampled actions, results into `step_out` (an _lib.StepOut of device pointers).
        Returns False - having done nothing - when the library has no fused kernel for this shape."""
        return self._rollout_call("cm_rollout_step", env_batch, (), obs, (None,), dist_adj, channels, step_out,
                                  (C.byref(tape) if tape is not None else None,), (), greedy, out_actions, out_probs, out_attn,
                                  policy_step, step_base, env_id_offset)

    @torch.no_grad()
    def chunk_fused(self, env_batch, n_steps, strides, obs, dist_adj, channels, step_out, greedy=False, out_actions=None,
                    out_probs=None, out_attn=None, policy_step=0, step_base=None, env_id_offset=None, tail_next=None):
        """n_steps sampler iterations in ONE persistent launch (cm_rollout_chunk): pointers are those of the first
        step, `strides` (_lib.ChunkStrides) the per-step element strides of the time-major buffers.  tail_next = (obs,
        dist_adj | None, channels | None) of the slot that receives the last step's outputs, with the advance of `step_base`
        by n_steps (cm_rollout_chunk_tail: part of the same launch where the library can).  Returns False - having done
        nothing - when the library has no fused kernel for this shape."""
        tail = () if tail_next is None else tuple(L.ptr(x) for x in tail_next)
        return self._rollout_call("cm_rollout_chunk_tail" if tail else "cm_rollout_chunk", env_batch, (int(n_steps), C.byref(strides)),
                                  obs, (), dist_adj, channels, step_out, (), tail, greedy, out_actions, out_probs, out_attn,
                                  policy_step, step_base, env_id_offset)

    def get_actions(self, obs_n, avail_actions_n, dist_adj, channels, greedy=False):
        """numpy in / numpy out, as the reference sampler calls it (:98-119)."""
        dev = next(self.parameters()).device
        obs = _as_dev(obs_n, dev)
        S = obs.shape[0]
        act, probs, attn = self.act_device(obs.reshape(S, -1), _as_dev(avail_actions_n, dev), _as_dev(dist_adj, dev),
                                           _as_dev(channels, dev), greedy=greedy)
        probs, attn = probs.cpu().numpy(), attn.cpu().numpy()
        infos = dict(action_probs=[probs[i] for i in range(S)], attention_weights=[attn[i] for i in range(S)])
        return act.cpu().numpy().astype(np.int64), infos


# ---------------------------------------------------------------------------------------------
# critic
# ---------------------------------------------------------------------------------------------
class GaussianMLPModule(nn.Module):
    """gaussian_mlp_module.py:62-188 in the configuration the critic uses: learned shared
    log-std ``_init_std`` (init log 1.0), min_std 1e-6, exp parameterisation."""

    def __init__(self, input_dim, output_dim, hidden_sizes=(32, 32), init_std=1.0, min_std=1e-6):
        super().__init__()
        self._init_std = nn.Parameter(torch.Tensor([init_std]).log())
        self._min_std_param = None if min_std is None else math.log(min_std)
        self._mean_module = MLPModule(input_dim, output_dim, hidden_sizes)

    def forward(self, x):
        mean = self._mean_module(x)
        ls = self._init_std if self._min_std_param is None else self._init_std.clamp(min=self._min_std_param)
        return mean, ls.exp()


class _GaussNLLFn(torch.autograd.Function):
    """The critic's Gaussian NLL from the per-agent outputs in one launch, its gradient in one more (cm_gauss_nll_*:
    comm_base_critic.py:59-89 + :110-112 + the std of gaussian_mlp_module.py) instead of ~25 framework launches each way."""

    @staticmethod
    def forward(ctx, per_agent, returns, log_std, min_log_std, ws):
        S, N = per_agent.shape
        pa, r = per_agent.contiguous(), returns.contiguous()
        out = torch.empty(2, dtype=torch.float32, device=pa.device)
        has_min = 0 if min_log_std is None else 1
        # (deterministic mode: block sums summed in a fixed order, no f64 atomics)
        L.launch("cm_gauss_nll_forward", (S, N, L.ptr(pa), L.ptr(r), L.ptr(log_std), float(min_log_std or 0.0), has_min,
                                          L.ptr(out), L.ptr(ws)), (S,), device=pa.device)
        ctx.save_for_backward(pa, r, log_std, out)
        ctx.min_log_std = min_log_std
        return out[0]

    @staticmethod
    def backward(ctx, g):
        pa, r, log_std, out = ctx.saved_tensors
        S, N = pa.shape
        d_pa, d_ls = torch.empty_like(pa), torch.empty_like(log_std)
        g = g.to(torch.float32).contiguous()
        L.run("cm_gauss_nll_backward", S, N, L.ptr(pa), L.ptr(r), L.ptr(log_std), float(ctx.min_log_std or 0.0),
              0 if ctx.min_log_std is None else 1, L.ptr(out), L.ptr(g), L.ptr(d_pa), L.ptr(d_ls), device=pa.device)
        return d_pa, None, d_ls, None, None


class CommBaseCritic(CommBaseNet):
    """comm_base_critic.py:11-122, aggregators 'sum' and 'direct' (same ctor kwargs as runner_pp_commDP.py:63-74)."""

    def __init__(self, env_spec, n_agents, encoder_hidden_sizes=(128,), embedding_dim=64, decoder_hidden_sizes=(64,),
                 attention_type="general", n_gcn_layers=2, residual=True, gcn_bias=True, share_std=False,
                 state_include_actions=False, aggregator_type="sum", name="base_critic", device="cpu"):
        super().__init__(env_spec=env_spec, n_agents=n_agents, encoder_hidden_sizes=encoder_hidden_sizes,
                         embedding_dim=embedding_dim, attention_type=attention_type, n_gcn_layers=n_gcn_layers,
                         residual=residual, gcn_bias=gcn_bias, state_include_actions=state_include_actions, name=name,
                         device=device)
        if aggregator_type not in ("sum", "direct"):
            raise ValueError("aggregator_type must be 'sum' or 'direct' (comm_base_critic.py:46-49)")
        self.aggregator_type = aggregator_type
        self._dec_hidden = tuple(decoder_hidden_sizes)
        if aggregator_type != "sum" or n_agents > MAX_FUSED_AGENTS or not self._default_shape:
            self._graph_capturable_update = False        # framework GEMMs / per-layer fallbacks in the step: eager
        # 'sum': one value per agent from its embedding, summed (:110-112).  'direct': ONE value from the concatenated
        # embeddings of the whole team (:113-116) - the head is then a plain [N * 64] -> 64 -> 1 MLP on the framework's GEMMs
        # behind the fused trunk kernels (per-layer path; the fused critic kernels carry the per-agent head only)
        agg_in = embedding_dim if aggregator_type == "sum" else embedding_dim * n_agents
        self.baseline_aggregator = GaussianMLPModule(agg_in, 1, hidden_sizes=decoder_hidden_sizes)
        # 'sum' critics of layer sizes other than the default: which no-grad forward values_device takes - "auto": one launch
        # (cm_critic_forward_any) where it fits, else layer by layer; "layers": always layer by layer.  _last_forward says which one
        # the last call took (it stays None on the 'direct' and default-shape routes).
        self._general_forward, self._last_forward = "auto", None
        self.to(device)

    _HEAD_DEFAULT = (64,)

    def _head_hidden(self):
        return self._dec_hidden

    def _head_mlp(self):
        return self.baseline_aggregator._mean_module

    def sync_weights(self):
        if self.aggregator_type == "sum":
            super().sync_weights()                       # 'direct': no fused kernel, hence no weight pack to refresh

    def _head_tensors(self):
        m = self.baseline_aggregator._mean_module
        if len(m._layers) != 1:
            raise L.CommarlError("fused critic forward is built for one decoder hidden layer (default)")
        return OrderedDict(dec_w1t=m._layers[0].linear.weight.t(), dec_b1=m._layers[0].linear.bias,
                           dec_w2t=m._output_layers[0].linear.weight.t(), dec_b2=m._output_layers[0].linear.bias)

    _mfma, _mfma_fns = None, ("cm_critic_pack_bytes", "cm_critic_pack_sections")

    def _struct_from(self, p):
        w = L.CriticWeights()
        w.d, w.n_agents, w.n_hops = self._dec_obs_dim, self._n_agents, len(self.gcn_layers)
        w.enc_hidden, w.emb, w.dec_hidden = self._enc_hidden[0], self._embedding_dim, self._dec_hidden[0]
        w.no_residual = 0 if self.residual else 1
        for k, v in p.items():
            setattr(w, k, v)
        return w

    def _fused_head_ok(self, obs):
        return (self.aggregator_type == "sum" and _fused_train_ok(self, obs)
                and len(self.baseline_aggregator._mean_module._layers) == 1)

    def _values_grad(self, obs_n, dist_adj, channels):
        lead, S, obs, adj, ch = self._flatten(obs_n, dist_adj, channels)
        if self.aggregator_type == "direct":
            E, H, _ = self.trunk(obs, adj, ch)
            x = E + H if self.residual else H
            mean, std = self.baseline_aggregator(x.reshape(S, -1))                   # concatenated embeddings (:113-115)
            return mean.squeeze(-1).reshape(*lead), std
        if self._fused_head_ok(obs):
            per_agent, _ = _FusedNetFn.apply(self, obs, adj, ch, *self.parameters())  # [S,N] per-agent means
            ag = self.baseline_aggregator
            ls = ag._init_std if ag._min_std_param is None else ag._init_std.clamp(min=ag._min_std_param)
            return per_agent.sum(-1).reshape(*lead), ls.exp()
        E, H, _ = self.trunk(obs, adj, ch)
        x = E + H if self.residual else H
        mean, std = self.baseline_aggregator(x)
        return mean.squeeze(-1).sum(-1).reshape(*lead), std

    @torch.no_grad()
    def values_device(self, obs, dist_adj, channels, out=None):
        """Fused no-grad forward (cm_critic_forward; cm_critic_forward_any for other layer sizes): obs [..., N*d] CUDA -> values [...]."""
        dev = obs.device
        if dev.type != "cuda":
            raise L.CommarlError("critic forward is a HIP kernel: inputs must be CUDA tensors (no CPU fallback)")
        N = self._n_agents
        lead = obs.shape[:-1] if obs.shape[-1] == N * self._dec_obs_dim else obs.shape[:-2]
        S = obs.numel() // (N * self._dec_obs_dim)
        values = None

        def launch(name, w, maybe=False):
            nonlocal values
            values = out if out is not None else torch.empty(S, dtype=torch.float32, device=dev)
            return L.run(name, C.byref(w), S, L.cptr(obs), L.cptr(dist_adj), L.cptr(channels), L.ptr(values), device=dev, maybe=maybe)

        if self.aggregator_type == "sum" and not self._default_shape:
            # layer sizes other than the default: ONE launch of the run-time-sized kernel (cm_critic_forward_any, csrc/cm_critic_g.hip);
            # where it answers "not for this shape" (1) or the route is pinned (_general_forward = "layers"), layer by layer
            one_launch = self._general_route(lambda w: launch("cm_critic_forward_any", w, maybe=True))
        elif self.aggregator_type == "sum" and N <= MAX_FUSED_AGENTS:
            one_launch = launch("cm_critic_forward", self._weights_struct())
        else:
            one_launch = False
        if not one_launch:                                   # 'direct', teams above 80 agents, sizes the kernel refuses: layer by layer
            v = self._values_grad(obs, dist_adj, channels)[0]
            return v if out is None else out.copy_(v.reshape(out.shape))
        return values.reshape(*lead) if out is None else values

    def forward(self, obs_n, avail_actions_n, dist_adj, channels, get_actions=False):
        """-> values [P,T] (:91-114).  Under no_grad this is the fused kernel."""
        dev = next(self.parameters()).device
        if get_actions or not torch.is_tensor(obs_n):
            obs_n, dist_adj, channels = _as_dev(obs_n, dev), _as_dev(dist_adj, dev), _as_dev(channels, dev)
        if not torch.is_grad_enabled():
            return self.values_device(obs_n, dist_adj, channels)
        return self._values_grad(obs_n, dist_adj, channels)[0]

    def compute_loss(self, obs_n, returns, dist_adj, channels, get_actions=False):
        """Gaussian NLL with the shared learned std; padded steps are included in the mean (:59-89)."""
        lead, S, obs, adj, ch = self._flatten(obs_n, dist_adj, channels)
        ag = self.baseline_aggregator
        if (self._fused_head_ok(obs) and torch.is_tensor(returns) and returns.is_cuda and returns.dtype == torch.float32
                and ag._init_std.numel() == 1):
            per_agent, _ = _FusedNetFn.apply(self, obs, adj, ch, *self.parameters())  # [S,N] per-agent means
            ws = getattr(self, "_nll_ws", None)
            if ws is None or ws.device != per_agent.device:
                ws = self._nll_ws = torch.zeros(2, dtype=torch.float64, device=per_agent.device)   # CM_GAUSS_WS_BYTES, left zero by each launch
            return _GaussNLLFn.apply(per_agent, returns.reshape(-1), ag._init_std, ag._min_std_param, ws)
        values, std = self._values_grad(obs_n, dist_adj, channels)
        # validate_args=False: the constructor's argument check reads a device flag back (a host sync per optimiser step, and not
        # capturable into the update's hipGraphs); a non-finite value still surfaces - as a NaN loss in the epoch's statistics
        return -Normal(values, std.mean(), validate_args=False).log_prob(returns).mean()


# ---------------------------------------------------------------------------------------------
# Obs-DP / CENT variants: no communication, plain row-wise MLPs
# ---------------------------------------------------------------------------------------------
class _RowMLPPolicy(_Acting, _WeightPack):
    """Shared rollout path of the two non-communicating policies: one fused HIP launch
    (cm_mlp_policy_forward, csrc/cm_mlp.hip) over the layer chain listed by ``_chain()``."""

    def _chain(self):
        """-> list of (nn.Linear, activation code) in forward order: 0 none, 1 (or True) tanh, 2 ReLU."""
        raise NotImplementedError

    def _pack_tensors(self):
        t = OrderedDict()
        for i, (lin, _) in enumerate(self._chain()):
            t[f"w{i}t"] = lin.weight.t()
            t[f"b{i}"] = lin.bias
        return t

    _mlp_pack = None

    def _after_pack(self, ptrs, sections=15):
        """(Re)build the B-fragment pack of the chain (cm_mlp_pack) in a persistent buffer."""
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            return
        w = self._struct_from(ptrs)
        if self._mlp_pack is None or self._mlp_pack.device != dev:
            self._mlp_pack = torch.zeros(L.lib().cm_mlp_pack_bytes(C.byref(w)) // 4, dtype=torch.float32, device=dev)
        L.run("cm_mlp_pack", C.byref(w), L.ptr(self._mlp_pack), device=dev)

    def _mlp_struct(self):
        w = self._struct_from(self._packed())
        w.mfma_pack = None if self._mlp_pack is None else self._mlp_pack.data_ptr()
        return w

    def _struct_from(self, p):
        chain = self._chain()
        if len(chain) > L.MLP_MAX_LAYERS:
            raise L.CommarlError(f"fused MLP forward takes at most {L.MLP_MAX_LAYERS} linear layers")
        w = L.MlpWeights()
        w.in_dim, w.n_layers, w.tanh_mask, w.relu_mask = chain[0][0].in_features, len(chain), 0, 0
        for i, (lin, act) in enumerate(chain):
            w.out_dim[i] = lin.out_features
            w.wt[i], w.b[i] = p[f"w{i}t"], p[f"b{i}"]
            w.tanh_mask |= int(int(act) == ACT_TANH) << i
            w.relu_mask |= int(int(act) == ACT_RELU) << i
        return w

    @torch.no_grad()
    def act_device(self, obs, avail=None, dist_adj=None, channels=None, greedy=False, want_actions=True,
                   want_probs=True, want_attn=False, out_actions=None, out_probs=None, out_attn=None,
                   policy_step=None, step_base=None, env_id_offset=None):
        """obs [S,N*d] (CUDA) -> (actions int32 [S,N], probs [S,N,A], None).  dist_adj / channels are accepted
        and ignored so the rollout engine drives every policy through one call shape."""
        N, A = self._n_agents, self._action_dim
        S = obs.numel() // (N * self._dec_obs_dim)
        actions, probs, _ = self._act_outputs(S, obs.device, want_actions, want_probs, False, out_actions, out_probs, None)
        if policy_step is None:
            policy_step = self._next_step()
        rows, groups = (S * N, 1) if self._per_agent_rows else (S, N)
        obs, w = obs.contiguous(), self._mlp_struct()
        L.run("cm_mlp_policy_forward", C.byref(w), rows, groups, A, N, L.ptr(obs), L.cptr(avail), self.seed,
              self.env_id_offset if env_id_offset is None else int(env_id_offset), policy_step & 0xFFFFFFFF,
              L.ptr(step_base), int(greedy), L.ptr(actions), L.ptr(probs), device=obs.device)
        return actions, probs, None

    def evaluate_nograd(self, obs_n, dist_adj=None, channels=None):
        """One no-grad forward over a batch [..., N*d] -> (None, probs [..., N, A]): CommCategoricalMLPPolicy.evaluate_nograd's
        contract, on act_device's launch (no logits: the PPO loss runs the autograd modules for those)."""
        _, probs, _ = self.act_device(obs_n.reshape(-1, obs_n.shape[-1]), want_actions=False, policy_step=0)
        return None, probs.reshape(*obs_n.shape[:-1], self._n_agents, -1)

    def get_actions(self, observations, avail_actions, greedy=False):
        """numpy in / numpy out (dec_categorical_mlp_policy.py:150-176, centralized_...:99-118)."""
        dev = next(self.parameters()).device
        obs = _as_dev(observations, dev)
        S = obs.shape[0]
        act, probs, _ = self.act_device(obs.reshape(S, -1), _as_dev(avail_actions, dev), greedy=greedy)
        probs = probs.cpu().numpy()
        return act.cpu().numpy().astype(np.int64), dict(action_probs=[probs[i] for i in range(S)])

    def forward(self, obs_n, avail_actions_n, get_actions=False):
        """-> Categorical over [..., N, A] (masked + renormalised)."""
        dev = next(self.parameters()).device
        if get_actions:
            obs_n, avail_actions_n = _as_dev(obs_n, dev), _as_dev(avail_actions_n, dev)
            _, probs, _ = self.act_device(obs_n.reshape(-1, self._n_agents * self._dec_obs_dim), avail_actions_n,
                                          want_actions=False)
            return Categorical(probs=probs.reshape(*obs_n.shape[:-1], self._n_agents, -1).cpu())
        return Categorical(probs=self._probs(obs_n, avail_actions_n)[0])

    @staticmethod
    def _need_gpu(x):
        if not x.is_cuda:
            raise L.CommarlError("policy tensors must live on the MI355X (device cuda:k); there is no CPU path")

    def _masked(self, logits, avail_actions_n):
        probs = torch.softmax(logits, dim=-1)
        if avail_actions_n is not None:
            probs = probs * avail_actions_n.reshape(probs.shape)
        return probs / probs.sum(dim=-1, keepdim=True)

    def entropy(self, observations, avail_actions):
        return self.forward(observations, avail_actions).entropy().mean(axis=-1)

    def log_likelihood(self, observations, avail_actions, actions):
        return self.forward(observations, avail_actions).log_prob(actions).sum(axis=-1)

    @property
    def vectorized(self):
        return True


class _HeadSampler(_RowMLPPolicy):
    """The Comm-DP policy's head (64 -> 128 -> 64 -> 32 -> A, categorical_mlp_module.py:64-80) + softmax x avail + Philox sample as
    a row-MLP chain over the trunk output x = E + H_L: the rollout forward of teams too large for the one-launch kernel."""
    _per_agent_rows = True

    def __init__(self, policy):
        self._policy = policy
        self._n_agents, self._action_dim = policy._n_agents, policy._action_dim
        self._dec_obs_dim = self._obs_dim = policy._embedding_dim
        self.seed, self.env_id_offset, self._policy_step = policy.seed, policy.env_id_offset, 0

    def parameters(self):
        return self._policy.categorical_output_layer.parameters()

    def _chain(self):
        h = self._policy.categorical_output_layer
        return [(l.linear, True) for l in h._layers] + [(h._output_layers[0].linear, False)]


class DecCategoricalMLPPolicy(_RowMLPPolicy, MLPModule):
    """dec_categorical_mlp_policy.py:14-232 (ctor of runner_pp_obsDP.py:52-59).  ``hidden_sizes`` =
    (encoder hidden, embedding, head hidden); parameters: ``_layers.0`` / ``_output_layers.0`` (head, created
    first as in the reference) and ``encoder.*``."""
    _per_agent_rows = True

    def __init__(self, env_spec, n_agents, hidden_sizes=(32, 32), hidden_nonlinearity=torch.tanh,
                 name="DecCategoricalMLPPolicy", device="cpu", _embedding_dim=64):
        act = hidden_act_code(hidden_nonlinearity)
        self._n_agents = n_agents
        self._dec_obs_dim = self._obs_dim = int(env_spec.observation_space.flat_dim / n_agents)
        self._action_dim = env_spec.action_space.n
        self._embedding_dim = hidden_sizes[1]
        # the head's hidden layers take hidden_nonlinearity (dec_categorical_mlp_policy.py:80-90); the encoder stays tanh
        # (MLPEncoderModule's default, :92-95)
        MLPModule.__init__(self, self._embedding_dim, self._action_dim, (hidden_sizes[-1],), hidden_act=act)
        self.hidden_nonlinearity = "relu" if act == ACT_RELU else "tanh"      # a string: the net still pickles
        self.encoder = MLPModule(self._obs_dim, self._embedding_dim, (hidden_sizes[0],), output_tanh=True)
        self.device, self.name, self.step, self.centralized = device, name, 0, True
        self.seed, self.env_id_offset, self._policy_step = 1, 0, 0
        self.to(device)

    def _chain(self):
        e = self.encoder
        return ([(l.linear, ACT_TANH) for l in e._layers] + [(e._output_layers[0].linear, ACT_TANH)]
                + [(l.linear, self._hidden_act) for l in self._layers] + [(self._output_layers[0].linear, ACT_NONE)])

    def _logits(self, obs_n, dist_adj=None, channels=None):
        """Raw per-agent logits [..., N, A] (what CentralizedMAPPO's one-launch surrogate loss consumes)."""
        self._need_gpu(obs_n)
        obs = obs_n.reshape(obs_n.shape[:-1] + (self._n_agents, -1))              # :110
        return MLPModule.forward(self, self.encoder(obs))

    def _probs(self, obs_n, avail_actions_n, dist_adj=None, channels=None):
        return self._masked(self._logits(obs_n), avail_actions_n), None


class CentralizedCategoricalMLPPolicy(_RowMLPPolicy, MLPModule):
    """centralized_categorical_mlp_policy.py:11-144 (ctor of runner_pp_cent.py:51-59): one MLP over the
    concatenated observation, N x 5 logits, agents' actions independent given the joint observation."""
    _per_agent_rows = False

    def __init__(self, env_spec, n_agents, hidden_sizes=(32, 32), hidden_nonlinearity=torch.tanh,
                 name="CentralizedCategoricalMLPPolicy", device="cpu"):
        act = hidden_act_code(hidden_nonlinearity)                       # every hidden layer (centralized_...:40-50)
        self._n_agents = n_agents
        self._obs_dim = env_spec.observation_space.flat_dim
        self._dec_obs_dim = self._obs_dim // n_agents
        self._action_dim = env_spec.action_space.n
        MLPModule.__init__(self, self._obs_dim, self._action_dim * n_agents, tuple(hidden_sizes), hidden_act=act)
        self.hidden_nonlinearity = "relu" if act == ACT_RELU else "tanh"
        self.device, self.name, self.step, self.centralized = device, name, 0, True
        self.seed, self.env_id_offset, self._policy_step = 1, 0, 0
        self.to(device)

    def _chain(self):
        return [(l.linear, self._hidden_act) for l in self._layers] + [(self._output_layers[0].linear, ACT_NONE)]

    def _logits(self, obs_n, dist_adj=None, channels=None):
        """Raw logits [..., N, A] (what CentralizedMAPPO's one-launch surrogate loss consumes)."""
        self._need_gpu(obs_n)
        logits = MLPModule.forward(self, obs_n)
        return logits.reshape(logits.shape[:-1] + (self._n_agents, -1))           # :83

    def _probs(self, obs_n, avail_actions_n, dist_adj=None, channels=None):
        return self._masked(self._logits(obs_n), avail_actions_n), None


class GaussianMLPBaseline(_WeightPack, nn.Module):
    """com_marl/torch/baselines/gaussian_mlp_baseline.py:7-115 (runner_pp_cent.py:61-63): V(s) from the
    concatenated observation, Gaussian NLL with a learned shared std (no clamp: min_std=None)."""

    def __init__(self, env_spec, hidden_sizes=(32, 32), learn_std=True, init_std=1.0, name="GaussianMLPBaseline",
                 device="cpu", **unused):
        super().__init__()
        self.name = name
        self.input_dim = env_spec.observation_space.flat_dim
        self.module = GaussianMLPModule(self.input_dim, 1, hidden_sizes=tuple(hidden_sizes), init_std=init_std,
                                        min_std=None)
        if not learn_std:
            self.module._init_std.requires_grad_(False)
        self.device = device
        self.to(device)

    def _chain(self):
        m = self.module._mean_module
        return [(l.linear, True) for l in m._layers] + [(m._output_layers[0].linear, False)]

    _pack_tensors = _RowMLPPolicy._pack_tensors
    _mlp_struct = _RowMLPPolicy._mlp_struct
    _struct_from = _RowMLPPolicy._struct_from
    _after_pack = _RowMLPPolicy._after_pack
    _mlp_pack = None

    @torch.no_grad()
    def values_device(self, obs, out=None):
        """Fused no-grad forward (cm_mlp_value_forward): obs [..., input_dim] CUDA -> values [...]; `out` (f32, contiguous, one value
        per row) receives them when given and is returned as it is."""
        dev = obs.device
        if dev.type != "cuda":
            raise L.CommarlError("baseline forward is a HIP kernel: inputs must be CUDA tensors (no CPU fallback)")
        lead = obs.shape[:-1]
        rows = obs.numel() // self.input_dim
        values = out if out is not None else torch.empty(rows, dtype=torch.float32, device=dev)
        w = self._mlp_struct()
        L.run("cm_mlp_value_forward", C.byref(w), rows, L.cptr(obs), L.ptr(values), device=dev)
        return values.reshape(*lead) if out is None else values

    def forward(self, obs):
        """-> values [P,T] (:100-115).  Under no_grad this is the fused kernel."""
        if not torch.is_tensor(obs):
            obs = _as_dev(obs, next(self.parameters()).device)
        if not torch.is_grad_enabled():
            return self.values_device(obs)
        return self.module(obs)[0].flatten(-2)

    def compute_loss(self, obs, returns):
        _RowMLPPolicy._need_gpu(obs)
        mean, std = self.module(obs.reshape(-1, self.input_dim))                  # :93-96
        return -Normal(mean, std, validate_args=False).log_prob(returns.reshape(-1, 1)).mean()      # (no host sync, as above)


# ---------------------------------------------------------------------------------------------
# policy sets (several policies of one architecture in one rollout)
# ---------------------------------------------------------------------------------------------
def _architecture(p):
    """(name, value) pairs that must agree between the members of a PolicySet, in the order they are checked."""
    comm = isinstance(p, CommBaseNet)
    act = p.categorical_output_layer._hidden_act if comm else getattr(p, "_hidden_act", ACT_TANH)
    return [("class", type(p).__name__), ("team size", p._n_agents), ("observation dim", p._dec_obs_dim),
            ("action dim", p._action_dim),
            ("hops", len(p.gcn_layers) if comm else None),
            ("attention type", p.attention_layer.attention_type if comm else None),
            ("residual", bool(p.residual) if comm else None),
            ("hidden sizes", tuple((n, tuple(t.shape)) for n, t in p.named_parameters())),
            ("hidden nonlinearity", int(act)),
            ("device", next(p.parameters()).device)]


# what the members of a PolicySet(any_sizes=True) of Comm-DP policies may differ in: the layer sizes (encoder, embedding, head),
# 'general' / 'dot' attention, the residual and the GCN bias (the last is part of "hidden sizes": a parameter more or less)
_ANY_SIZES_FREE = ("attention type", "residual", "hidden sizes")


def _differences(policies, skip=()):
    """(member index, field, value, member 0's value) of the first disagreement with member 0 in a field not in `skip`, or None."""
    ref = _architecture(policies[0])
    for i, p in enumerate(policies[1:], 1):
        for (name, v0), (_, v) in zip(ref, _architecture(p)):
            if v != v0 and name not in skip:
                return i, name, v, v0
    return None


class PolicySet:
    """K policies of ONE architecture (class, team size, observation dim, hops, attention type, residual, hidden sizes, hidden
    nonlinearity, device) that one RolloutEngine runs side by side, each on its own contiguous range of the envs - e.g. the
    checkpoints of one run evaluated at once (evaluate.eval_models).  What the engine reads from a policy (``_n_agents``,
    ``_action_dim``, ``comm``, ...) comes from member 0; ``sync_weights()`` refreshes every member's pack,
    ``pack_table()`` keeps the device table of the members' pack addresses that cm_rollout_chunk_multi reads and
    ``forward_table()`` the one the set forward reads (cm_policy_forward_multi for Comm-DP members,
    cm_mlp_policy_forward_multi for Obs-DP / CENT members).

    any_sizes=True (Comm-DP members only; Obs-DP / CENT members keep the whole check): the members may differ in their layer
    sizes - encoder hidden sizes, embedding dim, head hidden sizes -, in 'general' / 'dot' attention, the residual and the GCN
    bias (an architecture ablation in one rollout); class, team size, observation dim, action dim, hops, hidden nonlinearity and
    device still agree.  Such a set of non-default nets - mixed or K checkpoints of one non-default shape - takes its forward as
    ONE cm_policy_forward_any_multi launch per step (``set_kernel == "any"``); with a member of the default layer sizes in it, it
    runs member by member.  A set whose members pass the whole check and have the default sizes behaves as without the keyword.
    ``uniform`` says whether the members pass the whole check (always true without the keyword); ``forward_kind`` names the set
    forward the members can have: "mlp" (Obs-DP / CENT), "default" (Comm-DP, default layer sizes), "any" (Comm-DP, any sizes) or
    None (no set kernel: member by member)."""
    _SHARED = ("_n_agents", "_action_dim", "_dec_obs_dim", "_obs_dim", "comm", "centralized", "device", "n_gcn_layers")

    def __init__(self, policies, any_sizes=False):
        policies = list(policies)
        if not policies:
            raise ValueError("PolicySet needs at least one policy")
        comm = all(isinstance(p, CommBaseNet) for p in policies)
        self.any_sizes = bool(any_sizes)
        bad = _differences(policies, skip=_ANY_SIZES_FREE if (self.any_sizes and comm) else ())
        if bad is not None:
            i, name, v, v0 = bad
            raise ValueError(f"PolicySet: policies[{i}] differs from policies[0] in {name}: {v!r} != {v0!r}")
        self.uniform = not (self.any_sizes and comm) or _differences(policies) is None
        # the kind of set forward the members can have (a key of _FORWARDS, or None: member by member), decided here once.  (The
        # class is part of the check above: what member 0 has, every member has.)
        default = self.uniform and all(getattr(p, "_default_shape", True) for p in policies)
        if all(hasattr(p, "_mlp_struct") for p in policies):
            self.forward_kind = "mlp"               # Obs-DP / CENT
        elif self.any_sizes and comm and not default:
            # the route of the run-time-sized set kernel: opted into, and not the set the default kernels already serve
            self.forward_kind = "any"
        elif default and all(hasattr(p, "_weights_struct") for p in policies):
            self.forward_kind = "default"           # Comm-DP policies of the default layer sizes
        else:
            self.forward_kind = None
        self.set_kernel = "any" if self.forward_kind == "any" else "default"
        self.policies = policies
        self._table = None                      # (pack addresses, int64 device tensor of them)
        self._fwd_table = None                  # (key, device image | None, workgroup count): forward_table()
        self.forward_lds = 0                    # set_kernel "any": the launch's dynamic LDS bytes, with _fwd_table

    def __getattr__(self, name):
        if name in PolicySet._SHARED:
            return getattr(self.policies[0], name)
        raise AttributeError(name)

    def __len__(self):
        return len(self.policies)

    def __getitem__(self, k):
        return self.policies[k]

    def __iter__(self):
        return iter(self.policies)

    @property
    def seed(self):
        """The sampler seed the members share, or None when they differ (one launch keys one Philox stream)."""
        seeds = {p.seed for p in self.policies}
        return seeds.pop() if len(seeds) == 1 else None

    def sync_weights(self):
        for p in self.policies:
            p.sync_weights()

    def reset(self, dones=None):
        for p in self.policies:
            p.reset(dones)

    def pack_table(self):
        """int64 device tensor [K] of the members' operand-pack addresses (cm_policy_pack outputs); rebuilt when a member's pack
        buffer was (re)allocated, packing the members that have none yet."""
        if any(getattr(p, "_mfma", None) is None for p in self.policies):
            self.sync_weights()
        ptrs = tuple(p._mfma.data_ptr() for p in self.policies)
        if self._table is None or self._table[0] != ptrs:
            dev = self.policies[0]._mfma.device
            self._table = (ptrs, torch.tensor(ptrs, dtype=torch.int64).to(dev))
        return self._table[1]

    # the set forwards by kind: (entry point, its planner, the type of a member's record, the member's method that fills one, the
    # operand pack the kernel reads besides the flat weight copy)
    _FORWARDS = {
        "mlp": ("cm_mlp_policy_forward_multi", "cm_mlp_forward_multi_plan", L.MlpWeights, "_mlp_struct", "_mlp_pack"),
        "default": ("cm_policy_forward_multi", "cm_policy_forward_multi_plan", L.PolicyWeights, "_weights_struct", "_mfma"),
        "any": ("cm_policy_forward_any_multi", "cm_policy_forward_any_multi_plan", L.NetWeights, "_net_struct", None),
    }

    def _mlp_dims(self):
        """Obs-DP / CENT: the rows of the chain per env (one per agent, or the team's one), the actions and the agents."""
        p0 = self.policies[0]
        return (1 if p0._per_agent_rows else p0._n_agents, p0._action_dim, p0._n_agents)

    def forward_table(self, groups):
        """(device table, workgroup count) of the set forward - cm_policy_forward_multi (Comm-DP members of the default layer
        sizes), cm_policy_forward_any_multi (a PolicySet(any_sizes=True) of non-default Comm-DP nets: cm_policy_forward_any_multi_plan
        over every member's cm_net_weights; ``forward_lds`` is then the launch's LDS need) or cm_mlp_policy_forward_multi (Obs-DP /
        CENT members), every member's acting forward in one launch - with member k on the next groups[k] envs; (None, 0) when the
        library has no set kernel for the shape or the members have no operand pack.  Kept until a member's operand pack
        (``_mfma``, ``_mlp_pack``) or flat weight copy was reallocated or the groups change, packing the members that have no
        pack yet; the weights themselves are read as they are (sync_weights() refreshes them in place).  A set the planner refuses
        (a group without envs, ...) raises."""
        ps, kind = self.policies, self.forward_kind
        if kind is None:
            # a non-default member in a default set: cm_policy_forward_multi is built for the default layer sizes
            return None, 0
        if kind == "any" and any(p._default_shape for p in ps):
            # a default-sized member in an any-sizes set: its own forward is the f16-split cm_policy_forward, which the f32 set
            # kernel would not equal bit for bit
            return None, 0
        pack = self._FORWARDS[kind][4]
        if any(p._pack is None or (pack and getattr(p, pack) is None) for p in ps):
            self.sync_weights()
            if pack and any(getattr(p, pack) is None for p in ps):
                return None, 0                               # members without a pack
        groups = tuple(int(g) for g in groups)
        if len(groups) != len(ps):
            raise ValueError(f"forward_table: {len(groups)} groups for {len(ps)} policies")
        key = (groups, tuple((p._pack[0].data_ptr(), getattr(p, pack).data_ptr() if pack else None) for p in ps))
        if self._fwd_table is None or self._fwd_table[0] != key:
            self._fwd_table = (key,) + self._plan_forward(groups)
        return self._fwd_table[1], self._fwd_table[2]

    def _plan_forward(self, groups):
        """The planner protocol of the set's kind for `groups`: the table's size, the table into a host buffer of that size, its
        copy to the device -> (device table | None, workgroup count); sets ``forward_lds``."""
        ps, K = self.policies, len(self.policies)
        kind, p0 = self.forward_kind, ps[0]
        _, planner, record, struct, _ = self._FORWARDS[kind]
        self.forward_lds = 0
        members = [getattr(p, struct)() for p in ps]
        if any(w is None for w in members):
            return None, 0                                   # a member _net_struct() refuses: more layers than cm_policy_forward_any takes
        ws, sizes, n_wg, lds = (record * K)(*members), (C.c_int32 * K)(*groups), C.c_int32(0), C.c_size_t(0)
        shape = (K, sum(groups))                             # the planner's arguments between `sizes` and the buffer
        if kind == "mlp":
            shape += self._mlp_dims()
        outs = (C.byref(n_wg), C.byref(lds)) if kind == "any" else (C.byref(n_wg),)
        plan = getattr(L.lib(), planner)
        need = plan(ws, sizes, *shape, None, 0, *outs)
        # (the planner answering 0 - no set kernel for the shape: a team above 80 agents, a member above 160 KB of LDS - leaves no
        # table and n_wg = 0)
        table = None
        if need > 0:
            image = bytearray(need)
            need = plan(ws, sizes, *shape, (C.c_char * need).from_buffer(image), need, *outs)
            table = torch.frombuffer(image, dtype=torch.uint8).to(p0._pack[0].device)
        if need < 0:
            L.check(int(need), planner)
        if table is not None:
            self.forward_lds = lds.value
        return table, n_wg.value

    def forward_call(self, groups, B):
        """What the engine's launch of the set forward over B envs starts with: (entry point's name, [member 0's record - the
        shape every member shares; any sizes: the team, observation, hops and actions -, table, workgroup count, B, then what
        the kind's entry point takes besides: rows per env, actions, agents (Obs-DP / CENT) or forward_lds (any sizes)]); None
        where forward_table(groups) has no table."""
        table, n_wg = self.forward_table(groups)
        if table is None:
            return None
        kind, p0 = self.forward_kind, self.policies[0]
        what, _, _, struct, _ = self._FORWARDS[kind]
        lead = [C.byref(getattr(p0, struct)()), L.ptr(table), n_wg, B]
        if kind == "mlp":
            lead += self._mlp_dims()
        elif kind == "any":
            lead.append(self.forward_lds)
        return what, lead
