"""Dense building blocks with the reference's state_dict names, and their autograd functions: the MLP of every encoder and head
(``MLPModule``, ``GaussianMLPModule``), ``hip_linear`` / ``HipLinear`` (nn.Linear + activation as the one-pass kernel pair
cm_linear_act_forward / _backward of csrc/cm_linear.hip under autograd, the weight gradient on cm_linear_wgrad otherwise),
``_MatmulWFn`` for the hops' H.W, the activation codes ``ACT_*`` with ``hidden_act_code``, and the critic's Gaussian NLL in one
launch each way (``_GaussNLLFn``, cm_gauss_nll_*).

Reference: garage/torch/modules/multi_headed_mlp_module.py, com_marl/torch/modules/mlp_encoder_module.py,
categorical_mlp_module.py, gaussian_mlp_module.py.
"""
import math
from collections import OrderedDict

import torch
from torch import nn

from .. import _lib as L


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
