"""The Comm-DP trunk (``CommBaseNet``: encoder, attention, L graph-convolution hops; its weight pack for the fused kernels and
the route of nets with non-default layer sizes), and its whole-network training forward (teams up to MAX_FUSED_AGENTS):
``_FusedNetFn`` is ONE fused launch that stores what the backward needs (cm_policy_forward_saved / cm_critic_forward_saved)
and a hand-written backward chain over the C-ABI kernels - no per-layer forward kernels, no gradient-accumulation adds from
autograd; ``_fused_logits_nograd`` is the same kernel storing the logits only.  ``_fused_shape_ok`` / ``_fused_train_ok`` /
``_fwd_wave_ok`` say which shapes and batches take which kernel.

Reference: com_marl/torch/modules/comm_base_net.py.
"""
import ctypes as C
import os
from collections import OrderedDict

import numpy as np
import torch
from torch import nn

from .. import _lib as L
from .. import deterministic as _det
from .layers import MLPModule, _linear_act_backward, _MatmulWFn, _LinearActFn, _fused_ok
from .graph import _hop_channels, AttentionModule, GraphConvolutionModule, masked_aggregate
from .pack import _Stacked, _WeightPack


# team size up to which the one-launch forward (rollout and training) holds one env's planes in LDS (cm_policy_h_dev.h LDS map)
MAX_FUSED_AGENTS = 80
MAX_FUSED_OBS = 80           # per-agent observation size up to which the matrix-core pack, hence the training forward, exists


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
