"""The Comm-DP critic (``CommBaseCritic``, aggregators 'sum' and 'direct'): the no-grad forward ``values_device`` (one launch of
cm_critic_forward, or cm_critic_forward_any for other layer sizes) and ``compute_loss``, the Gaussian NLL over the fused training
forward.

Reference: com_marl/torch/baselines/comm_base_critic.py.
"""
import ctypes as C
from collections import OrderedDict

import torch
from torch.distributions import Normal

from .. import _lib as L
from .layers import GaussianMLPModule, _GaussNLLFn
from .pack import _as_dev
from .comm import MAX_FUSED_AGENTS, _fused_train_ok, _FusedNetFn, CommBaseNet


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
