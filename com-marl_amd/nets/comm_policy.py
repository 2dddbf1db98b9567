"""The Comm-DP policy (``CommCategoricalMLPPolicy``): the autograd path of the PPO update (``forward``, ``log_likelihood``,
``entropy``, ``evaluate_nograd``), the acting forward ``act_device`` - one launch of cm_policy_forward (csrc/cm_policy.hip), of
cm_policy_forward_any for other layer sizes, or layer by layer for teams above MAX_FUSED_AGENTS - and the fused rollout calls
``step_fused`` / ``chunk_fused`` (cm_rollout_*).

Reference: com_marl/torch/policies/comm_categorical_mlp_policy.py.
"""
import ctypes as C
from collections import OrderedDict

import numpy as np
import torch
from torch.distributions import Categorical

from .. import _lib as L
from .layers import MLPModule
from .pack import _as_dev, _Acting
from .comm import MAX_FUSED_AGENTS, _fused_shape_ok, _fused_train_ok, _FusedNetFn, _fused_logits_nograd, CommBaseNet
from .row_mlp import _HeadSampler


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
