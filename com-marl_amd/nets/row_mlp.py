"""The Obs-DP / CENT variants: no communication, plain row-wise MLPs.  ``_RowMLPPolicy`` is the shared rollout
path - one fused HIP launch (cm_mlp_policy_forward, csrc/cm_mlp.hip) over a layer chain - under ``DecCategoricalMLPPolicy``,
``CentralizedCategoricalMLPPolicy`` and ``_HeadSampler`` (the Comm-DP head + sampler of teams too large for the one-launch
forward); ``GaussianMLPBaseline`` is their critic (cm_mlp_value_forward).

Reference: com_marl/torch/policies/dec_categorical_mlp_policy.py, centralized_categorical_mlp_policy.py,
com_marl/torch/baselines/gaussian_mlp_baseline.py.
"""
import ctypes as C
from collections import OrderedDict

import numpy as np
import torch
from torch import nn
from torch.distributions import Categorical, Normal

from .. import _lib as L
from .layers import ACT_NONE, ACT_TANH, ACT_RELU, hidden_act_code, MLPModule, GaussianMLPModule
from .pack import _as_dev, _WeightPack, _Acting


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
        return -Normal(mean, std, validate_args=False).log_prob(returns.reshape(-1, 1)).mean()      # (no host sync: see CommBaseCritic.compute_loss)
