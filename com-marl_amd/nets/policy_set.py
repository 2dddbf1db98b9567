"""Policy sets: several policies of one architecture in one rollout (``PolicySet``), the architecture check behind it
(``_architecture``, ``_differences``) and the launch planner of the set forwards (``forward_table``, ``forward_call``:
cm_policy_forward_multi, cm_policy_forward_any_multi, cm_mlp_policy_forward_multi).  No counterpart in the reference, which
evaluates one checkpoint at a time.
"""
import ctypes as C

import torch

from .. import _lib as L
from .layers import ACT_TANH
from .comm import CommBaseNet


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
