"""Comm-DP policy and critic: same classes, ctor kwargs, parameter names and numerics as the
reference, two execution paths:

  * rollout / no-grad : ONE fused HIP launch per batch of env states through the C ABI
    (``cm_policy_forward`` / ``cm_critic_forward``, csrc/cm_policy.hip);
  * PPO update (autograd): dense per-agent GEMMs on PyTorch-ROCm (rocBLAS / MFMA), the
    adjacency-masked aggregation as the custom HIP op ``masked_aggregate``
    (``cm_masked_agg_forward/backward``, csrc/cm_graph_ops.hip).

A package of role modules, each importing only from those before it: layers -> graph -> pack -> comm -> row_mlp ->
comm_policy, comm_critic -> policy_set ("nets as a package").  This module is the one name callers import: every
module-level name of the role modules is bound here, explicitly, as a real attribute (tests patch them here; a patch that must
reach a caller inside the package goes on the role module that caller lives in).
"""
from .layers import (_Tanh, _ReLU, ACT_NONE, ACT_TANH, ACT_RELU, hidden_act_code, MLPModule, _wgrad, _linear_act_backward,  # noqa: F401
    _LinearFn, _MatmulWFn, _LinearActFn, _fused_ok, hip_linear, HipLinear, GaussianMLPModule, _GaussNLLFn)
from .graph import (MAX_KERNEL_AGENTS, _NotCovered, _GRAPH_ROUTE, graph_op_route, set_graph_op_route, _graph_forward,  # noqa: F401
    _hop_channels, _AttentionSoftmax, AttentionModule, GraphConvolutionModule, _MaskedAggregate, masked_aggregate)
from .pack import _as_dev, _Stacked, _WeightPack, _Acting  # noqa: F401
from .comm import (MAX_FUSED_AGENTS, MAX_FUSED_OBS, _ZeroPool, _lin_bwd, _fused_shape_ok, _fused_train_ok, _fwd_wave_ok,  # noqa: F401
    _forward_saved, _FusedNetFn, _fused_logits_nograd, CommBaseNet)
from .row_mlp import (_RowMLPPolicy, _HeadSampler, DecCategoricalMLPPolicy, CentralizedCategoricalMLPPolicy,  # noqa: F401
    GaussianMLPBaseline)
from .comm_policy import CommCategoricalMLPPolicy  # noqa: F401
from .comm_critic import CommBaseCritic  # noqa: F401
from .policy_set import _architecture, _ANY_SIZES_FREE, _differences, PolicySet  # noqa: F401
