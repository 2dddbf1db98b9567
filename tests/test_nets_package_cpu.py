"""com_marl_amd.nets as a package of role modules (no GPU): the façade binds every module-level name nets.py defined, each once;
the role modules import only from the ones before them; class references pickled under the old path still resolve; the
parameter names did not move.  The literals were printed at the commit before the split."""
import ast
import os
import pickle
import sys

import pytest

from tests import any_shapes as G

# every module-level name of nets.py at the commit before the split (ast over its top-level def / class / assignment nodes)
NAMES = (
    'MAX_KERNEL_AGENTS', 'MAX_FUSED_AGENTS', 'MAX_FUSED_OBS', '_Tanh', '_ReLU', 'ACT_NONE', 'ACT_TANH', 'ACT_RELU',
    'hidden_act_code', 'MLPModule', '_NotCovered', '_GRAPH_ROUTE', 'graph_op_route', 'set_graph_op_route', '_graph_forward',
    '_hop_channels', '_AttentionSoftmax', 'AttentionModule', 'GraphConvolutionModule', '_wgrad', '_linear_act_backward',
    '_LinearFn', '_MatmulWFn', '_LinearActFn', '_fused_ok', 'hip_linear', 'HipLinear', '_MaskedAggregate', 'masked_aggregate',
    '_ZeroPool', '_lin_bwd', '_fused_shape_ok', '_fused_train_ok', '_fwd_wave_ok', '_forward_saved', '_FusedNetFn',
    '_fused_logits_nograd', '_as_dev', '_Stacked', '_WeightPack', 'CommBaseNet', '_Acting', 'CommCategoricalMLPPolicy',
    'GaussianMLPModule', '_GaussNLLFn', 'CommBaseCritic', '_RowMLPPolicy', '_HeadSampler', 'DecCategoricalMLPPolicy',
    'CentralizedCategoricalMLPPolicy', 'GaussianMLPBaseline', '_architecture', '_ANY_SIZES_FREE', '_differences', 'PolicySet')

# the role modules in import order: a module imports only from those before it (comm_policy and comm_critic are siblings)
ORDER = ("layers", "graph", "pack", "comm", "row_mlp", "comm_policy", "comm_critic", "policy_set")
SIBLINGS = {"comm_critic": "comm_policy"}

PICKLED = ("CommCategoricalMLPPolicy", "CommBaseCritic", "DecCategoricalMLPPolicy", "CentralizedCategoricalMLPPolicy",
           "GaussianMLPBaseline", "PolicySet")

_TRUNK = ('encoder._layers.0.linear.weight', 'encoder._layers.0.linear.bias', 'encoder._output_layers.0.linear.weight',
          'encoder._output_layers.0.linear.bias', 'attention_layer.linear_in.weight', 'gcn_layers.0.weight', 'gcn_layers.0.bias',
          'gcn_layers.1.weight', 'gcn_layers.1.bias')
STATE_KEYS = {
    "CommCategoricalMLPPolicy": _TRUNK + (
        'categorical_output_layer._layers.0.linear.weight', 'categorical_output_layer._layers.0.linear.bias',
        'categorical_output_layer._layers.1.linear.weight', 'categorical_output_layer._layers.1.linear.bias',
        'categorical_output_layer._layers.2.linear.weight', 'categorical_output_layer._layers.2.linear.bias',
        'categorical_output_layer._output_layers.0.linear.weight', 'categorical_output_layer._output_layers.0.linear.bias'),
    "CommBaseCritic": _TRUNK + (
        'baseline_aggregator._init_std', 'baseline_aggregator._mean_module._layers.0.linear.weight',
        'baseline_aggregator._mean_module._layers.0.linear.bias', 'baseline_aggregator._mean_module._output_layers.0.linear.weight',
        'baseline_aggregator._mean_module._output_layers.0.linear.bias'),
    "DecCategoricalMLPPolicy": (
        '_layers.0.linear.weight', '_layers.0.linear.bias', '_output_layers.0.linear.weight', '_output_layers.0.linear.bias',
        'encoder._layers.0.linear.weight', 'encoder._layers.0.linear.bias', 'encoder._output_layers.0.linear.weight',
        'encoder._output_layers.0.linear.bias'),
    "CentralizedCategoricalMLPPolicy": (
        '_layers.0.linear.weight', '_layers.0.linear.bias', '_layers.1.linear.weight', '_layers.1.linear.bias',
        '_output_layers.0.linear.weight', '_output_layers.0.linear.bias'),
    "GaussianMLPBaseline": (
        'module._init_std', 'module._mean_module._layers.0.linear.weight', 'module._mean_module._layers.0.linear.bias',
        'module._mean_module._layers.1.linear.weight', 'module._mean_module._layers.1.linear.bias',
        'module._mean_module._output_layers.0.linear.weight', 'module._mean_module._output_layers.0.linear.bias'),
}


@pytest.fixture(scope="module")
def nets():
    from com_marl_amd import nets
    return nets


def test_surface_is_every_old_name_once(nets):
    roles = {f"{nets.__name__}.{m}" for m in ORDER}
    assert len(set(NAMES)) == len(NAMES) == 55
    homes = {}
    for name in NAMES:
        assert name in vars(nets), f"nets.{name} is not an attribute of the façade"
        obj = getattr(nets, name)
        if isinstance(obj, type) or callable(obj):
            assert obj.__module__ in roles, (name, obj.__module__)
            assert getattr(sys.modules[obj.__module__], name) is obj, f"{name}: the façade holds a copy"
            homes[name] = obj.__module__
        else:                                                   # constants and the route table: one role module binds the object
            owners = [m for m in sorted(roles) if name in vars(sys.modules[m]) and _defines(sys.modules[m], name)]
            assert len(owners) == 1 and getattr(sys.modules[owners[0]], name) is obj, (name, owners)
    # the two objects with module-level state are single objects: the route table, and the class whose attributes the packs default to
    assert nets._GRAPH_ROUTE is sys.modules[f"{nets.__name__}.graph"]._GRAPH_ROUTE
    assert homes["_WeightPack"] == f"{nets.__name__}.pack"


def _tree(module):
    with open(module.__file__) as f:
        return ast.parse(f.read())


def _defines(module, name):
    """Whether `module`'s own text assigns `name` at its top level (and does not merely import it)."""
    for node in _tree(module).body:
        if isinstance(node, ast.Assign):
            for t in node.targets:
                if name in [e.id for e in (t.elts if isinstance(t, ast.Tuple) else [t])]:
                    return True
    return False


def test_role_modules_import_only_from_those_before(nets):
    pkg_dir = os.path.dirname(nets.__file__)
    assert sorted(f[:-3] for f in os.listdir(pkg_dir) if f.endswith(".py")) == sorted(ORDER + ("__init__",))
    for i, m in enumerate(ORDER):
        allowed = set(ORDER[:i]) - {SIBLINGS.get(m)}
        with open(os.path.join(pkg_dir, m + ".py")) as f:
            tree = ast.parse(f.read())
        assert ast.get_docstring(tree), f"{m}: no module docstring"
        for node in ast.walk(tree):
            if isinstance(node, ast.Import):
                assert not any(a.name.startswith("com_marl_amd") for a in node.names), (m, ast.dump(node))
            if not isinstance(node, ast.ImportFrom):
                continue
            if node.level == 0:
                assert not (node.module or "").startswith("com_marl_amd"), (m, node.module)
                continue
            assert node in tree.body, f"{m}: import inside a function"
            if node.level == 2:                                 # the parent package: _lib and deterministic only
                assert node.module is None and {a.name for a in node.names} <= {"_lib", "deterministic"}, (m, ast.dump(node))
            else:           # a role module named outright: `from . import x` would be the façade's namespace, and attribute hops
                assert node.level == 1 and node.module in allowed, f"{m} imports from {node.module!r}"


@pytest.mark.parametrize("name", PICKLED)
def test_class_references_pickled_under_the_old_path_resolve(name, nets):
    cls = getattr(nets, name)
    assert pickle.loads(f"ccom_marl_amd.nets\n{name}\n.".encode()) is cls        # protocol 0, global opcode: the old path
    for protocol in (0, pickle.HIGHEST_PROTOCOL):
        assert pickle.loads(pickle.dumps(cls, protocol)) is cls


def test_state_dict_keys_are_the_old_ones(nets):
    spec = G.spec_of(4, 21)
    built = {
        "CommCategoricalMLPPolicy": nets.CommCategoricalMLPPolicy(spec, n_agents=4),
        "CommBaseCritic": nets.CommBaseCritic(spec, n_agents=4),
        "DecCategoricalMLPPolicy": nets.DecCategoricalMLPPolicy(spec, 4),
        "CentralizedCategoricalMLPPolicy": nets.CentralizedCategoricalMLPPolicy(spec, n_agents=4),
        "GaussianMLPBaseline": nets.GaussianMLPBaseline(env_spec=spec),
    }
    for name, net in built.items():
        assert tuple(net.state_dict().keys()) == STATE_KEYS[name], name
