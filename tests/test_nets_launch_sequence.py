"""Which C entry points each route of com_marl_amd.nets launches, in order, at the smallest shape that still takes the route: a
characterisation of the host path between a net's method and the library.  The literals of _PARENT are what the commit BEFORE
nets.py became a package printed for these test bodies on the MI355X, pasted (the print-out is kept as
profiles/nets_launch_sequence_parent.txt): they do not come from the code under test.  Every name is reached through the façade (com_marl_amd.nets), the calls are recorded by the stand-in of tests/lib_spy.py, and a
route's outputs are checked to be finite - the parity tests judge the values."""
import pytest

from tests import any_shapes as G
from tests.lib_spy import spy  # noqa: F401  (the fixture: a recording proxy around _lib.lib())

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, D, HOPS = 4, 21, 2                       # PP map 10: teams of 4, 21 features per agent, the runners' two hops

_PARENT = {'default/act_device': ['cm_multi_copy_t', 'cm_policy_pack_bytes', 'cm_policy_pack_sections', 'cm_policy_forward'],
 'default/evaluate_nograd': ['cm_policy_forward_saved'],
 'default/log_likelihood.backward': ['cm_policy_forward_saved', 'cm_linear_act_backward', 'cm_linear_act_backward',
                                     'cm_linear_act_backward', 'cm_linear_act_backward', 'cm_masked_agg_backward_r',
                                     'cm_linear_act_backward', 'cm_masked_agg_backward_r', 'cm_linear_act_backward',
                                     'cm_attention_backward', 'cm_linear_act_backward', 'cm_encoder_backward'],
 'default/critic.values_device': ['cm_multi_copy_t', 'cm_critic_pack_bytes', 'cm_critic_pack_sections', 'cm_critic_forward'],
 'default/critic.compute_loss.backward': ['cm_critic_forward_saved', 'cm_gauss_nll_forward', 'cm_gauss_nll_backward',
                                          'cm_linear_act_backward', 'cm_linear_act_backward', 'cm_masked_agg_backward_r',
                                          'cm_linear_act_backward', 'cm_masked_agg_backward_r', 'cm_linear_act_backward',
                                          'cm_attention_backward', 'cm_linear_act_backward', 'cm_encoder_backward'],
 'A/act_device': ['cm_multi_copy_t', 'cm_policy_forward_any'],
 'A/log_likelihood.backward': ['cm_linear_act_forward', 'cm_linear_act_forward', 'cm_linear_act_forward',
                               'cm_linear_act_forward', 'cm_attention_forward_any', 'cm_linear_act_forward',
                               'cm_masked_agg_forward_any', 'cm_linear_act_forward', 'cm_masked_agg_forward_any',
                               'cm_linear_act_forward', 'cm_linear_act_forward', 'cm_linear_act_forward',
                               'cm_linear_act_backward', 'cm_linear_act_backward', 'cm_linear_act_backward',
                               'cm_masked_agg_backward_any', 'cm_linear_act_backward', 'cm_masked_agg_backward_any',
                               'cm_linear_act_backward', 'cm_attention_backward_any', 'cm_linear_act_backward',
                               'cm_linear_act_backward', 'cm_linear_act_backward', 'cm_linear_act_backward'],
 'dec/act_device': ['cm_multi_copy_t', 'cm_mlp_pack_bytes', 'cm_mlp_pack', 'cm_mlp_policy_forward'],
 'cent/act_device': ['cm_multi_copy_t', 'cm_mlp_pack_bytes', 'cm_mlp_pack', 'cm_mlp_policy_forward'],
 'baseline/values_device': ['cm_multi_copy_t', 'cm_mlp_pack_bytes', 'cm_mlp_pack', 'cm_mlp_value_forward'],
 'baseline/compute_loss.backward': ['cm_linear_act_forward', 'cm_linear_act_forward', 'cm_linear_act_forward',
                                    'cm_linear_act_backward', 'cm_linear_act_backward', 'cm_linear_act_backward'],
 'layers/act_device': ['cm_attention_forward', 'cm_masked_agg_forward', 'cm_masked_agg_forward', 'cm_multi_copy_t',
                       'cm_mlp_pack_bytes', 'cm_mlp_pack', 'cm_mlp_policy_forward'],
 'set/N8/forward_call': ['cm_multi_copy_t', 'cm_policy_pack_bytes', 'cm_policy_pack_sections', 'cm_multi_copy_t',
                         'cm_policy_pack_bytes', 'cm_policy_pack_sections', 'cm_policy_forward_multi_plan',
                         'cm_policy_forward_multi_plan'],
 'set/N8/entry_point': 'cm_policy_forward_multi',
 'set/N4/forward_call': ['cm_multi_copy_t', 'cm_policy_pack_bytes', 'cm_policy_pack_sections', 'cm_multi_copy_t',
                         'cm_policy_pack_bytes', 'cm_policy_pack_sections', 'cm_policy_forward_multi_plan'],
 'set/N4/entry_point': None}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need the MI355X")
    return torch


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    """The launch choices that read a switch read its default."""
    import com_marl_amd
    monkeypatch.setattr(com_marl_amd, "_deterministic", False)
    for knob in ("COMMARL_POLICY_KERNEL", "COMMARL_FUSED_TRAIN", "COMMARL_TRAIN_FWD_WAVE_MIN"):
        monkeypatch.delenv(knob, raising=False)


class _Routes:
    """Runs one route at a time with the recorder emptied before it, keeps and prints its calls, checks its outputs."""

    def __init__(self, torch, spy):
        self.torch, self.spy, self.seen = torch, spy, {}

    def run(self, label, fn, grads_of=None):
        del self.spy.calls[:]
        out = fn()
        self.torch.cuda.synchronize()
        self.seen[label] = [str(c) for c in self.spy.calls]
        print(f"\n    {label!r}: {self.seen[label]},")
        outs = [t for t in (out if isinstance(out, (tuple, list)) else (out,)) if self.torch.is_tensor(t)]
        if grads_of is not None:
            grads = [p.grad for p in grads_of.parameters()]
            assert all(g is not None for g in grads), label
            outs += grads
        for t in outs:
            assert bool(self.torch.isfinite(t.float()).all()), label
        return out

    def check(self):
        assert self.seen == {k: _PARENT.get(k) for k in self.seen}


def _pp_map10(torch, S):
    """S reset envs of PP map 10 -> obs [S,N*d], dist_adj [S,N,N], channels [S,hops,N,N] and the env spec."""
    from com_marl_amd import envs
    params = dict(load=2, max_env_steps=20, capture_reward=10, step_cost=0.1, rm=0, penalty=0, grid_size=10, Rsen=1,
                  n_agents=N, n_preys=N, n_gcn_layers=HOPS, mode="train", trRcom=9, trpl=0)
    env = envs.GridEnvBatch("pp", params, S, device=DEV, seed=3)
    env.reset_all()
    assert env.d == D
    return env.obs.reshape(S, -1).clone(), env.dist_adj.clone(), env.channels.clone(), G.spec_of(N, D)


def test_comm_default_sizes(torch_cuda, spy):  # noqa: F811
    torch = torch_cuda
    from com_marl_amd import nets
    S = 2
    obs, adj, ch, spec = _pp_map10(torch, S)
    torch.manual_seed(0)
    pol = nets.CommCategoricalMLPPolicy(spec, n_agents=N, device=DEV)
    crit = nets.CommBaseCritic(spec, n_agents=N, device=DEV)
    pol.set_rng(seed=3)
    r = _Routes(torch, spy)
    act, _, _ = r.run("default/act_device", lambda: pol.act_device(obs, None, adj, ch, policy_step=0))
    r.run("default/evaluate_nograd", lambda: pol.evaluate_nograd(obs, adj, ch))
    r.run("default/log_likelihood.backward", lambda: pol.log_likelihood(obs, None, adj, ch, act).sum().backward(), grads_of=pol)
    r.run("default/critic.values_device", lambda: crit.values_device(obs, adj, ch))
    returns = torch.linspace(-1.0, 1.0, S, device=DEV)
    r.run("default/critic.compute_loss.backward", lambda: crit.compute_loss(obs, returns, adj, ch).backward(), grads_of=crit)
    r.check()


def test_comm_shape_a(torch_cuda, spy):  # noqa: F811
    """Non-default layer sizes (shape A of tests/any_shapes.py): the one-launch acting forward, and forward + backward on the
    per-layer autograd path with the any-width graph ops."""
    torch = torch_cuda
    S = 2
    pol, _ = G.build("A", critic=False)
    pol.set_rng(seed=3)
    obs, avail, adj, ch = (torch.as_tensor(a, device=DEV) for a in G.inputs(N, D, HOPS, S=S))
    r = _Routes(torch, spy)
    act, _, _ = r.run("A/act_device", lambda: pol.act_device(obs, avail, adj, ch, policy_step=0))
    r.run("A/log_likelihood.backward", lambda: pol.log_likelihood(obs, avail, adj, ch, act).sum().backward(), grads_of=pol)
    r.check()


def test_comm_layer_by_layer(torch_cuda, spy):  # noqa: F811
    """A team above MAX_FUSED_AGENTS: the acting forward runs layer by layer (_act_device_layers)."""
    torch = torch_cuda
    from com_marl_amd import nets
    n, S = 96, 1
    assert nets.MAX_FUSED_AGENTS < n <= nets.MAX_KERNEL_AGENTS
    torch.manual_seed(0)
    pol = nets.CommCategoricalMLPPolicy(G.spec_of(n, D), n_agents=n, device=DEV)
    pol.set_rng(seed=3)
    obs, avail, adj, ch = (torch.as_tensor(a[:S], device=DEV) for a in G.inputs(n, D, HOPS, S=2))
    r = _Routes(torch, spy)
    r.run("layers/act_device", lambda: pol.act_device(obs, avail, adj, ch, policy_step=0))
    r.check()


def test_row_mlp_nets(torch_cuda, spy):  # noqa: F811
    torch = torch_cuda
    from com_marl_amd import nets
    S = 2
    spec = G.spec_of(N, D)
    torch.manual_seed(0)
    dec = nets.DecCategoricalMLPPolicy(spec, N, device=DEV)
    cent = nets.CentralizedCategoricalMLPPolicy(spec, n_agents=N, device=DEV)
    base = nets.GaussianMLPBaseline(env_spec=spec, device=DEV)
    obs = torch.as_tensor(G.inputs(N, D, HOPS, S=S)[0], device=DEV)
    r = _Routes(torch, spy)
    for name, pol in (("dec", dec), ("cent", cent)):
        pol.set_rng(seed=3)
        r.run(name + "/act_device", lambda: pol.act_device(obs, policy_step=0))
    r.run("baseline/values_device", lambda: base.values_device(obs))
    returns = torch.linspace(-1.0, 1.0, S, device=DEV)
    r.run("baseline/compute_loss.backward", lambda: base.compute_loss(obs, returns).backward(), grads_of=base)
    r.check()


def test_policy_set_forward_call(torch_cuda, spy):  # noqa: F811
    """Two default-size Comm-DP policies on two groups of 16 envs: what one forward_call (packs, planner, table) launches, and the
    entry point it names - for teams of 8, the smallest the set forward is built for, and for teams of 4, which the planner refuses
    (their set runs in the wave-owned rollout)."""
    torch = torch_cuda
    from com_marl_amd import nets
    r = _Routes(torch, spy)
    for n in (8, 4):
        torch.manual_seed(0)
        ps = nets.PolicySet([nets.CommCategoricalMLPPolicy(G.spec_of(n, D), n_agents=n, device=DEV) for _ in range(2)])
        call = r.run(f"set/N{n}/forward_call", lambda: ps.forward_call([16, 16], 32))
        r.seen[f"set/N{n}/entry_point"] = None if call is None else call[0]
        print(f"    'set/N{n}/entry_point': {r.seen[f'set/N{n}/entry_point']!r},")
        if call is not None:
            assert ps.forward_table([16, 16])[0].numel() > 0
    r.check()
