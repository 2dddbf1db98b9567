"""The PPO update's full-batch evaluations with the row-MLP policies (Obs-DP: DecCategoricalMLPPolicy, CENT:
CentralizedCategoricalMLPPolicy): train_once runs three forwards per epoch and shares their outputs, where it once re-ran the old
policy after `load_state_dict`.  That is the same computation only if the old policy, once it holds the policy's weights, gives the
policy's own probabilities bit for bit (same kernel, same weights, weight pack refreshed) - pinned here, with the launch count."""
import numpy as np
import pytest

from tests.lib_spy import spy  # noqa: F401  (the fixture: a recording proxy around _lib.lib())
from tests.test_variants_parity import _algo, _variant_nets

N = 4
PARAMS = dict(load=2, capture_reward=10, step_cost=0.1, rm=0, penalty=0, grid_size=10, Rsen=1, n_agents=N, n_preys=N,
              n_gcn_layers=2, mode="train", trRcom=9, trpl=0)                       # PP map10


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need the MI355X")
    return torch


def _policy(kind, spec, hidden):
    from com_marl_amd import nets
    if kind == "obsdp":
        return nets.DecCategoricalMLPPolicy(spec, N, hidden_sizes=hidden, device="cuda:0")
    return nets.CentralizedCategoricalMLPPolicy(spec, n_agents=N, hidden_sizes=hidden, device="cuda:0")


# Obs-DP's hidden_sizes name three roles (encoder hidden, embedding, head hidden: dec_categorical_mlp_policy.py:77-79), so its
# net of width 8 is spelled [8, 8]; CENT's is [8]
@pytest.mark.gpu
@pytest.mark.parametrize("kind,hidden", [("obsdp", [8, 8]), ("cent", [8]), ("obsdp", [128, 64, 32]), ("cent", [128, 64, 32])])
def test_old_policy_after_load_is_the_policy_bit_for_bit(kind, hidden, torch_cuda):
    """P = 3 paths of T = 5 steps of PP map10 (the envs' own observations, the policy's own actions)."""
    torch = torch_cuda
    from com_marl_amd import envs, nets
    P, T = 3, 5
    env = envs.GridEnvBatch("pp", dict(PARAMS, max_env_steps=20), P, device="cuda:0", seed=3)
    spec = envs.EnvSpec(envs._Box(np.zeros(env.d * N), np.ones(env.d * N)), envs._Discrete(5))
    torch.manual_seed(11)
    pol = _policy(kind, spec, hidden)
    pol.set_rng(seed=3)
    algo = _algo(spec, pol, nets.GaussianMLPBaseline(env_spec=spec, hidden_sizes=(8,), device="cuda:0"), mpl=T)
    old = algo._old_policy
    env.reset_all()
    obs, actions = [], []
    for t in range(T):
        obs.append(env.obs.reshape(P, -1).clone())
        act, _, _ = pol.act_device(obs[-1], policy_step=t)
        actions.append(act.clone())
        env.step_device(act)
    obs, actions = torch.stack(obs, 1), torch.stack(actions, 1)               # [P,T,N*d], [P,T,N]
    _, p_stale = old.evaluate_nograd(obs)                                     # (the old policy's pack now holds ITS weights)
    with torch.no_grad():
        for w in pol.parameters():
            w.add_(0.05 * torch.randn_like(w))
    old.load_state_dict(pol.state_dict())
    lg, p_pol = pol.evaluate_nograd(obs, None, None)
    _, p_old = old.evaluate_nograd(obs)
    assert lg is None and tuple(p_pol.shape) == (P, T, N, 5)
    assert not torch.equal(p_stale, p_pol)                                    # the weights did move
    assert torch.equal(p_old, p_pol)
    _, p_act, _ = pol.act_device(obs.reshape(P * T, -1), want_actions=False, policy_step=0)
    assert torch.equal(p_act.reshape(P, T, N, 5), p_pol)
    assert torch.equal(algo._ll_from_probs(p_pol, actions), algo._old_log_likelihood(obs, actions, None, None))


@pytest.mark.gpu
def test_obsdp_epoch_runs_three_full_batch_forwards(torch_cuda, spy):  # noqa: F811
    """One train_once of the Obs-DP nets, one mini-epoch: old policy, policy before and policy after the update - three
    cm_mlp_policy_forward launches over the P * T * N rows of the batch, and no other launch of that kernel."""
    torch = torch_cuda
    from com_marl_amd import envs as E
    from com_marl_amd.sampler import CentralizedMAOnPolicyVectorizedSampler
    B, mpl, seed = 8, 6, 9
    env = E.PredatorPreyWrapper(centralized=True, params=dict(PARAMS, max_env_steps=mpl, seed=seed), n_envs=B, device="cuda:0")
    torch.manual_seed(seed)
    pol, crit = _variant_nets(torch, "obsdp", env.spec)
    pol.set_rng(seed)
    algo = _algo(env.spec, pol, crit, mpl=mpl)
    algo._optimization_mini_epochs = 1
    smp = CentralizedMAOnPolicyVectorizedSampler(algo, env, n_envs=B)
    smp.start_worker()
    paths = smp.obtain_samples(0, batch_size=B * N * mpl)
    first = len(spy.calls)
    algo.train_once(itr=0, paths=paths)
    rows = [c.args[1] for c in spy.calls[first:] if c == "cm_mlp_policy_forward"]
    assert rows == [len(paths) * algo.stats["MaxPathLength"] * N] * 3, rows
