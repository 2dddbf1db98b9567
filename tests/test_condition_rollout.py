"""Rollouts over a conditions batch: RolloutEngine with one policy or a PolicySet of 2 must play, in every (policy, condition)
cell, exactly what an engine over the uniform batch W_c plays (tests/conditions_common.py) - actions, probs and every env output
bit for bit - although the conditions batch steps in two launches and W_c may take the fused kernels; and the sampler + one
train_once run on such a wrapper."""
import numpy as np
import pytest

from tests import conditions_common as cc

pytestmark = pytest.mark.gpu

BUFS = ("obs", "actions", "probs", "attn", "reward", "reward64", "done", "details", "prey_alive", "success", "path_len",
        "dist_adj", "channels")
OFF = 7
# scenario, params, channel, conditions, E, steps
SHAPES = {
    "pp4": ("pp", cc.base_params("pp", 10, 1, 4, 4), "IID", [dict(Rcom=9, pl=0), dict(Rcom=1, pl=0.9)], 8, 8),
    "co24": ("co", cc.base_params("co", 20, 2, 24, 0), "GE", [dict(Rcom=3, Pgb=0.05, Pbg=0.3), dict(Rcom=19, Pgb=0.4, Pbg=0.1)], 2, 6),
}


def _policies(env, K):
    import torch
    from com_marl_amd import envs as E, nets
    spec = E.EnvSpec(E._Box(np.zeros(env.d * env.N), np.ones(env.d * env.N)), E._Discrete(5))
    out = []
    for k in range(K):
        torch.manual_seed(20 + k)
        p = nets.CommCategoricalMLPPolicy(spec, n_agents=env.N, n_gcn_layers=env.Lh, device="cuda:0")
        p.set_rng(3)
        out.append(p)
    return out


def _play(eng, H, greedy):
    import torch
    eng.policy.sync_weights()
    eng.reset()
    if not eng.steps_fused(0, H, greedy=greedy):
        eng.fork()
        for t in range(H):
            eng.step(t, greedy=greedy)
        eng.join()
    torch.cuda.synchronize()
    eng.env.check_status()
    return {k: getattr(eng, k).cpu().numpy() for k in BUFS if getattr(eng, k) is not None}


@pytest.mark.parametrize("K", [1, 2], ids=["one_policy", "policy_set"])
@pytest.mark.parametrize("greedy", [True, False], ids=["greedy_paired", "sampled_unpaired"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_cells_equal_engines_over_uniform_batches(shape, greedy, K):
    from com_marl_amd import nets
    from com_marl_amd.evaluate import sweep_layout
    from com_marl_amd.rollout import RolloutEngine
    scen, params, channel, conds, E, H = SHAPES[shape]
    Cn = len(conds)
    B = K * Cn * E
    paired = greedy                                   # sampled: the policy's draws are keyed by the physical env id
    cond_of, ids = sweep_layout(B, K, Cn, OFF, paired)
    env = cc.make_batch(scen, params, B, OFF, channel, conditions=conds, condition_of=cond_of, rng_ids=ids)
    pols = _policies(env, K)
    if K == 1:
        eng = RolloutEngine(env, pols[0], H)
    else:
        eng = RolloutEngine(env, nets.PolicySet(pols), H, groups=[Cn * E] * K)
    got = _play(eng, H, greedy)
    assert eng.dist_adj is not None and eng.channels is not None
    if K == 1:
        assert eng._fused is False                    # the fused entry points declined; two launches per step
    else:
        assert eng.multi_form == "loop"
    assert got["done"].any(0).all(), "every env must auto-reset at least once"
    full = [c["Rcom"] + 1 >= params["grid_size"] for c in conds]
    differs = []
    for k in range(K):
        for c in range(Cn):
            lo = (k * Cn + c) * E
            hi = lo + E
            w = cc.uniform_batch(scen, params, conds[c], E, OFF if paired else OFF + lo, channel)
            ref = _play(RolloutEngine(w, pols[k], H), H, greedy)
            assert ("dist_adj" in ref) == (not full[c])
            for name in got:
                if name == "dist_adj" and full[c]:
                    assert (got[name][:, lo:hi] == 1).all()
                    continue
                np.testing.assert_array_equal(got[name][:, lo:hi], ref[name], err_msg=f"policy {k}, condition {c}, {name}")
            # control: the neighbouring condition's cell of the same policy is something else
            lo2 = (k * Cn + (c + 1) % Cn) * E
            differs.append(any(not np.array_equal(got[n][:, lo2:lo2 + E], ref[n]) for n in ref))
    assert all(differs)


def test_sampler_and_train_once_run_on_two_conditions():
    import torch
    from com_marl_amd import envs as E, nets
    from com_marl_amd.algos import CentralizedMAPPO
    from com_marl_amd.sampler import CentralizedMAOnPolicyVectorizedSampler
    params = cc.base_params("pp", 10, 1, 4, 4, max_env_steps=6, mode="train", trRcom=9, trpl=0.0, seed=5)
    conds = [dict(Rcom=9, pl=0.0), dict(Rcom=1, pl=0.5)]              # the mix a packet-loss curriculum trains on
    B, N, mpl = 32, 4, 6
    env = E.PredatorPreyWrapper(centralized=True, params=params, n_envs=B, device="cuda:0", conditions=conds)
    assert env.conditions == conds and env.channelType == "IID"
    np.testing.assert_array_equal(env.condition_of, np.repeat([0, 1], 16))
    torch.manual_seed(5)
    pol = nets.CommCategoricalMLPPolicy(env.spec, n_agents=N, device="cuda:0")
    crit = nets.CommBaseCritic(env.spec, n_agents=N, device="cuda:0")
    pol.set_rng(5)
    algo = CentralizedMAPPO(env_spec=env.spec, policy=pol, baseline=crit, max_path_length=mpl, discount=0.99, center_adv=True,
                            positive_adv=False, gae_lambda=0.97, policy_ent_coeff=0.1, entropy_method='regularized',
                            stop_entropy_gradient=False, clip_grad_norm=7, optimization_n_minibatches=3, optimization_mini_epochs=2,
                            device="cuda:0")
    smp = CentralizedMAOnPolicyVectorizedSampler(algo, env, n_envs=B)
    smp.start_worker()
    paths = smp.obtain_samples(0, batch_size=B * N * mpl + 3)
    assert len(paths) >= B
    env_idx = paths.env_idx.cpu().numpy()
    seen = set()
    for i in range(len(paths)):
        p = paths[i]
        c = int(env.condition_of[env_idx[i]])
        seen.add(c)
        n = len(p["rewards"])
        adj = p["dist_adjs"].reshape(n, N, N)
        if c == 0:
            assert (adj == 1).all()                                   # Rcom 9 on map 10: fully connected
        else:                                                         # Rcom 1: recomputed from the positions in the observation
            obs = p["observations"].reshape(n, N, -1)
            d = obs.shape[-1]
            row, col = np.rint(obs[:, :, d - 3] * 10).astype(int), np.rint(obs[:, :, d - 2] * 9).astype(int)
            dr, dc = row[:, :, None] - row[:, None, :], col[:, :, None] - col[:, None, :]
            np.testing.assert_array_equal(adj, (dr * dr + dc * dc <= 2).astype(np.float32), err_msg=f"path {i}")
            ch = p["channels"].reshape(n, -1, N, N)
            assert ((ch == 0) | (ch == 1)).all() and (ch[:, :, np.arange(N), np.arange(N)] == 1).all()
    assert seen == {0, 1}
    lossy = np.concatenate([paths[i]["channels"].reshape(-1, N, N) for i in range(len(paths)) if env.condition_of[env_idx[i]] == 1])
    clean = np.concatenate([paths[i]["channels"].reshape(-1, N, N) for i in range(len(paths)) if env.condition_of[env_idx[i]] == 0])
    assert (clean == 1).all() and 0.3 < cc.offdiag_mean(lossy) < 0.7
    before = [q.detach().clone() for q in pol.parameters()]
    algo.train_once(itr=0, paths=paths)
    flat = torch.cat([q.detach().flatten() for q in pol.parameters()])
    assert torch.isfinite(flat).all() and any(not torch.equal(a, b) for a, b in zip(before, pol.parameters()))
    for k in ("LossBefore", "LossAfter", "KL", "Entropy", "GradNorm", "AverageReturn"):
        assert np.isfinite(algo.stats[k]), (k, algo.stats[k])
