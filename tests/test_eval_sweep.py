"""evaluate.eval_sweep: K checkpoints x C comm conditions scored in one rollout.  Cell (k, c) must hold exactly what
eval_summary returns for policy k on the uniform wrapper W_c (same class, seed and channel kind, params carrying condition c, E
envs at the same env_id_offset): all 12 numbers and the episode table, compared with ==."""
import numpy as np
import pytest

from tests import conditions_common as cc

pytestmark = pytest.mark.gpu

K, E, N_EPI, T, OFF = 2, 8, 12, 20, 5            # 12 episodes of 8 envs: a second round that takes 4
SHAPES = {
    "pp4": ("pp", cc.base_params("pp", 10, 1, 4, 4, max_env_steps=T), "IID",
            [dict(Rcom=9, pl=0), dict(Rcom=2, pl=0.3), dict(Rcom=1, pl=0.9)]),
    "co24": ("co", cc.base_params("co", 20, 2, 24, 0, max_env_steps=T), "GE",
             [dict(Rcom=3, Pgb=0.05, Pbg=0.3), dict(Rcom=6, Pgb=0.4, Pbg=0.1), dict(Rcom=19, Pgb=0.9, Pbg=0.9)]),
}


def _wrapper(scen, params, n_envs, channel, **kw):
    from com_marl_amd import envs as E_
    cls = E_.PredatorPreyWrapper if scen == "pp" else E_.CoverageWrapper
    return cls(True, params=params, n_envs=n_envs, device="cuda:0", seed=3, env_id_offset=OFF, channel=channel, **kw)


def _policies(env, n):
    import torch
    from com_marl_amd import nets
    out = []
    for k in range(n):
        torch.manual_seed(30 + k)
        p = nets.CommCategoricalMLPPolicy(env.spec, n_agents=env.n_agents, n_gcn_layers=env.GCNHops, device="cuda:0")
        p.set_rng(3)
        out.append(p)
    return out


def _same(a, b, what):
    import torch
    assert set(a) == set(b) | {"condition"}, what
    for key, v in b.items():
        if key == "episodes":
            assert tuple(a[key].shape) == (N_EPI, 9) and torch.equal(a[key], v), f"{what}: episodes"
        else:
            assert a[key] == v, f"{what}: {key}: {a[key]!r} != {v!r}"


@pytest.mark.parametrize("shape", list(SHAPES))
def test_cells_equal_eval_summary_on_uniform_wrappers(shape):
    from com_marl_amd.evaluate import eval_summary, eval_sweep, sweep_layout
    scen, params, channel, conds = SHAPES[shape]
    Cn = len(conds)
    env = _wrapper(scen, params, K * Cn * E, channel, conditions=conds)
    pols = _policies(env, K)
    got = eval_sweep(env, pols, 0, n_eval_episodes=N_EPI, max_env_steps=T, paired=True, episodes=True)
    assert len(got) == K and all(len(row) == Cn for row in got)
    assert env.eval_n_epi == N_EPI
    cond_of, ids = sweep_layout(K * Cn * E, K, Cn, OFF, True)
    np.testing.assert_array_equal(env.condition_of, cond_of)              # the call sets the layout itself and leaves it
    np.testing.assert_array_equal(env.batch.rng_ids, ids)
    for k in range(K):
        for c in range(Cn):
            assert got[k][c]["condition"] == conds[c]
            w = _wrapper(scen, cc.with_condition(params, conds[c]), E, channel)
            ref = eval_summary(w, pols[k], 0, n_eval_episodes=N_EPI, max_env_steps=T, episodes=True)
            _same(got[k][c], ref, f"policy {k}, condition {c}")
            assert env.last_eval_average_reward[k][c] == w.last_eval_average_reward
    # paired, greedy: the cells of one policy saw the same spawns and prey moves and differ only through the condition
    for k in range(K):
        assert any(got[k][0][key] != got[k][1][key] for key in ("reward", "success", "nodeDeg", "step_cnt"))
    # two calls on the same episodes (a fresh wrapper: an env's Philox step counter runs on across calls) give the same bits
    again = eval_sweep(_wrapper(scen, params, K * Cn * E, channel, conditions=conds), pols, 0, n_eval_episodes=N_EPI, max_env_steps=T, paired=True, episodes=True)
    for k in range(K):
        for c in range(Cn):
            _same(got[k][c], {key: v for key, v in again[k][c].items() if key != "condition"}, f"second call, cell {k},{c}")


def test_single_policy_unpaired_flag_and_refusals():
    from com_marl_amd.evaluate import eval_summary, eval_sweep
    scen, params, channel, conds = SHAPES["pp4"]
    Cn = len(conds)
    env = _wrapper(scen, params, Cn * E, channel, conditions=conds)
    pol = _policies(env, 1)[0]
    got = eval_sweep(env, pol, 0, n_eval_episodes=N_EPI, max_env_steps=T, paired=False)
    assert isinstance(got, list) and len(got) == Cn and isinstance(got[0], dict) and "episodes" not in got[0]
    assert isinstance(env.last_eval_average_reward, list) and len(env.last_eval_average_reward) == Cn
    np.testing.assert_array_equal(env.batch.rng_ids, OFF + np.arange(Cn * E))
    for c in range(Cn):                                                   # unpaired: the cell's own ids, W_c starts at its first env
        w = type(env)(True, params=cc.with_condition(params, conds[c]), n_envs=E, device="cuda:0", seed=3, env_id_offset=OFF + c * E,
                      channel=channel)
        _same(got[c], eval_summary(w, pol, 0, n_eval_episodes=N_EPI, max_env_steps=T), f"condition {c}")
        assert env.last_eval_average_reward[c] == w.last_eval_average_reward
    # flag[0] set: nothing runs
    assert eval_sweep(env, pol, 0, flag=[True]) == [None] * Cn
    assert eval_sweep(env, [pol, pol], 0, flag=[True]) == [[None] * Cn, [None] * Cn]
    # refusals
    with pytest.raises(ValueError, match="evenly"):
        eval_sweep(env, _policies(env, 5), 0, n_eval_episodes=4, max_env_steps=T)               # 24 envs, 5 x 3 cells
    with pytest.raises(ValueError, match="max_path_length"):
        eval_sweep(env, pol, 0, n_eval_episodes=4, max_env_steps=T + 1)
    with pytest.raises(ValueError, match="at least 1"):
        eval_sweep(env, pol, 0, n_eval_episodes=0, max_env_steps=T)
    plain = _wrapper(scen, params, Cn * E, channel)
    with pytest.raises(ValueError, match="without conditions"):
        eval_sweep(plain, pol, 0, n_eval_episodes=4, max_env_steps=T)
