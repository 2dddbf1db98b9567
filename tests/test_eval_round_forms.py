"""Which form the rounds of each evaluation entry point take: eval_model and eval_summary with a single policy step one by one
and never ask for the chunk launch, eval_models and eval_summary with several policies play a round as one chunk launch, and
eval_sweep asks for the chunk with a single policy too (a conditions wrapper without fused_conditions declines it).  Counted on a
spy engine; every call plays two rounds, the second ragged."""
import pytest

from tests import conditions_common as cc

pytestmark = pytest.mark.gpu

T, B = 6, 32
PARAMS = cc.base_params("pp", 10, 1, 4, 4, max_env_steps=T)
CONDS = [dict(Rcom=9, pl=0), dict(Rcom=2, pl=0.3)]


def _wrapper(**kw):
    from com_marl_amd import envs as E
    return E.PredatorPreyWrapper(True, params=PARAMS, n_envs=B, device="cuda:0", seed=3, **kw)


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


@pytest.fixture
def spy(monkeypatch):
    """-> the list of engines the evaluation built, each with `fused` (the steps_fused answers), `steps` and `resets`."""
    from com_marl_amd import evaluate
    used = []

    class Spy(evaluate.RolloutEngine):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.fused, self.steps, self.resets = [], 0, 0
            used.append(self)

        def reset(self):
            self.resets += 1
            return super().reset()

        def steps_fused(self, *a, **kw):
            ok = super().steps_fused(*a, **kw)
            self.fused.append(ok)
            return ok

        def step(self, *a, **kw):
            self.steps += 1
            return super().step(*a, **kw)

    monkeypatch.setattr(evaluate, "RolloutEngine", Spy)
    return used


def _counts(used):
    assert len(used) == 1
    return used[0].resets, used[0].fused, used[0].steps


def test_eval_model_steps_one_by_one(spy):
    from com_marl_amd.evaluate import eval_model
    env = _wrapper()
    out = eval_model(env, _policies(env, 1)[0], 0, n_eval_episodes=40, max_env_steps=T)       # 32 + 8 episodes
    assert len(out[0]) == 40
    assert _counts(spy) == (2, [], 2 * T)


def test_eval_summary_of_a_single_policy_steps_one_by_one(spy):
    from com_marl_amd.evaluate import eval_summary
    env = _wrapper()
    out = eval_summary(env, _policies(env, 1)[0], 0, n_eval_episodes=40, max_env_steps=T)
    assert out["n_episodes"] == 40
    assert _counts(spy) == (2, [], 2 * T)


def test_eval_models_plays_a_round_as_one_chunk(spy):
    from com_marl_amd.evaluate import eval_models
    env = _wrapper()
    out = eval_models(env, _policies(env, 2), 0, n_eval_episodes=24, max_env_steps=T)         # 16 + 8 episodes of 16 envs each
    assert [len(o[0]) for o in out] == [24, 24]
    assert _counts(spy) == (2, [True, True], 0)


def test_eval_summary_of_two_policies_plays_a_round_as_one_chunk(spy):
    from com_marl_amd.evaluate import eval_summary
    env = _wrapper()
    out = eval_summary(env, _policies(env, 2), 0, n_eval_episodes=24, max_env_steps=T)
    assert [o["n_episodes"] for o in out] == [24, 24]
    assert _counts(spy) == (2, [True, True], 0)


def test_eval_sweep_of_a_single_policy_asks_for_the_chunk(spy):
    from com_marl_amd.evaluate import eval_sweep
    env = _wrapper(channel="IID", conditions=CONDS)                                           # no fused_conditions: declined
    out = eval_sweep(env, _policies(env, 1)[0], 0, n_eval_episodes=24, max_env_steps=T)       # 16 envs per cell
    assert [o["n_episodes"] for o in out] == [24, 24]
    assert _counts(spy) == (2, [False, False], 2 * T)


def test_eval_summary_without_comm_stats_allocates_none(spy, monkeypatch):
    from com_marl_amd import evaluate

    class Refusing:
        def __init__(self, *a, **kw):
            raise AssertionError("comm_stats=False built a _CommStats")

    monkeypatch.setattr(evaluate, "_CommStats", Refusing)
    env = _wrapper()
    out = evaluate.eval_summary(env, _policies(env, 2), 0, n_eval_episodes=24, max_env_steps=T, comm_stats=False)
    assert all(not set(evaluate.COMM_KEYS) & set(o) for o in out)
    with pytest.raises(AssertionError, match="built a _CommStats"):                           # the replacement bites
        evaluate.eval_summary(_wrapper(), _policies(env, 2), 0, n_eval_episodes=24, max_env_steps=T, comm_stats=True)
