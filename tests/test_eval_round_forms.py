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

    from tests.test_value_stats import _critics

    class Refusing:
        def __init__(self, fam, *a, **kw):
            raise AssertionError(f"built a _Side for {fam.name}")

    monkeypatch.setattr(evaluate, "_Side", Refusing)
    env = _wrapper()
    pols = _policies(env, 2)
    out = evaluate.eval_summary(env, pols, 0, n_eval_episodes=24, max_env_steps=T, comm_stats=False, attn_stats=False,
                                listen_stats=False, value_stats=False)
    keys = set(evaluate.COMM_KEYS + evaluate.ATTN_KEYS + evaluate.LISTEN_KEYS + evaluate.VALUE_KEYS)
    assert all(not keys & set(o) for o in out)
    for switch, fam in evaluate.FAMILIES.items():                                             # the replacement bites, for each switch
        kw = dict(baselines=_critics(env, 2)) if switch == "value_stats" else {}
        with pytest.raises(AssertionError, match=f"built a _Side for {fam.name}"):
            evaluate.eval_summary(_wrapper(), pols, 0, n_eval_episodes=24, max_env_steps=T, **{switch: True}, **kw)


def test_all_switches_at_once_equal_each_switch_alone():
    """eval_sweep of 2 policies x 2 conditions x 8 envs, 12 episodes: two rounds, the second ragged (take = 4 < 8 at row0 = 8).  With
    all five switches on, every key, episode table and curve of every cell is bit for bit what a call with that family alone
    returns - without and with curves - and the keys of a call with every switch off are the same in all of them: no section of
    the one buffer, no side's place in the order and no round's accumulate depends on which other switches are on."""
    import numpy as np
    import torch
    from com_marl_amd import evaluate
    from tests.test_value_stats import _critics

    def same(a, b, what):
        if isinstance(a, torch.Tensor):
            assert torch.equal(a, b), what
        elif isinstance(a, np.ndarray):
            np.testing.assert_array_equal(a, b, err_msg=str(what))
        else:
            assert a == b, what

    env = _wrapper(channel="IID", conditions=CONDS)
    pols, critics = _policies(env, 2), _critics(env, 2)

    def sweep(**kw):
        if kw.get("value_stats"):
            kw["baselines"] = critics
        return evaluate.eval_sweep(_wrapper(channel="IID", conditions=CONDS), pols, 0, n_eval_episodes=12, max_env_steps=T,
                                   episodes=True, **kw)

    families = {"comm_stats": evaluate.COMM_KEYS, "attn_stats": evaluate.ATTN_KEYS, "listen_stats": evaluate.LISTEN_KEYS,
                "value_stats": evaluate.VALUE_KEYS}
    every = sweep(curves=True, **{switch: True for switch in families})
    none = sweep()
    calls = [((), False, none), ((), True, sweep(curves=True))]
    for switch in families:
        calls += [((switch,), False, sweep(**{switch: True})), ((switch,), True, sweep(curves=True, **{switch: True}))]
    for on, curves, got in calls:
        for k in range(2):
            for c in range(2):
                cell, full, what = got[k][c], every[k][c], (on, curves, k, c)
                names = [name for switch in on for name in families[switch]]
                tables = [switch[:-len("stats")] + "episodes" for switch in on]
                assert set(cell) == set(none[k][c]) | set(names) | set(tables) | ({"curves"} if curves else set()), what
                for key, v in cell.items():
                    if key != "curves":
                        same(v, full[key], what + (key,))
                if curves:
                    assert set(cell["curves"]) == set(["success"] + evaluate.VECTORS + names), what
                    for key, v in cell["curves"].items():
                        same(v, full["curves"][key], what + ("curves", key))
    assert set(every[0][0]) == set(none[0][0]) | {"curves", "comm_episodes", "attn_episodes", "listen_episodes", "value_episodes"} | {
        name for names in families.values() for name in names}
