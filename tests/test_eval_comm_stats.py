"""evaluate.eval_summary / eval_sweep with comm_stats=True.  The keys of a call without the flag stay what they are; the new keys
are what tests/comm_ref.py computes from the engine's dist_adj / channels / path_len of the same rounds, which a third fresh
wrapper of the same params and seed plays through a RolloutEngine of its own (fresh wrappers of one seed play the same episodes:
the premise of tests/test_eval_summary.py).  Per-episode rows are integer sums divided once: ==.  Means of E rows: within
episode_ref.mean_bound.  The anchors hold exactly: equal integer sums give equal quotients, and a mean of equal values is that
value."""
import numpy as np
import pytest

from tests import comm_ref as R, conditions_common as cc, episode_ref as ER

pytestmark = pytest.mark.gpu

T, N = 20, 4


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch


def _params(**over):
    return cc.base_params("pp", 10, 1, N, 4, max_env_steps=T, **over)


def _wrapper(scen, params, n_envs, channel=None, off=0, **kw):
    from com_marl_amd import envs as E_
    cls = E_.PredatorPreyWrapper if scen == "pp" else E_.CoverageWrapper
    return cls(True, params=params, n_envs=n_envs, device="cuda:0", seed=3, env_id_offset=off, channel=channel, **kw)


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


def _expected(env, pols, n_epi, greedy=True):
    """The rounds eval_summary plays on `env` (a fresh wrapper), through an engine of this test's own -> per policy the
    [n_epi, 4] episode table comm_ref computes from the copied-out buffers."""
    from com_marl_amd.nets import PolicySet
    from com_marl_amd.rollout import RolloutEngine
    batch = getattr(env, "env", env).batch
    single = not isinstance(pols, list)
    ps = pols if single else PolicySet(pols)
    K = 1 if single else len(pols)
    B, n, Lh = batch.B, batch.N, batch.Lh
    Bk = B // K
    ps.sync_weights()
    ps.reset([True] * Bk)
    kw = {} if single else dict(groups=[Bk] * K)
    eng = RolloutEngine(batch, ps, T, store_attn=False, store_probs=False, **kw)
    table = np.zeros((K * n_epi, R.EPC_COLS))
    done = 0
    while done < n_epi:
        eng.reset()
        if single or not eng.steps_fused(0, T, greedy=greedy):
            eng.fork()
            for t in range(T):
                eng.step(t, greedy=greedy)
            eng.join()
        eng.bump(T)
        batch.check_status()
        adj = None if eng.dist_adj is None else eng.dist_adj.cpu().numpy().reshape((T + 1) * B, n, n)
        if eng.channels is not None:
            chan = eng.channels.cpu().numpy().reshape((T + 1) * B, Lh, n, n)
        else:
            chan = None if batch.channelType == "FC" else batch.channels[0].cpu().numpy()       # FL: the constant block
        stats = R.comm_stats(adj, chan, n, Lh, (T + 1) * B).reshape(T + 1, B, R.COMM_COLS)
        take = min(Bk, n_epi - done)
        R.episode_comm(eng.path_len.cpu().numpy(), stats, n, Lh, Bk, take, n_epi, done, table)
        done += take
    return table.reshape(K, n_epi, R.EPC_COLS)


def _check_comm(summary, table):
    from com_marl_amd.evaluate import COMM_KEYS
    assert set(COMM_KEYS) <= set(summary)
    want = R.comm_means(table[None])[0]
    for c, name in enumerate(R.EPC):
        assert abs(summary[name] - want[c]) <= ER.mean_bound(table[:, c]), (name, summary[name], want[c])
    assert summary["delivery"] == (summary["heard_degree"] / summary["range_degree"] if summary["range_degree"] != 0 else 1.0)
    if "comm_episodes" in summary:
        ep = summary["comm_episodes"]
        assert tuple(ep.shape) == table.shape and ep.is_cuda
        np.testing.assert_array_equal(ep.cpu().numpy(), table)


def _same_but_comm(with_, without):
    import torch
    from com_marl_amd.evaluate import COMM_KEYS
    assert set(with_) == set(without) | set(COMM_KEYS) | ({"comm_episodes"} if "episodes" in without else set())
    for key, v in without.items():
        if key == "episodes":
            assert torch.equal(with_[key], v)
        else:
            assert with_[key] == v, key


def test_two_policies_two_rounds_with_loss_and_range(gpu):
    """PP map 10, teams of 4, 64 envs = 2 policies x 32, T = 20, 48 episodes each: a full round and one that takes 16."""
    from com_marl_amd.evaluate import eval_summary
    params = _params(teRcom=2, tepl=0.3)
    w1, w2, w3 = (_wrapper("pp", params, 64) for _ in range(3))
    pols = _policies(w1, 2)
    got = eval_summary(w1, pols, 0, n_eval_episodes=48, max_env_steps=T, episodes=True, comm_stats=True)
    plain = eval_summary(w2, pols, 0, n_eval_episodes=48, max_env_steps=T, episodes=True)
    table = _expected(w3, pols, 48)
    for k in range(2):
        _same_but_comm(got[k], plain[k])
        _check_comm(got[k], table[k])
        assert 0 < got[k]["heard_degree"] < got[k]["range_degree"] < N - 1 and 0 < got[k]["delivery"] < 1
        assert 0 < got[k]["reach"] < got[k]["range_reach"] <= N - 1
    assert w1.eval_n_epi == 48 and w1.last_eval_average_reward == w2.last_eval_average_reward


ANCHORS = {
    "no_loss": dict(teRcom=2, tepl=0.0),
    "full_loss": dict(teRcom=2, tepl=1.0),
    "full_graph": dict(teRcom=0, tepl=0.0),
}


@pytest.mark.parametrize("name", list(ANCHORS))
def test_anchors_hold_exactly_for_a_single_policy(gpu, name):
    """A single policy on 64 envs, 100 episodes (two rounds), sampled actions.  Constant inputs reach the kernel as NULL (full
    graph, FC channel) or as one block with stride 0 (FL: the identity)."""
    from com_marl_amd.evaluate import eval_summary
    params = _params(**ANCHORS[name])
    w1, w2, w3 = (_wrapper("pp", params, 64) for _ in range(3))
    pol = _policies(w1, 1)[0]
    got = eval_summary(w1, pol, 0, n_eval_episodes=100, max_env_steps=T, eval_greedy=False, comm_stats=True)
    plain = eval_summary(w2, pol, 0, n_eval_episodes=100, max_env_steps=T, eval_greedy=False)
    assert isinstance(got, dict) and "comm_episodes" not in got
    _same_but_comm(got, plain)
    _check_comm(got, _expected(w3, pol, 100, greedy=False)[0])
    batch = getattr(w1, "env", w1).batch
    if name == "no_loss":
        assert batch.ch_const and not batch.adj_const
        assert got["delivery"] == 1.0 and got["reach"] == got["range_reach"] and 0 < got["range_degree"] < N - 1
    elif name == "full_loss":
        assert batch.ch_const and batch.channelType == "FL"
        assert got["heard_degree"] == 0 and got["reach"] == 0 and got["delivery"] == 0 and got["range_reach"] > 0
    else:
        assert batch.adj_const and batch.ch_const
        assert got["range_degree"] == N - 1 and got["reach"] == N - 1 and got["delivery"] == 1.0


K, E, N_EPI = 2, 16, 24                          # cells of 16 envs, 24 episodes: a second round that takes 8
SHAPES = {
    "pp4": ("pp", cc.base_params("pp", 10, 1, 4, 4, max_env_steps=T), "IID",
            [dict(Rcom=0, pl=0), dict(Rcom=2, pl=0.3), dict(Rcom=1, pl=0.9)]),
    "co24": ("co", cc.base_params("co", 20, 2, 24, 0, max_env_steps=T), "GE",
             [dict(Rcom=0, Pgb=0.0, Pbg=1.0), dict(Rcom=6, Pgb=0.4, Pbg=0.1), dict(Rcom=3, Pgb=0.9, Pbg=0.9)]),
}


def _cells_equal_eval_summary(shape, e, n_epi=N_EPI, **kw):
    from com_marl_amd.evaluate import COMM_KEYS, eval_summary, eval_sweep
    scen, params, channel, conds = SHAPES[shape]
    Cn = len(conds)
    env = _wrapper(scen, params, K * Cn * e, channel, off=5, conditions=conds, **kw)
    pols = _policies(env, K)
    got = eval_sweep(env, pols, 0, n_eval_episodes=n_epi, max_env_steps=T, paired=True, episodes=True, comm_stats=True)
    for k in range(K):
        for c in range(Cn):
            w = _wrapper(scen, cc.with_condition(params, conds[c]), e, channel, off=5)
            ref = eval_summary(w, pols[k], 0, n_eval_episodes=n_epi, max_env_steps=T, episodes=True, comm_stats=True)
            for key in COMM_KEYS:
                assert got[k][c][key] == ref[key], (k, c, key, got[k][c][key], ref[key])
            assert gpu_equal(got[k][c]["comm_episodes"], ref["comm_episodes"]), (k, c)
            assert got[k][c]["reward"] == ref["reward"] and got[k][c]["nodeDeg"] == ref["nodeDeg"]
    return env, got


def gpu_equal(a, b):
    import torch
    return a.shape == b.shape and torch.equal(a, b)


def test_sweep_cells_equal_eval_summary_fused_and_not(gpu):
    """K = 2 x C = 3 on teams of 4, one condition fully connected without loss; the wave-owned one-launch rollout
    (fused_conditions=True, policy groups of 48 envs = whole workgroups of 16) and the two-launch form give the same cells."""
    from com_marl_amd.evaluate import COMM_KEYS
    env_f, fused = _cells_equal_eval_summary("pp4", E, fused_conditions=True)
    env_p, plain = _cells_equal_eval_summary("pp4", E)
    assert getattr(env_f, 'env', env_f).batch.fused_conditions and not getattr(env_p, 'env', env_p).batch.fused_conditions
    for k in range(K):
        for c in range(3):
            assert set(fused[k][c]) == set(plain[k][c])
            for key, v in plain[k][c].items():
                if key in ("episodes", "comm_episodes"):
                    assert gpu_equal(fused[k][c][key], v)
                else:
                    assert fused[k][c][key] == v, (k, c, key)
            assert set(COMM_KEYS) <= set(fused[k][c])
        full = fused[k][0]                                       # Rcom = 0, pl = 0
        assert full["range_degree"] == N - 1 and full["reach"] == N - 1 and full["delivery"] == 1.0
        assert fused[k][2]["delivery"] < fused[k][1]["delivery"] < 1.0 and fused[k][2]["reach"] < fused[k][1]["reach"]


def test_sweep_coverage_teams_of_24_on_the_two_launch_path(gpu):
    _, got = _cells_equal_eval_summary("co24", 4, n_epi=6)             # cells of 4 envs: a second round that takes 2
    for k in range(K):
        full = got[k][0]                                         # Rcom = 0 and a GE chain that never leaves the good state
        assert full["range_degree"] == 23 and full["reach"] == 23 and full["delivery"] == 1.0
        assert got[k][2]["range_degree"] < got[k][1]["range_degree"] < 23 and got[k][1]["delivery"] < 1.0
