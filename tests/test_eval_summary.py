"""evaluate.eval_summary: the score of K policies from ONE [K,12] device-to-host copy must be the score numpy computes from what
evaluate.eval_models (one policy: eval_model) returns for the same episodes.  Two fresh wrappers of the same params and seed play
the same episodes (a second call on one wrapper would play new ones), one through each path.

Bounds (tests/episode_ref.py).  Per episode: integer-valued columns equal; a summed column within 2 n 2^-53 sum|x_t| (two n-term
f64 sums in different orders); nodeDeg within rtol 2^-23 (the host path rounds each step's degree to f32) plus its sum bound.
Over a policy's E episodes, with delta the per-episode bound: means within 2 E 2^-53 mean|x| + mean(delta); the standard
deviation within (2 E 2^-53 mean|x| + max(delta)) range / std + 2 E 2^-53 std; min and max within max(delta)."""
import numpy as np
import pytest

from tests import any_shapes as G, episode_ref as R

pytestmark = pytest.mark.gpu

T_PP = 40                       # with one prey, wrapper seed 3 and policy seeds 10, 11 the CPU oracle (driven as
#                                 test_hip_eval_parity._oracle_greedy_episodes drives it, sampled actions through oracle.sample_actions)
#                                 ends one of the 32 first-round episodes early - step 13 greedy, step 23 sampled - and cuts the rest


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch


def _params(scen, map_, sen, N, M, mpl, **kw):
    pp = scen == "pp"
    p = dict(load=2, max_env_steps=mpl, capture_reward=10 if pp else 2, step_cost=0.1 if pp else 0, rm=0,
             penalty=0 if pp else 1, revisit_penalty=0.5, lazy_penalty=1, grid_size=map_, Rsen=sen, n_agents=N,
             n_preys=M, n_gcn_layers=2, mode="train", trRcom=9, trpl=0, obstComplex="Easy", add_clock=0)
    p.update(kw)
    return p


def _wrapper(scen, params, n_envs, off=0):
    from com_marl_amd import envs as E
    cls = E.PredatorPreyWrapper if scen == "pp" else E.CoverageWrapper
    return cls(True, params=params, n_envs=n_envs, device="cuda:0", seed=3, env_id_offset=off)


def _policies(env, K, seed0=10):
    import torch
    from com_marl_amd import nets
    out = []
    for k in range(K):
        torch.manual_seed(seed0 + k)
        p = nets.CommCategoricalMLPPolicy(env.spec, n_agents=env.n_agents, n_gcn_layers=2, device="cuda:0")
        p.set_rng(3)
        out.append(p)
    return out


def _host_table(out, pp):
    """One eval_model / eval_models tuple -> the [E,9] per-episode table it holds and the [E,9] bound of every entry."""
    from com_marl_amd.evaluate import VECTORS
    data, succ, rew, _ = out
    E = len(data)
    tab, delta = np.zeros((E, R.EPI_COLS)), np.zeros((E, R.EPI_COLS))
    tab[:, 0] = succ
    whole = {"step_cnt"} | ({"capture_cnt", "penalty_cnt", "vars2"} if pp else set())
    for i, vec in enumerate(VECTORS):
        tab[:, 1 + i] = rew[vec]
        for e, (_, steps) in enumerate(data):
            x = np.abs(np.asarray(steps[vec], np.float64))
            if vec == "nodeDeg":
                delta[e, 1 + i] = 2.0 ** -23 * abs(tab[e, 1 + i]) + R.sum_bound(len(x), x.sum()) / len(x)
            elif vec not in whole:
                delta[e, 1 + i] = R.sum_bound(len(x), x.sum())
    return tab, delta


def _check(summary, out, pp, episodes=None):
    from com_marl_amd.evaluate import VECTORS
    tab, delta = _host_table(out, pp)
    want = R.episode_means(tab[None])[0]
    E = len(tab)
    assert summary["n_episodes"] == E and summary["bound_return"] == out[3]
    got = [summary["success"]] + [summary[v] for v in VECTORS]
    for c in range(R.EPI_COLS):
        assert abs(got[c] - want[c]) <= R.mean_bound(tab[:, c], delta[:, c]), (R.COLS[c], got[c], want[c])
    assert abs(summary["return_std"] - want[9]) <= R.std_bound(tab[:, 1], delta[:, 1])
    assert abs(summary["return_min"] - want[10]) <= delta[:, 1].max()
    assert abs(summary["return_max"] - want[11]) <= delta[:, 1].max()
    if episodes is not None:
        assert (np.abs(episodes - tab) <= delta).all(), np.abs(episodes - tab).max(0)
    return tab


def _both(scen, params, K, Bk, n_epi, T, greedy, pols_of=_policies, **kw):
    from com_marl_amd.evaluate import eval_models, eval_summary
    w1, w2 = _wrapper(scen, params, K * Bk), _wrapper(scen, params, K * Bk)
    pols = pols_of(w1, K)
    got = eval_summary(w1, pols, 0, n_eval_episodes=n_epi, max_env_steps=T, eval_greedy=greedy, **kw)
    ref = eval_models(w2, pols, 0, n_eval_episodes=n_epi, max_env_steps=T, eval_greedy=greedy)
    assert isinstance(got, list) and len(got) == K == len(ref)
    return w1, w2, got, ref


@pytest.mark.parametrize("greedy", [True, False], ids=["greedy", "sampled"])
@pytest.mark.parametrize("recorded", [False, True], ids=["full_graph", "recorded_adjacency"])
def test_pp_two_policies_two_rounds(gpu, greedy, recorded):
    """PP map 10, teams of 4, K = 2 on 16 envs each, 20 episodes: a full round and a ragged one of 4.  With mode='test',
    teRcom=2, tepl=0.25 the adjacency is range-limited and recorded per step: nodeDeg comes from the adjacency walk."""
    extra = dict(mode="test", teRcom=2, tepl=0.25) if recorded else {}
    params = _params("pp", 10, 1, 4, 1, T_PP, **extra)
    w1, w2, got, ref = _both("pp", params, 2, 16, 20, T_PP, greedy, episodes=True)
    assert w1.batch.adj_const != recorded
    lengths = []
    for k in range(2):
        ep = got[k]["episodes"]
        assert ep.shape == (20, 9) and ep.is_cuda and ep.dtype == gpu.float64
        tab = _check(got[k], ref[k], True, ep.cpu().numpy())
        lengths += tab[:, 3].tolist()
        if recorded:
            assert 0 < got[k]["nodeDeg"] < 4 and got[k]["nodeDeg"] != round(got[k]["nodeDeg"])
        else:
            assert got[k]["nodeDeg"] == 4.0
    # the condition of the comparison: some compared episode ends before the step limit and some is cut by it (the seeds were
    # picked for the full graph; a range-limited team plays other episodes)
    assert max(lengths) == T_PP and (recorded or min(lengths) < T_PP), sorted(lengths)
    assert w1.eval_n_epi == w2.eval_n_epi == 20
    for k in range(2):
        assert w1.last_eval_average_reward[k] == got[k]["reward"] / got[k]["bound_return"]


def test_coverage_with_iid_loss(gpu):
    """Coverage map 10 with IID link loss, teams of 4: the CO column rules (every detail column / nA, vars2); bound_return is
    the scalar."""
    params = _params("co", 10, 2, 4, 0, 8, trpl=0.3)
    w1, _, got, ref = _both("co", params, 3, 4, 6, 8, True)
    for k in range(3):
        _check(got[k], ref[k], False)
        assert np.isscalar(got[k]["bound_return"]) and "episodes" not in got[k]
    assert all(g["step_cnt"] == 8.0 for g in got) and any(g["vars2"] != 0.0 or g["penalty_cnt"] != 0.0 for g in got)


def test_single_policy_equals_eval_model(gpu):
    from com_marl_amd.evaluate import eval_model, eval_summary
    params = _params("pp", 10, 1, 4, 1, T_PP)
    w1, w2 = _wrapper("pp", params, 16), _wrapper("pp", params, 16)
    pol = _policies(w1, 1)[0]
    got = eval_summary(w1, pol, 0, n_eval_episodes=20, max_env_steps=T_PP, eval_greedy=False)
    ref = eval_model(w2, pol, 0, n_eval_episodes=20, max_env_steps=T_PP, eval_greedy=False)
    assert isinstance(got, dict)
    _check(got, ref, True)
    assert w1.eval_n_epi == w2.eval_n_epi == 20 and w1.last_eval_average_reward == got["reward"] / got["bound_return"]


def test_custom_layer_sizes_policy_set(gpu):
    """A PolicySet of non-default layer sizes (tests/any_shapes.py shape A): the member form of the loop engine."""
    torch = gpu
    from com_marl_amd import nets

    def pols_of(env, K):
        out = []
        for k in range(K):
            p, _ = G.build("A", critic=False)
            with torch.no_grad():
                for q in p.parameters():
                    q.mul_(1.0 + 0.25 * k)
            p.set_rng(3)
            out.append(p)
        return nets.PolicySet(out)

    params = _params("pp", 10, 1, 4, 4, 10, trRcom=3, trpl=0.3)
    _, _, got, ref = _both("pp", params, 2, 8, 12, 10, False, pols_of=pols_of)
    for k in range(2):
        _check(got[k], ref[k], True)


def test_summary_row_flag_and_refusals(gpu):
    from com_marl_amd.evaluate import VECTORS, eval_summary, summary_row
    params = _params("pp", 10, 1, 4, 4, 10)
    w = _wrapper("pp", params, 6)
    pols = _policies(w, 4)
    assert eval_summary(w, pols[:2], 0, flag=[1]) == [None, None] and eval_summary(w, pols[0], 0, flag=[1]) is None
    with pytest.raises(ValueError, match="evenly"):
        eval_summary(w, pols, 0, n_eval_episodes=4, max_env_steps=10)             # 6 envs, 4 policies
    with pytest.raises(ValueError, match="max_path_length"):
        eval_summary(w, pols[:2], 0, n_eval_episodes=4, max_env_steps=11)
    s = eval_summary(w, pols[:2], 0, n_eval_episodes=4, max_env_steps=10)[1]
    assert summary_row(s) == [s["success"]] + [s[v] for v in VECTORS] and len(summary_row(s)) == 9
    assert summary_row(s)[3] == s["step_cnt"] and 1 <= s["step_cnt"] <= 10
    assert s["return_min"] <= s["reward"] <= s["return_max"] and s["return_std"] >= 0.0
