"""evaluate.eval_summary / eval_sweep with curves=True: the per-step curves of cell / policy k must be the zero-padded mean over
the episodes of what evaluate.eval_models (one policy: eval_model) lists per step for the same episodes - the reference's rewMat3
rule (pad_sequence(..., padding_value=0), then the mean over the episode axis).  Fresh wrappers of the same params and seed play
the same episodes (the premise of tests/test_eval_summary.py), one through each path.

Bounds (tests/curves_ref.py).  With E episodes and, per step, S = the sum over the episodes of |x|: the reward within E 2^-53 S on
the sum, i.e. 2^-53 S on the mean (two f64 sums of the same terms in different orders); the columns that are integers divided by
nA within the same bound (the host divides per step and sums the quotients, the device sums the integers and divides once);
nodeDeg additionally rtol 2^-23 (the host path rounds each step's degree to f32).  A summed vector's curve adds up to the
vector's summary value: both are sums of the same E T terms grouped differently, within 2 (E T) 2^-53 (sum of all |x|) / E."""
import numpy as np
import pytest

from tests import comm_ref, conditions_common as cc, curves_ref as V, episode_ref as R

pytestmark = pytest.mark.gpu

T_PP = 40                       # tests/test_eval_summary.py: with these seeds one first-round episode ends early, the rest are cut


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


def _wrapper(scen, params, n_envs, off=0, **kw):
    from com_marl_amd import envs as E
    cls = E.PredatorPreyWrapper if scen == "pp" else E.CoverageWrapper
    return cls(True, params=params, n_envs=n_envs, device="cuda:0", seed=3, env_id_offset=off, **kw)


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


def _check_curves(summary, out, pp, T, comm=False):
    """summary: one eval_summary dict with curves; out: the eval_model(s) tuple of the same episodes."""
    from com_marl_amd.evaluate import COMM_KEYS, VECTORS
    curves = summary["curves"]
    data = out[0]
    E = len(data)
    assert set(curves) == {"success"} | set(VECTORS) | (set(COMM_KEYS) if comm else set())
    lists = {vec: [steps[vec] for _, steps in data] for vec in VECTORS}
    lists["success"] = [succ for succ, _ in data]
    whole = {"success", "step_cnt"} | ({"capture_cnt", "penalty_cnt", "vars2"} if pp else set())
    for name in ["success"] + VECTORS:
        got = curves[name]
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (T,)
        want, mean_abs = V.padded_mean(lists[name], T)
        bound = np.zeros(T) if name in whole else V.reward_bound(E, mean_abs * E)
        if name == "nodeDeg":
            bound = bound + 2.0 ** -23 * np.abs(want)
        err = np.abs(got - want)
        print(f"{name}: max err {err.max():.3e}, bound at it {bound[err.argmax()]:.3e}")
        assert (err <= bound).all(), (name, err.max(), got[err > bound], want[err > bound])
        if name not in ("success", "nodeDeg"):                  # the summed vectors
            tot = R.sum_bound(E * T, mean_abs.sum() * E) / E
            assert abs(got.sum() - summary[name]) <= tot, (name, got.sum(), summary[name])
    step = curves["step_cnt"]
    assert step[0] == 1.0 and (np.diff(step) <= 0).all() and step[-1] >= 0.0
    return step


def _same_but_curves(with_, without):
    assert set(with_) == set(without) | {"curves"}
    for key, v in without.items():
        assert with_[key] == v, key                              # floats: the same bits


@pytest.mark.parametrize("greedy", [True, False], ids=["greedy", "sampled"])
@pytest.mark.parametrize("recorded", [False, True], ids=["full_graph", "recorded_adjacency"])
def test_pp_two_policies_two_rounds(gpu, greedy, recorded):
    """PP map 10, teams of 4, K = 2 on 16 envs each, 20 episodes: a full round and a ragged one of 4.  With mode='test',
    teRcom=2, tepl=0.25 the adjacency is range-limited and recorded per step: nodeDeg comes from the adjacency walk."""
    from com_marl_amd.evaluate import eval_models, eval_summary
    params = _params("pp", 10, 1, 4, 1, T_PP, **(dict(mode="test", teRcom=2, tepl=0.25) if recorded else {}))
    w1, w2, w3 = (_wrapper("pp", params, 32) for _ in range(3))
    pols = _policies(w1, 2)
    kw = dict(n_eval_episodes=20, max_env_steps=T_PP, eval_greedy=greedy)
    got = eval_summary(w1, pols, 0, curves=True, **kw)
    ref = eval_models(w2, pols, 0, **kw)
    plain = eval_summary(w3, pols, 0, **kw)
    assert w1.batch.adj_const != recorded
    last = []
    for k in range(2):
        step = _check_curves(got[k], ref[k], True, T_PP)
        _same_but_curves(got[k], plain[k])
        deg = got[k]["curves"]["nodeDeg"]
        last.append(step[-1])
        if recorded:
            assert 0 < deg[0] < 4 and deg[0] != round(deg[0])
        else:
            assert (deg == 4.0 * step).all()                     # the constant full graph: N per running episode
    # the condition of the comparison: some compared episode ends before the step limit (tests/test_eval_summary.py picked the
    # seeds for the full graph): the zero padding is exercised
    assert recorded or min(last) < 1.0, last
    assert w1.last_eval_average_reward == w3.last_eval_average_reward and w1.eval_n_epi == 20


def test_coverage_with_iid_loss_teams_of_5(gpu):
    """Coverage map 10 with IID link loss, N = 5: the CO column rules (every detail column / nA with nA no power of two, vars2)
    and the 4-byte adjacency walk; K = 3 on 4 envs each, 6 episodes (a ragged second round of 2)."""
    from com_marl_amd.evaluate import eval_models, eval_summary
    params = _params("co", 10, 2, 5, 0, 8, mode="test", teRcom=3, tepl=0.3)
    w1, w2, w3 = (_wrapper("co", params, 12) for _ in range(3))
    pols = _policies(w1, 3)
    kw = dict(n_eval_episodes=6, max_env_steps=8)
    got = eval_summary(w1, pols, 0, curves=True, **kw)
    ref = eval_models(w2, pols, 0, **kw)
    plain = eval_summary(w3, pols, 0, **kw)
    for k in range(3):
        _check_curves(got[k], ref[k], False, 8)
        _same_but_curves(got[k], plain[k])
    assert any((g["curves"]["vars2"] != 0).any() or (g["curves"]["penalty_cnt"] != 0).any() for g in got)


def test_single_policy_equals_eval_model(gpu):
    from com_marl_amd.evaluate import eval_model, eval_summary
    params = _params("pp", 10, 1, 4, 1, T_PP)
    w1, w2, w3 = (_wrapper("pp", params, 16) for _ in range(3))
    pol = _policies(w1, 1)[0]
    kw = dict(n_eval_episodes=20, max_env_steps=T_PP, eval_greedy=False)
    got = eval_summary(w1, pol, 0, curves=True, **kw)
    ref = eval_model(w2, pol, 0, **kw)
    assert isinstance(got, dict)
    step = _check_curves(got, ref, True, T_PP)
    _same_but_curves(got, eval_summary(w3, pol, 0, **kw))
    assert (got["curves"]["nodeDeg"] == 4.0 * step).all()        # the constant full graph: N per running episode


class _Recorder:
    """Stands in for evaluate.RolloutEngine: after every round (bump) the engine's path_len and the rows comm_ref computes from
    its recorded dist_adj / channels, on the host."""
    rounds = []

    @classmethod
    def install(cls, monkeypatch, T):
        from com_marl_amd import evaluate
        cls.rounds = rounds = []

        class Spy(evaluate.RolloutEngine):
            def bump(self, n):
                out = super().bump(n)
                batch = self.env
                B, N, Lh = batch.B, batch.N, batch.Lh
                adj = None if self.dist_adj is None else self.dist_adj.cpu().numpy().reshape((T + 1) * B, N, N)
                if self.channels is not None:
                    chan = self.channels.cpu().numpy().reshape((T + 1) * B, Lh, N, N)
                else:
                    chan = None if batch.channelType == "FC" else batch.channels[0].cpu().numpy()
                stats = comm_ref.comm_stats(adj, chan, N, Lh, (T + 1) * B).reshape(T + 1, B, V.COMM_COLS)
                rounds.append((self.path_len[:T].cpu().numpy(), stats))
                return out

        monkeypatch.setattr(evaluate, "RolloutEngine", Spy)
        return rounds


def test_sweep_two_policies_two_conditions_with_comm_stats(gpu, monkeypatch):
    """K = 2 x C = 2 on teams of 4, cells of 8 envs, 12 episodes (a second round that takes 4), IID loss: every cell's curves
    against eval_model on the uniform wrapper of its condition, the comm curves against the restatement applied to the engine's
    recorded dist_adj / channels, and curves=False against the same call without the key."""
    from com_marl_amd.evaluate import COMM_STATS, eval_model, eval_sweep
    T, E, n_epi, off = 20, 8, 12, 5
    params = cc.base_params("pp", 10, 1, 4, 4, max_env_steps=T)
    conds = [dict(Rcom=9, pl=0), dict(Rcom=2, pl=0.3)]

    def wrapper(**kw):
        return _wrapper("pp", params, 2 * 2 * E, off=off, channel="IID", conditions=conds, **kw)

    env = wrapper()
    pols = _policies(env, 2, seed0=30)
    rounds = _Recorder.install(monkeypatch, T)
    got = eval_sweep(env, pols, 0, n_eval_episodes=n_epi, max_env_steps=T, paired=True, comm_stats=True, curves=True)
    monkeypatch.undo()
    assert len(rounds) == 2
    plain = eval_sweep(wrapper(), pols, 0, n_eval_episodes=n_epi, max_env_steps=T, paired=True, comm_stats=True)
    sums = np.zeros((4, T, V.COMM_COLS))
    for r, (path_len, stats) in enumerate(rounds):
        V.comm_curves(path_len, stats, E, min(E, n_epi - r * E), int(r > 0), sums)
    want = V.comm_curve_means(sums, n_epi, 4, env.batch.Lh)
    for k in range(2):
        for c in range(2):
            cell = got[k][c]
            w = _wrapper("pp", cc.with_condition(params, conds[c]), E, off=off, channel="IID")
            ref = eval_model(w, pols[k], 0, n_eval_episodes=n_epi, max_env_steps=T)
            _check_curves(cell, ref, True, T, comm=True)
            _same_but_curves(cell, plain[k][c])
            for i, name in enumerate(COMM_STATS):
                assert (cell["curves"][name] == want[k * 2 + c, :, i]).all(), (k, c, name)
            assert (cell["curves"]["delivery"] == V.delivery(want[k * 2 + c])).all()
        full, lossy = got[k][0]["curves"], got[k][1]["curves"]
        run = full["step_cnt"] > 0
        assert (full["range_degree"][run] == 3 * full["step_cnt"][run]).all() and (full["delivery"] == 1.0).all()
        assert (lossy["delivery"][lossy["range_degree"] > 0] < 1.0).any()


def test_fused_conditions_sweep_gives_the_same_curves(gpu):
    """The wave-owned one-launch rollout of a fused_conditions wrapper and the two-launch form: the same curves, bit for bit."""
    from com_marl_amd.evaluate import eval_sweep
    T, E = 20, 16
    params = cc.base_params("pp", 10, 1, 4, 4, max_env_steps=T)
    conds = [dict(Rcom=9, pl=0), dict(Rcom=2, pl=0.3), dict(Rcom=1, pl=0.9)]
    outs = []
    for kw in (dict(fused_conditions=True), {}):
        env = _wrapper("pp", params, 2 * 3 * E, off=5, channel="IID", conditions=conds, **kw)
        outs.append(eval_sweep(env, _policies(env, 2, seed0=30), 0, n_eval_episodes=24, max_env_steps=T, comm_stats=True, curves=True))
    for k in range(2):
        for c in range(3):
            a, b = outs[0][k][c]["curves"], outs[1][k][c]["curves"]
            assert set(a) == set(b)
            for name in a:
                assert a[name].tobytes() == b[name].tobytes(), (k, c, name)


def test_flag_and_default_leave_no_curves(gpu):
    from com_marl_amd.evaluate import eval_summary
    params = _params("pp", 10, 1, 4, 4, 10)
    w = _wrapper("pp", params, 6)
    pols = _policies(w, 2)
    assert eval_summary(w, pols, 0, flag=[1], curves=True) == [None, None]
    assert all("curves" not in d for d in eval_summary(w, pols, 0, n_eval_episodes=4, max_env_steps=10))
    assert all(d["curves"]["reward"].shape == (10,) for d in eval_summary(w, pols, 0, n_eval_episodes=4, max_env_steps=10, curves=True))
