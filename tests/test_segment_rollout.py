"""obtain_segments on the GPU: three consecutive segments of 7 steps, weights fixed, are slot for slot and bit for bit ONE
RolloutEngine of horizon 21 stepped from the same reset - with the graph route and with eager steps, for teams of 4 (the
persistent launch; 41 envs leave a ragged wave tile) and for a team of 6 under a short range and a lossy channel (the two-launch
route, both mask buffers kept).  max_env_steps = 9: episodes end inside segments and across their borders.  The episode tables
of the three segments add up to what numpy computes from the long rollout's ended episodes."""
import types

import numpy as np
import pytest

from tests import segments_ref as R

pytestmark = pytest.mark.gpu

N_STEPS, N_SEG, GAMMA = 7, 3, 0.99
SETUPS = {
    "pp4_41envs": dict(B=41, n_agents=4, n_preys=4, trRcom=9, trpl=0),
    "pp4_64envs": dict(B=64, n_agents=4, n_preys=4, trRcom=9, trpl=0),
    "pp6_short_range_lossy": dict(B=24, n_agents=6, n_preys=6, trRcom=2, trpl=0.3),
}
_LONG = {}


@pytest.fixture
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need the MI355X")
    return torch


def _make(torch, B, n_agents, n_preys, trRcom, trpl, seed=4):
    from com_marl_amd import envs as E, nets
    params = dict(load=2, max_env_steps=9, capture_reward=10, step_cost=0.1, rm=0, penalty=0, grid_size=10, Rsen=1, n_agents=n_agents,
                  n_preys=n_preys, n_gcn_layers=2, mode="train", trRcom=trRcom, trpl=trpl, seed=seed)
    env = E.PredatorPreyWrapper(centralized=True, params=params, n_envs=B, device="cuda:0")
    torch.manual_seed(seed)
    pol = nets.CommCategoricalMLPPolicy(env.spec, n_agents=n_agents, device="cuda:0")
    pol.set_rng(seed)
    return env, pol


def _names(eng):
    return [n for n in ("obs", "actions", "probs", "reward64", "done", "path_len", "dist_adj", "channels", "details", "success")
            if getattr(eng, n) is not None]


def _long(torch, name):
    """The one engine of horizon 21 from the reset, its buffers on the host: computed once per setup, left unchanged."""
    if name not in _LONG:
        from com_marl_amd.rollout import RolloutEngine
        env, pol = _make(torch, **SETUPS[name])
        eng = RolloutEngine(env.batch, pol, N_STEPS * N_SEG)
        pol.sync_weights()
        eng.reset()
        pol.reset([True] * env.batch.B)
        eng.play(0, N_STEPS * N_SEG, chunk=False)
        torch.cuda.synchronize()
        env.batch.check_status()
        _LONG[name] = {n: getattr(eng, n).cpu().numpy() for n in _names(eng)}
    return _LONG[name]


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("name", list(SETUPS))
def test_three_segments_are_one_long_rollout(name, use_graph, gpu):
    torch = gpu
    from com_marl_amd import _lib as L
    from com_marl_amd.sampler import CentralizedMAOnPolicyVectorizedSampler, SegmentBatch
    cfg = SETUPS[name]
    long = _long(torch, name)
    if name == "pp6_short_range_lossy":
        assert "dist_adj" in long and "channels" in long                       # both mask buffers are kept and compared
    env, pol = _make(torch, **cfg)
    algo = types.SimpleNamespace(policy=pol, discount=GAMMA, max_path_length=9)
    smp = CentralizedMAOnPolicyVectorizedSampler(algo, env, n_envs=cfg["B"])
    smp.start_worker()
    tables, first = [], None
    for k in range(N_SEG):
        seg = smp.obtain_segments(k, N_STEPS, use_graph=use_graph)
        assert isinstance(seg, SegmentBatch) and (seg.n_steps, seg.B, len(seg)) == (N_STEPS, cfg["B"], cfg["B"])
        assert seg.n_samples == N_STEPS * cfg["B"] * cfg["n_agents"] and seg.length.tolist() == [N_STEPS] * cfg["B"]
        eng = seg.engine
        if name.startswith("pp4"):
            assert eng._persistent                                             # teams of 4: the one-launch route
        else:
            assert not eng._persistent and eng._fused is False                 # the two-launch route
        t0 = k * N_STEPS
        for n in _names(eng):
            extra = 1 if n in ("obs", "dist_adj", "channels") else 0           # these keep the state behind the last step too
            got = getattr(eng, n)[:N_STEPS + extra].cpu().numpy()
            assert got.tobytes() == long[n][t0:t0 + N_STEPS + extra].tobytes(), (name, use_graph, k, n)
        boot = seg.bootstrap()
        assert boot[0].cpu().numpy().tobytes() == long["obs"][t0 + N_STEPS].reshape(cfg["B"], -1).tobytes()
        assert (boot[1] is None) == ("dist_adj" not in long) and (boot[2] is None) == ("channels" not in long)
        if k < N_SEG - 1:                                                      # (rows come to the host for the last one only)
            tables.append(seg.episodes)
            first = first or seg
            continue
        row = seg[cfg["B"] - 1]
        assert set(row) == {"observations", "actions", "rewards", "dones", "dist_adjs", "channels"}
        assert np.array_equal(row["rewards"], long["reward64"][t0:t0 + N_STEPS, -1]) and row["observations"].shape[0] == N_STEPS
        assert np.array_equal(row["dones"], long["done"][t0:t0 + N_STEPS, -1].astype(bool))
        tables.append(seg.episodes)
    with pytest.raises(RuntimeError, match="earlier rollout"):                  # a batch of an earlier call refuses the buffers
        first.bootstrap()
    with pytest.raises(RuntimeError, match="earlier rollout"):                  # (no host copy was made while it was current)
        first[1]
    assert seg[0] is seg[0] and len(seg[:3]) == 3                               # the current one: one dict per env, built once
    # episodes end inside segments and across their borders
    done = long["done"].astype(bool)
    ends = np.nonzero(done)[0]
    assert len(ends) and (ends % N_STEPS != N_STEPS - 1).any() and (long["path_len"][done] > (ends % N_STEPS) + 1).any()
    eps, _ = R.episodes(long["reward64"], done, long["details"], long["success"], GAMMA)
    want = R.episode_table(eps)
    got = {c: sum(t[c] for t in tables) for c in L.SEG_COLUMNS}
    got["ret_min"], got["ret_max"] = min(t["ret_min"] for t in tables), max(t["ret_max"] for t in tables)
    assert want["count"] >= cfg["B"] * 2
    for c in ("count", "ret_min", "ret_max", "len_sum", "success") + tuple(f"details_{j}" for j in range(5)):
        assert got[c] == want[c], (c, got[c], want[c])
    for c in ("ret_sum", "ret_sumsq", "disc_sum"):
        assert abs(got[c] - want[c]) <= 1e-12 * abs(want[c]), (c, got[c], want[c])
    # a restart resets the envs and the episode records (the sampler's Philox base goes on: other draws than the first time)
    seg = smp.obtain_segments(9, N_STEPS, use_graph=use_graph, restart=True)
    assert seg.episodes["len_sum"] <= N_STEPS * seg.episodes["count"]
    open_len = smp._seg[3][1][0].cpu().numpy()
    assert ((open_len == N_STEPS) == ~seg.engine.done[:N_STEPS].cpu().numpy().astype(bool).any(0)).all()


def test_obtain_samples_in_between_resets_the_segments(gpu):
    """An obtain_samples resets the envs: the next obtain_segments starts from a reset of its own, with fresh episode records."""
    torch = gpu
    from com_marl_amd.sampler import CentralizedMAOnPolicyVectorizedSampler
    cfg = SETUPS["pp4_64envs"]
    env, pol = _make(torch, **cfg)
    algo = types.SimpleNamespace(policy=pol, discount=GAMMA, max_path_length=9, _segment_steps=None)
    smp = CentralizedMAOnPolicyVectorizedSampler(algo, env, n_envs=cfg["B"])
    smp.start_worker()
    smp.obtain_segments(0, N_STEPS)
    a = smp.obtain_segments(1, N_STEPS)
    assert smp._seg[3][1][0].max().item() > 0 or a.episodes["count"] > 0       # (open episodes are carried)
    paths = smp.obtain_samples(2, batch_size=cfg["B"] * cfg["n_agents"] * 9)
    assert len(paths) >= cfg["B"]
    b = smp.obtain_segments(3, N_STEPS)
    # 7 steps from a reset with max_env_steps = 9: an episode that ended is at most 7 steps long, and none carries over
    assert b.episodes["len_sum"] <= 7 * b.episodes["count"]
    rec_len = smp._seg[3][1][0].cpu().numpy()
    done = b.engine.done[:N_STEPS].cpu().numpy().astype(bool)
    assert ((rec_len == N_STEPS) == ~done.any(0)).all()
    algo._segment_steps = N_STEPS                                               # the switch: obtain_samples answers with segments
    c = smp.obtain_samples(4, batch_size=123)
    assert type(c).__name__ == "SegmentBatch" and c.n_steps == N_STEPS
