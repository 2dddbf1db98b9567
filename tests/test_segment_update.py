"""CentralizedMAPPO on rollout segments (segment_steps=...) on the GPU: the whole glue pinned against the whole-path update
where the two must coincide, the bootstrapped targets the minibatches get against the float64 reference, the update graphs'
reuse at constant shapes, the update statistics on segments, and the refusals."""
import numpy as np
import pytest

from tests import segments_ref as R

pytestmark = pytest.mark.gpu

GAMMA, LAM = 0.99, 0.97


@pytest.fixture
def gpu(monkeypatch):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need the MI355X")
    for k in ("COMMARL_SEGMENT_STEPS", "COMMARL_UPDATE_STATS", "COMMARL_TARGET_KL"):
        monkeypatch.delenv(k, raising=False)
    return torch


@pytest.fixture
def det_on(gpu):
    import com_marl_amd
    com_marl_amd.set_deterministic(True)
    yield gpu
    com_marl_amd.set_deterministic(None)


def _make(torch, scenario="pp", B=16, mpl=200, seed=5, **algo_kw):
    from com_marl_amd import envs as E, nets
    from com_marl_amd.algos import CentralizedMAPPO
    from com_marl_amd.sampler import CentralizedMAOnPolicyVectorizedSampler
    if scenario == "pp":
        params = dict(load=2, max_env_steps=mpl, capture_reward=10, step_cost=0.1, rm=0, penalty=0, grid_size=10, Rsen=1, n_agents=4,
                      n_preys=4, n_gcn_layers=2, mode="train", trRcom=9, trpl=0, seed=seed)
        env = E.PredatorPreyWrapper(centralized=True, params=params, n_envs=B, device="cuda:0")
    else:                                       # Coverage on a small map, a short range and a lossy channel: both masks are kept
        params = dict(load=2, max_env_steps=mpl, capture_reward=2, step_cost=0, rm=0, penalty=1, revisit_penalty=0.5, lazy_penalty=1,
                      grid_size=10, Rsen=1, n_agents=4, n_preys=0, n_gcn_layers=2, mode="train", trRcom=3, trpl=0.3, seed=seed)
        env = E.CoverageWrapper(centralized=True, params=params, n_envs=B, device="cuda:0", max_steps=mpl)
    torch.manual_seed(seed)
    N = env.n_agents
    pol = nets.CommCategoricalMLPPolicy(env.spec, n_agents=N, device="cuda:0")
    crit = nets.CommBaseCritic(env.spec, n_agents=N, device="cuda:0")
    pol.set_rng(seed)
    kw = dict(max_path_length=mpl, discount=GAMMA, positive_adv=False, gae_lambda=LAM, policy_ent_coeff=0.1, clip_grad_norm=7,
              optimization_n_minibatches=1, optimization_mini_epochs=3, device="cuda:0", entropy_method="regularized", center_adv=False,
              stop_entropy_gradient=False)
    kw.update(algo_kw)
    algo = CentralizedMAPPO(env_spec=env.spec, policy=pol, baseline=crit, **kw)
    smp = CentralizedMAOnPolicyVectorizedSampler(algo, env, n_envs=B)
    smp.start_worker()
    return env, pol, crit, algo, smp


def _state(net):
    return {k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}


def test_one_segment_per_episode_is_the_whole_path_update(det_on):
    """Coverage, max steps = n_steps = 8: every episode is exactly one segment, so the SegmentBatch and the PathBatch of two
    identically seeded setups hold the same batch - and one train_once on each must leave the same bits in both nets."""
    torch = det_on
    B, n = 48, 8
    kw = dict(scenario="co", B=B, mpl=n, optimization_n_minibatches=2)
    out = {}
    for mode in ("segments", "paths"):
        env, pol, crit, algo, smp = _make(torch, segment_steps=n if mode == "segments" else None, **kw)
        paths = smp.obtain_samples(0, batch_size=B * env.n_agents * n)
        assert type(paths).__name__ == ("SegmentBatch" if mode == "segments" else "PathBatch")
        done = paths.engine.done[:n].cpu().numpy()
        assert not done[:n - 1].any() and done[n - 1].all()                     # every episode ends with the time limit, none before
        assert len(paths) == B
        np.random.seed(7)
        algo.train_once(itr=0, paths=paths)
        env.batch.check_status()
        out[mode] = dict(pol=_state(pol), crit=_state(crit), stats=dict(algo.stats))
    for net in ("pol", "crit"):
        a, b = out["segments"][net], out["paths"][net]
        bad = [k for k in a if a[k].tobytes() != b[k].tobytes()]
        assert a.keys() == b.keys() and not bad, (net, bad)
    s, p = out["segments"]["stats"], out["paths"]["stats"]
    for k in ("NumTrajs", "EnvSteps", "MaxPathLength", "LossBefore", "LossAfter", "KL", "Entropy", "GradNorm", "AverageStepCount"):
        assert s[k] == p[k], (k, s[k], p[k])
    for k in ("AverageReturn", "StdReturn", "MaxReturn", "MinReturn", "SuccessRate", "AverageCaptureCount", "AverageMovingCount", "AveragePenaltyCount", "AverageVariable",
              "AverageVar2"):
        assert abs(s[k] - p[k]) <= 1e-9 * max(1.0, abs(p[k])), (k, s[k], p[k])
    assert abs(s["AverageDiscountedReturn"] - p["AverageDiscountedReturn"]) <= 1e-6 * max(1.0, abs(p["AverageDiscountedReturn"]))
    assert s["NumTrajs"] == B * 4 and s["EnvSteps"] == B * n


@pytest.mark.parametrize("center_adv", [False, True])
def test_the_minibatches_get_the_bootstrapped_targets(center_adv, gpu, monkeypatch):
    """PP map10, n_steps = 8 of episodes up to 200 steps long: nearly every row ends in a cut, so v_last carries the targets.  The
    reference is built from the engine's buffers and the critic's own forward over the segment and over bootstrap()."""
    torch = gpu
    B, n = 16, 8
    env, pol, crit, algo, smp = _make(torch, B=B, segment_steps=n, center_adv=center_adv)
    smp.obtain_samples(0)
    seg = smp.obtain_samples(1)                                                 # the second segment: behind a carry
    e = seg.engine
    rows = lambda b: None if b is None else b[:n].transpose(0, 1).contiguous()  # noqa: E731
    with torch.no_grad():
        val = algo._baseline_forward(rows(e.obs).reshape(B, n, -1), rows(e.dist_adj), rows(e.channels)).cpu().numpy()
        b_obs, b_adj, b_ch = seg.bootstrap()
        one = lambda x: None if x is None else x.unsqueeze(1)                   # noqa: E731
        v_last = algo._baseline_forward(one(b_obs), one(b_adj), one(b_ch)).reshape(B).cpu().numpy()
    rew, dones = e.reward64[:n].t().cpu().numpy(), e.done[:n].t().cpu().numpy().astype(bool)
    assert (~dones[:, -1]).sum() >= B // 2 and (np.abs(v_last) > 1e-6).all()
    coef = R.kernel_coefficients(GAMMA, LAM)
    adv64, ret64, terms = R.segment_targets(rew, dones, val, v_last, *coef)
    seen = {}
    inner = algo._minibatches

    def spy(batch, advantages, old_ll, distributed):
        seen.update(adv=advantages.cpu().numpy(), ret=batch[6].cpu().numpy(), val=batch[5].cpu().numpy(), valids=batch[4].cpu().numpy())
        return inner(batch, advantages, old_ll, distributed)
    monkeypatch.setattr(algo, "_minibatches", spy)
    np.random.seed(3)
    algo.train_once(itr=1, paths=seg)
    assert seen["val"].tobytes() == val.tobytes() and seen["valids"].tolist() == [n] * B
    assert seg.v_last.cpu().numpy().tobytes() == v_last.tobytes()
    e_ret = np.abs(seen["ret"] - ret64)
    assert (e_ret <= R.U * np.abs(ret64)).all()
    raw = seg.advantages.cpu().numpy()                                          # cm_segment_targets' output, before the normalisation
    bound = R.adv_bound(adv64, terms)
    print(f"\ncenter_adv={center_adv}: returns worst err/bound {np.max(e_ret / (R.U * np.abs(ret64))):.3f}, "
          f"advantages worst err/bound {np.max(np.abs(raw - adv64) / bound):.3f}")
    assert (np.abs(raw - adv64) <= bound).all()
    # without the bootstrap the targets would be others: the reference with v_last = 0 is rejected
    adv0, ret0, terms0 = R.segment_targets(rew, dones, val, np.zeros(B), *coef)
    assert (np.abs(raw - adv0) > R.adv_bound(adv0, terms0)).any() and (np.abs(seen["ret"] - ret0) > R.U * np.abs(ret0)).any()
    if not center_adv:
        assert seen["adv"].tobytes() == raw.tobytes()
    else:                                                                       # ONE normalisation over the whole batch
        want = R.adv_normalize(raw, 1e-8)
        m, s = float(raw.astype(np.float64).mean()), float(raw.astype(np.float64).std())
        assert (np.abs(seen["adv"] - want) <= R.U * (3 * np.abs(want) + 2 * abs(m) / s)).all()
        per_row = (raw - raw.mean(1, keepdims=True)) / np.sqrt(raw.var(1, keepdims=True) + 1e-8)
        assert np.abs(seen["adv"] - per_row).max() > 1e-3                       # not the per-path one
    assert algo.stats["EnvSteps"] == B * n and algo.stats["MaxPathLength"] == n


def test_update_graphs_are_captured_once_and_reused(gpu, monkeypatch):
    """Four segment epochs through train(): P and T never change, so the optimiser steps captured in the first epoch are
    replayed by every later one."""
    torch = gpu
    from com_marl_amd.dropin import SimpleRunner
    monkeypatch.setenv("COMMARL_UPDATE_GRAPH", "1")
    n_mb = 2
    env, pol, crit, algo, smp = _make(torch, B=16, segment_steps=8, optimization_n_minibatches=n_mb, center_adv=True)
    runner = SimpleRunner()
    runner.setup(algo, env)
    counts, inner = [], algo.train_once

    def train_once(*a, **k):
        out = inner(*a, **k)
        ug = algo._update_graphs
        counts.append((ug.captured, ug.reused, ug.broken))
        return out
    monkeypatch.setattr(algo, "train_once", train_once)
    np.random.seed(5)
    runner.train(n_epochs=4, batch_size=16 * 4 * 8)
    print(f"\n(captured, reused, broken) per epoch: {counts}")
    assert len(counts) == 4 and not any(c[2] for c in counts)
    assert counts[0][0] == n_mb and counts[0][1] == 0                           # mini-epoch 0 eager, mini-epoch 1 captures
    for prev, cur in zip(counts, counts[1:]):
        assert cur[0] == prev[0] and cur[1] == prev[1] + n_mb
    assert runner.total_env_steps == 4 * 16 * 8
    assert [h["EnvSteps"] for h in runner.history] == [16 * 8] * 4
    assert all(np.isfinite(h["LossAfter"]) for h in runner.history)


def test_update_statistics_and_the_kl_stop_run_on_segments(gpu):
    torch = gpu
    env, pol, crit, algo, smp = _make(torch, B=16, segment_steps=8, optimization_n_minibatches=2, optimization_mini_epochs=4,
                                      update_stats=True, target_kl=1e9, positive_adv=True, center_adv=True)
    for itr in range(2):
        seg = smp.obtain_samples(itr)
        np.random.seed(itr)
        algo.train_once(itr=itr, paths=seg)
        r = algo.update_rows
        assert len(r["n_valid"]) == 8 and r["stopped"].tolist() == [0.0] * 8 and (r["n_valid"] == 8 * 8).all()
        assert r["approx_kl"][0] < 1e-9 and r["minibatch"].tolist() == [0, 1] * 4
        assert algo.stats["PolicySteps"] == 8 and algo.stats["EnvSteps"] == 16 * 8
    # no episode of up to 200 steps ended within 16: NaN means, NumTrajs 0 - or, had one ended, finite ones
    if seg.episodes["count"] == 0:
        assert algo.stats["NumTrajs"] == 0 and np.isnan(algo.stats["AverageReturn"]) and np.isnan(algo.stats["StdReturn"])
    else:
        assert algo.stats["NumTrajs"] == int(seg.episodes["count"]) * 4 and np.isfinite(algo.stats["AverageReturn"])


def test_refusals_come_before_any_launch(gpu, monkeypatch):
    torch = gpu
    from com_marl_amd import _lib as L, dist, nets
    from tests.lib_spy import _Spy
    env, pol, crit, algo, smp = _make(torch, B=16)
    seg = smp.obtain_segments(0, 8)
    before = _state(pol)
    spy = _Spy(L.lib())
    monkeypatch.setattr(L, "lib", lambda: spy)
    # entropy_method='max' (an algo built without segment_steps - with it the constructor refuses already)
    env2, pol2, crit2, maxent, smp2 = _make(torch, B=16, entropy_method="max", stop_entropy_gradient=True, policy_ent_coeff=0.01)
    spy.calls.clear()
    with pytest.raises(NotImplementedError, match="cm_entropy_gae"):
        maxent.train_once(itr=0, paths=seg)
    # a distributed update
    with monkeypatch.context() as m:
        m.setattr(dist, "is_distributed", lambda: True)
        with pytest.raises(NotImplementedError, match="reduced over the ranks"):
            algo.train_once(itr=0, paths=seg)
    assert not spy.calls
    assert all(before[k].tobytes() == v.tobytes() for k, v in _state(pol).items())
    # the sampler's: n_steps and a PolicySet (the tape mode: tests/test_segments_cpu.py)
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError, match="n_steps"):
            smp.obtain_segments(1, bad)
    algo.policy = nets.PolicySet.__new__(nets.PolicySet)                        # (never initialised: the type decides)
    with pytest.raises(ValueError, match="PolicySet"):
        smp.obtain_segments(1, 8)
    algo.policy = pol
    assert not spy.calls
    # and the refused calls left the segments where they were: the next one goes on from the first
    nxt = smp.obtain_segments(1, 8)
    assert nxt.engine is seg.engine
    open_len = smp._seg[3][1][0].cpu().numpy()
    done = nxt.engine.done[:8].cpu().numpy().astype(bool)
    assert (open_len[~done.any(0)] >= 9).any() and open_len.max() <= 16
