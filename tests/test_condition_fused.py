"""Per-env comm conditions in the wave-owned rollout of teams of 4 (csrc/cm_rollout_wc.hip, GridEnvBatch(fused_conditions=True)).

Yardstick: the two-launch path on the same kind of handle.  Every case builds its conditions batch twice - same seed, table and
policies, one with fused_conditions=True - plays both with RolloutEngine and compares every buffer and get_state() with
assert_array_equal.  The first case of each kernel also compares every condition's slice against an engine over the uniform batch
W_c (tests/conditions_common.py, the scheme of tests/test_condition_rollout.py).  Each case asserts the route that ran on either
side and that its inputs bite: every env auto-resets, node degrees differ between ranges, a pl = 0.9 slice loses most links, a
slice differs from its neighbouring condition's."""
import numpy as np
import pytest

from tests import conditions_common as cc
from tests.test_condition_rollout import BUFS, _play, _policies

pytestmark = pytest.mark.gpu

OFF = 7
IID3 = [dict(Rcom=9, pl=0), dict(Rcom=1, pl=0.9), dict(Rcom=3, pl=0.5)]
PP10 = cc.base_params("pp", 10, 1, 4, 4)


def _engine(env, pols, H, groups=None, **kw):
    from com_marl_amd import nets
    from com_marl_amd.rollout import RolloutEngine
    if len(pols) == 1:
        return RolloutEngine(env, pols[0], H, **kw)
    return RolloutEngine(env, nets.PolicySet(pols), H, groups=groups, **kw)


def _with_state(bufs, env):
    bufs.update({"state." + k: v for k, v in env.get_state().items()})
    return bufs


def _assert_same(got, ref, what):
    assert set(got) == set(ref), what
    for name in ref:
        np.testing.assert_array_equal(got[name], ref[name], err_msg=f"{what}: {name}")


def _twins(scen, params, channel, conds, B, H, *, K=1, groups=None, cond_of=None, ids=None, greedy=False, fused_route=True,
           **engine_kw):
    """The conditions batch twice, fused and not, played with the same policies.  -> (fused buffers, envs, policies).  Asserts the
    routes and the equality of every buffer and of get_state()."""
    if cond_of is None:
        cond_of = np.repeat(np.arange(len(conds)), B // len(conds))
    kw = dict(conditions=conds, condition_of=cond_of, rng_ids=ids)
    env_f = cc.make_batch(scen, params, B, OFF, channel, fused_conditions=True, **kw)
    env_u = cc.make_batch(scen, params, B, OFF, channel, **kw)
    assert env_f.fused_conditions is True and env_u.fused_conditions is False
    pols = _policies(env_f, K)
    eng_f, eng_u = _engine(env_f, pols, H, groups, **engine_kw), _engine(env_u, pols, H, groups)
    got = _with_state(_play(eng_f, H, greedy), env_f)
    ref = _with_state(_play(eng_u, H, greedy), env_u)
    if K == 1:
        assert eng_f._fused is fused_route and eng_u._fused is False      # one launch for the chunk / two launches per step
    else:
        assert eng_f.multi_form == ("wave" if fused_route else "loop") and eng_u.multi_form == "loop"
    assert set(BUFS) - set(got) <= {"channels", "prey_alive"}             # (no channel model / no preys)
    _assert_same(got, ref, "fused against two launches")
    assert got["done"].any(0).all(), "every env must auto-reset at least once"
    return got, (env_f, env_u), pols


def _slices(cond_of):
    """Maximal runs of one condition: (lo, hi, condition)."""
    return [(lo, hi, c) for lo, hi, c, _ in cc.slices_of(cond_of, np.arange(len(cond_of)))]


def _assert_bites(got, cond_of, conds, full_at):
    """Node degrees differ between ranges, a pl = 0.9 slice loses most off-diagonal links, neighbouring slices differ."""
    sl = _slices(cond_of)
    deg = {}
    for lo, hi, c in sl:
        deg.setdefault(c, []).append(got["dist_adj"][:, lo:hi].sum(-1).mean())
    deg = {c: float(np.mean(v)) for c, v in deg.items()}
    by_range = sorted(range(len(conds)), key=lambda c: conds[c]["Rcom"])
    for a, b in zip(by_range, by_range[1:]):
        if conds[a]["Rcom"] != conds[b]["Rcom"]:
            assert deg[a] < deg[b], (conds[a], deg[a], conds[b], deg[b])
    for c in range(len(conds)):
        if conds[c]["Rcom"] + 1 >= full_at:
            assert deg[c] == 4.0
    for lo, hi, c in sl:
        if conds[c].get("pl") == 0.9:
            assert cc.offdiag_mean(got["channels"][:, lo:hi]) < 0.25      # expected 0.1
        if conds[c].get("pl") == 0:
            assert (got["channels"][:, lo:hi] == 1).all()
    for (lo, hi, _), (lo2, hi2, _) in zip(sl, sl[1:]):
        n = min(hi - lo, hi2 - lo2)
        assert any(not np.array_equal(got[k][:, lo:lo + n], got[k][:, lo2:lo2 + n]) for k in ("dist_adj", "channels", "obs") if k in got)


def _assert_cells_equal_uniform(got, scen, params, channel, conds, pols, H, greedy, K, E, paired):
    """Every (policy, condition) cell against an engine over the uniform batch W_c (the scheme of test_condition_rollout)."""
    from com_marl_amd.rollout import RolloutEngine
    Cn = len(conds)
    for k in range(K):
        for c in range(Cn):
            lo = (k * Cn + c) * E
            hi = lo + E
            full = conds[c]["Rcom"] + 1 >= params["grid_size"]
            w = cc.uniform_batch(scen, params, conds[c], E, OFF if paired else OFF + lo, channel)
            ref = _play(RolloutEngine(w, pols[k], H), H, greedy)
            assert ("dist_adj" in ref) == (not full)
            for name in ref:
                np.testing.assert_array_equal(got[name][:, lo:hi], ref[name], err_msg=f"policy {k}, condition {c}, {name}")
            if full:
                assert (got["dist_adj"][:, lo:hi] == 1).all()


# ---- 1: map 10, two hops, B = 15: one ragged workgroup, condition borders inside a wave --------------------------------------
@pytest.mark.parametrize("greedy", [False, True], ids=["sampled_own_ids", "greedy_paired"])
def test_one_ragged_workgroup_borders_inside_a_wave(greedy):
    from com_marl_amd.evaluate import sweep_layout
    E, H, B = 5, 8, 15
    cond_of, ids = sweep_layout(B, 1, 3, OFF, greedy)                     # sampled: rng_ids = OFF + b; greedy: paired
    got, _, pols = _twins("pp", PP10, "IID", IID3, B, H, cond_of=cond_of, ids=ids, greedy=greedy)
    _assert_bites(got, cond_of, IID3, 10)
    _assert_cells_equal_uniform(got, "pp", PP10, "IID", IID3, pols, H, greedy, 1, E, greedy)


# ---- 2: full workgroups; one and two hops ------------------------------------------------------------------------------------
@pytest.mark.parametrize("hops, B", [(1, 48), (2, 48), (1, 21)], ids=["one_hop_full", "two_hops_full", "one_hop_ragged"])
def test_full_workgroups_and_one_hop(hops, B):
    params = dict(PP10, n_gcn_layers=hops)
    got, (env_f, _), _ = _twins("pp", params, "IID", IID3, B, 8)
    assert env_f.Lh == hops
    _assert_bites(got, env_f.condition_of, IID3, 10)


# ---- 3: Gilbert-Elliott channel: random initial state, one transition per step ------------------------------------------------
def test_gilbert_elliott_channel():
    conds = [dict(Rcom=2, Pgb=0.05, Pbg=0.3), dict(Rcom=9, Pgb=0.9, Pbg=0.05), dict(Rcom=1, Pgb=0.4, Pbg=0.1), dict(Rcom=3, Pgb=0.0, Pbg=1.0)]
    got, (env_f, _), _ = _twins("pp", PP10, "GE", conds, 40, 8)
    assert env_f.channelType == "GE"
    _assert_bites(got, env_f.condition_of, conds, 10)
    rate = [cc.offdiag_mean(got["channels"][1:, lo:hi]) for lo, hi, _ in _slices(env_f.condition_of)]
    assert rate[1] < rate[2] < rate[0] < rate[3] == 1.0, rate             # stationary good rates 0.05 < 0.2 < 0.86 < 1


# ---- 4: no channel model: adjacency only -------------------------------------------------------------------------------------
def test_no_channel_model():
    conds = [dict(Rcom=9), dict(Rcom=2), dict(Rcom=1), dict(Rcom=2)]
    got, (env_f, _), _ = _twins("pp", PP10, None, conds, 20, 8)
    assert env_f.channelType == "FC" and env_f.ch_const and "channels" not in got
    _assert_bites(got, env_f.condition_of, conds, 10)


# ---- 5: the plain (non-prefetch) builds: a grid side above 16.  Map 20 does not fit LDS; map 17 does beside the one-hop image --
PLAIN_CONDS = [dict(Rcom=16, pl=0), dict(Rcom=2, pl=0.9), dict(Rcom=5, pl=0.5), dict(Rcom=2, pl=0.9)]


@pytest.mark.parametrize("B", [20, 32], ids=["ragged", "full"])
def test_plain_builds(B):
    params = cc.base_params("pp", 17, 1, 4, 4, n_gcn_layers=1)
    got, (env_f, _), _ = _twins("pp", params, "IID", PLAIN_CONDS, B, 8)
    assert env_f.S == 17 and env_f.Lh == 1                               # env_prefetch_ok<CM_PP, 16> is false: S > 16
    _assert_bites(got, env_f.condition_of, PLAIN_CONDS, 17)


@pytest.mark.parametrize("map_, hops", [(17, 2), (20, 1)], ids=["map17_two_hops", "map20_one_hop"])
def test_grids_above_16_that_do_not_fit_lds_decline(map_, hops):
    params = cc.base_params("pp", map_, 1, 4, 4, n_gcn_layers=hops)
    conds = [dict(Rcom=map_ - 1, pl=0), dict(Rcom=2, pl=0.9)]
    got, _, _ = _twins("pp", params, "IID", conds, 20, 8, fused_route=False)
    _assert_bites(got, np.repeat([0, 1], 10), conds, map_)


def test_two_hop_plain_build_is_not_shipped(monkeypatch):
    """More than 8 preys give an env 64 lanes; forced to 16 (COMMARL_ENV_LPE, read by cm_env_create) 11 preys would want the
    two-hop plain build, which cm_rollout_wc.hip leaves out: a decline, and the two launches."""
    monkeypatch.setenv("COMMARL_ENV_LPE", "16")
    params = cc.base_params("pp", 10, 1, 4, 11)
    got, (env_f, _), _ = _twins("pp", params, "IID", IID3, 21, 8, fused_route=False)
    assert env_f.M == 11
    _assert_bites(got, env_f.condition_of, IID3, 10)


# ---- 6: a policy set: rollout_wcm_kernel -------------------------------------------------------------------------------------
def test_policy_set_whole_workgroups():
    from com_marl_amd.evaluate import sweep_layout
    K, Cn, E, H = 2, 2, 8, 8
    conds = IID3[:2]
    cond_of, ids = sweep_layout(K * Cn * E, K, Cn, OFF, True)
    got, _, pols = _twins("pp", PP10, "IID", conds, K * Cn * E, H, K=K, groups=[Cn * E] * K, cond_of=cond_of, ids=ids, greedy=True)
    _assert_bites(got, cond_of, conds, 10)
    _assert_cells_equal_uniform(got, "pp", PP10, "IID", conds, pols, H, True, K, E, True)
    assert not np.array_equal(got["actions"][:, :16], got["actions"][:, 16:])      # two policies on paired episodes


@pytest.mark.parametrize("map_, hops, groups", [(10, 2, [32, 23]), (10, 1, [32, 23]), (17, 1, [32, 23]), (10, 1, [16, 16]), (17, 1, [16, 16])],
                         ids=["prefetch_two_hops_ragged", "prefetch_one_hop_ragged", "plain_one_hop_ragged", "prefetch_one_hop_full",
                              "plain_one_hop_full"])
def test_policy_set_other_builds(map_, hops, groups):
    """Groups of 32 with a ragged total (a uniform batch's set form allows a ragged last workgroup), and the one-hop builds."""
    params = cc.base_params("pp", map_, 1, 4, 4, n_gcn_layers=hops)
    B = sum(groups)
    cond_of = (np.arange(B) // 3) % 3                                     # borders inside every wave, across the policies' border
    conds = [dict(Rcom=map_ - 1, pl=0), dict(Rcom=1, pl=0.9), dict(Rcom=3, pl=0.5)]
    got, _, _ = _twins("pp", params, "IID", conds, B, 8, K=2, groups=groups, cond_of=cond_of, greedy=True)
    _assert_bites(got, cond_of, conds, map_)


# ---- 7: single fused steps through cm_rollout_step ---------------------------------------------------------------------------
def test_single_steps_outside_a_chunk():
    import torch
    H, B = 8, 21
    kw = dict(conditions=IID3)
    env_f = cc.make_batch("pp", PP10, B, OFF, "IID", fused_conditions=True, **kw)
    env_u = cc.make_batch("pp", PP10, B, OFF, "IID", **kw)
    pols = _policies(env_f, 1)
    out = []
    for env in (env_f, env_u):
        eng = _engine(env, pols, H)
        pols[0].sync_weights()
        eng.reset()
        for t in range(H):
            eng.step(t)
        torch.cuda.synchronize()
        env.check_status()
        assert eng._fused is (env is env_f)                               # cm_rollout_step ran / declined
        out.append(_with_state({k: getattr(eng, k).cpu().numpy() for k in BUFS if getattr(eng, k) is not None}, env))
    _assert_same(out[0], out[1], "single fused steps against two launches")
    assert out[0]["done"].any(0).all()
    _assert_bites(out[0], env_f.condition_of, IID3, 10)


# ---- 8: set_conditions() between rollouts under graph replay -----------------------------------------------------------------
def test_set_conditions_between_replayed_spans():
    import torch
    H, B, span = 8, 21, 4
    later = [IID3[1], IID3[2], IID3[0]]
    envs = [cc.make_batch("pp", PP10, B, OFF, "IID", conditions=IID3, fused_conditions=f) for f in (True, False)]
    pols = _policies(envs[0], 1)
    engs = [_engine(env, pols, H) for env in envs]

    def rollout(eng):                                                     # the sampler's spans: one captured graph per (t0, n)
        eng.policy.sync_weights()
        eng.reset()
        for t0 in range(0, H, span):
            eng.run_span(t0, span)
        torch.cuda.synchronize()
        eng.env.check_status()
        return _with_state({k: getattr(eng, k).cpu().numpy() for k in BUFS if getattr(eng, k) is not None}, eng.env)

    first = [rollout(e) for e in engs]
    assert engs[0]._fused is True and engs[1]._fused is False
    graphs = [dict(e._graphs) for e in engs]
    assert sorted(graphs[0]) == [(0, span, False), (span, span, False)]
    _assert_same(first[0], first[1], "first rollout")
    for env in envs:
        env.set_conditions(later)
    second = [rollout(e) for e in engs]
    assert all(e._graphs == g for e, g in zip(engs, graphs))              # replayed, not captured again
    _assert_same(second[0], second[1], "second rollout")
    for got, conds in ((first[0], IID3), (second[0], later)):
        _assert_bites(got, envs[0].condition_of, conds, 10)
    lo, hi = 0, B // 3                                                    # slice 0: fully connected and lossless, then Rcom 1 / pl 0.9
    assert (first[0]["channels"][:, lo:hi] == 1).all() and cc.offdiag_mean(second[0]["channels"][1:, lo:hi]) < 0.25
    assert (first[0]["dist_adj"][:, lo:hi] == 1).all() and not (second[0]["dist_adj"][1:, lo:hi] == 1).all()


# ---- 9: declines stay declines -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scen, params, channel, conds, B", [
    ("co", cc.base_params("co", 20, 2, 24, 0), "GE", [dict(Rcom=3, Pgb=0.05, Pbg=0.3), dict(Rcom=19, Pgb=0.4, Pbg=0.1)], 4),
    ("pp", cc.base_params("pp", 10, 1, 9, 4), "IID", [dict(Rcom=9, pl=0), dict(Rcom=2, pl=0.9)], 12),
], ids=["co24", "pp9"])
def test_declines_stay_declines(scen, params, channel, conds, B):
    got, (env_f, _), _ = _twins(scen, params, channel, conds, B, 6, fused_route=False, fused=True)   # fused=True: the library is asked
    lo = B // 2
    assert got["dist_adj"][:, :lo].sum(-1).mean() != got["dist_adj"][:, lo:].sum(-1).mean()


# ---- 10: eval_sweep follows the handle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 1], ids=["policy_set", "one_policy"])
def test_eval_sweep_on_a_fused_wrapper(K):
    import torch
    from com_marl_amd import envs as E_, nets
    from com_marl_amd.evaluate import eval_sweep
    Cn, E, T, n_epi = 2, 8, 64, 12
    params = cc.base_params("pp", 10, 1, 4, 4, max_env_steps=T)
    conds = [dict(Rcom=9, pl=0), dict(Rcom=1, pl=0.9)]
    res, routes = [], []
    for fused in (True, False):
        env = E_.PredatorPreyWrapper(True, params=params, n_envs=K * Cn * E, device="cuda:0", seed=3, env_id_offset=OFF, channel="IID",
                                     conditions=conds, fused_conditions=fused)
        pols = []
        for k in range(K):
            torch.manual_seed(30 + k)
            p = nets.CommCategoricalMLPPolicy(env.spec, n_agents=4, n_gcn_layers=2, device="cuda:0")
            p.set_rng(3)
            pols.append(p)
        calls = []
        real = nets.CommCategoricalMLPPolicy.chunk_fused
        if K == 1:                                                        # which form the round took: the answer of chunk_fused
            def spy(self, *a, _real=real, **kw):
                calls.append(_real(self, *a, **kw))
                return calls[-1]
            nets.CommCategoricalMLPPolicy.chunk_fused = spy
        try:
            res.append(eval_sweep(env, pols if K > 1 else pols[0], 0, n_eval_episodes=n_epi, max_env_steps=T, paired=True, episodes=True))
        finally:
            nets.CommCategoricalMLPPolicy.chunk_fused = real
        routes.append(calls)
    if K == 1:
        assert routes[0] == [True, True] and routes[1] == [False]         # two rounds of one launch / asked once, then stepping
        res = [[r] for r in res]
    for k in range(K):
        for c in range(Cn):
            a, b = res[0][k][c], res[1][k][c]
            assert set(a) == set(b) and sum(isinstance(v, float) for v in a.values()) >= 12
            for key in a:
                if key == "episodes":
                    assert tuple(a[key].shape) == (n_epi, 9) and torch.equal(a[key], b[key])
                else:
                    assert a[key] == b[key], (k, c, key, a[key], b[key])
        assert any(res[0][k][0][key] != res[0][k][1][key] for key in ("reward", "success", "nodeDeg", "step_cnt"))
