"""The policy-set forward for Comm-DP nets of any - also mixed - layer sizes in the engine and the evaluation entry points: a
nets.PolicySet(..., any_sizes=True) of differently sized members steps with ONE forward launch for the set (RolloutEngine
multi_forward == "set", cm_policy_forward_any_multi) and every member plays - bit for bit - what it plays in a single-policy
engine on a batch that starts at its first env; eval_models_co and eval_sweep return per policy what they return for it alone."""
import numpy as np
import pytest

from tests import any_set_members as M
from tests import conditions_common as cc

pytestmark = pytest.mark.gpu

H = 12                    # steps per chunk; two chunks per run
MPL = 6                   # episode limit: every env auto-resets inside a chunk
BUFS = ("obs", "actions", "probs", "attn", "reward", "reward64", "done", "details", "prey_alive", "success", "path_len",
        "dist_adj", "channels")


def _params(scen, map_, sen, N, n_preys, loss=0.0, rcom=9, mpl=MPL, hops=2, load=2):
    pp = scen == "pp"
    return dict(load=load, max_env_steps=mpl, capture_reward=10 if pp else 2, step_cost=0.1 if pp else 0, rm=0,
                penalty=0 if pp else 1, revisit_penalty=0.5, lazy_penalty=1, grid_size=map_, Rsen=sen, n_agents=N,
                n_preys=n_preys, n_gcn_layers=hops, mode="train", trRcom=rcom, trpl=loss, obstComplex="Easy", add_clock=0)


CO_MAP20 = ("co", _params("co", 20, 2, 24, 0))
PP_MAP10 = ("pp", _params("pp", 10, 1, 4, 4, loss=0.3, rcom=3))       # teams of 4, range-limited adjacency + IID loss


def _env(scen, params, B, off):
    from com_marl_amd import envs as E
    return E.GridEnvBatch(scen, params, B, device="cuda:0", seed=3, env_id_offset=off,
                          max_steps=MPL if scen == "pp" else 400, max_path_length=params["max_env_steps"])


def _members(env, fams, seed0=60):
    """One member per name: a family of any_set_members, or "default" (the default layer sizes); seeded by position."""
    out = []
    for k, f in enumerate(fams):
        if f == "default":
            out.append(M.build_default(env.N, env.d, env.Lh, seed=seed0 + k, rng_seed=3))
        else:
            out.append(M.build(f, env.N, env.d, env.Lh, seed=seed0 + k, rng_seed=3))
    return out


def _snap(eng):
    return {k: getattr(eng, k).cpu().numpy() for k in BUFS if getattr(eng, k) is not None}


def _two_chunks(torch, eng, greedy, h):
    """Two h-step chunks (each followed by its tail: slot h -> slot 0, Philox base += h); host copies of every buffer after each."""
    eng.policy.sync_weights()
    eng.reset()
    snaps = []
    for _ in range(2):
        if not eng.steps_fused(0, h, greedy=greedy, tail=True):
            eng.fork()
            for t in range(h):
                eng.step(t, greedy=greedy)
            eng.join()
            eng._chunk_tail(0, h)
        torch.cuda.synchronize()
        eng.env.check_status()
        snaps.append(_snap(eng))
    return snaps


def _check_groups(torch, case, fams, sizes, greedy, forward, h=H, off=5):
    from com_marl_amd import nets
    from com_marl_amd.rollout import RolloutEngine
    scen, params = case
    env = _env(scen, params, sum(sizes), off)
    pols = _members(env, fams)
    eng = RolloutEngine(env, nets.PolicySet(pols, any_sizes=True), h, groups=sizes)
    got = _two_chunks(torch, eng, greedy, h)
    assert (eng.multi_form, eng.multi_forward) == ("loop", forward)
    for k, (lo, hi) in enumerate(eng.groups):
        ref_eng = RolloutEngine(_env(scen, params, hi - lo, off + lo), pols[k], h)
        ref = _two_chunks(torch, ref_eng, greedy, h)
        for c in range(2):
            assert set(ref[c]) == set(got[c])
            for name, r in ref[c].items():
                np.testing.assert_array_equal(got[c][name][:, lo:hi], r, err_msg=f"policy {k}, chunk {c}, {name}")
    if h >= 2 * MPL:
        assert got[0]["done"].any(0).all()                # every env ended an episode (and restarted) inside the first chunk
    if not greedy:
        assert not np.array_equal(got[0]["actions"], got[1]["actions"])
    return got


@pytest.mark.parametrize("greedy", [True, False])
def test_mixed_set_takes_one_forward_launch_and_equals_per_policy_runs(greedy):
    import torch
    _check_groups(torch, CO_MAP20, ["m0", "m1", "m2"], [3, 1, 3], greedy, "set")


@pytest.mark.parametrize("greedy", [True, False])
def test_teams_of_4_are_covered(greedy):
    """Groups that start on multiples of 16 envs and off them: no wave form is picked from member 0 for a mixed set."""
    import torch
    _check_groups(torch, PP_MAP10, ["m0", "m1", "m0"], [5, 16, 3], greedy, "set")


def test_checkpoints_of_one_non_default_shape_take_the_set_kernel_only_with_the_keyword():
    import torch
    from com_marl_amd import nets
    from com_marl_amd.rollout import RolloutEngine
    scen, params = CO_MAP20
    _check_groups(torch, CO_MAP20, ["m0", "m0", "m0"], [2, 3, 1], False, "set", h=4)
    env = _env(scen, params, 4, 0)
    eng = RolloutEngine(env, nets.PolicySet(_members(env, ["m0", "m0"])), 4, groups=[2, 2])
    _two_chunks(torch, eng, False, 4)
    assert (eng.multi_form, eng.multi_forward) == ("loop", "member")


def test_a_default_sized_member_sends_the_set_member_by_member():
    import torch
    _check_groups(torch, CO_MAP20, ["default", "m0"], [3, 2], False, "member", h=6)


def test_members_with_their_own_seeds_step_member_by_member():
    from com_marl_amd import nets
    from com_marl_amd.rollout import RolloutEngine
    scen, params = CO_MAP20
    env = _env(scen, params, 4, 0)
    pols = _members(env, ["m0", "m1"])
    pols[1].set_rng(4)                                   # one launch keys one Philox stream
    eng = RolloutEngine(env, nets.PolicySet(pols, any_sizes=True), 4, groups=[2, 2])
    assert (eng.multi_form, eng.multi_forward) == ("loop", "member")


def test_captured_chunk_equals_eager_stepping_and_replays_draw_afresh():
    import torch
    from com_marl_amd import nets
    from com_marl_amd.rollout import RolloutEngine
    scen, params = CO_MAP20
    sizes, h = [3, 1, 3], H
    pols = _members(_env(scen, params, 1, 0), ["m0", "m1", "m2"])
    ps = nets.PolicySet(pols, any_sizes=True)
    runs = {}
    for use_graph in (True, False):
        eng = RolloutEngine(_env(scen, params, sum(sizes), 5), ps, h, groups=sizes)
        eng.reset()
        snaps = []
        for _ in range(2):
            eng.run_chunk(use_graph=use_graph)
            torch.cuda.synchronize()
            eng.env.check_status()
            snaps.append(_snap(eng))
        assert (eng.multi_form, eng.multi_forward) == ("loop", "set")
        assert int(eng.step_base.item()) == 2 * h
        runs[use_graph] = snaps
    for c in range(2):
        for name, r in runs[False][c].items():
            np.testing.assert_array_equal(runs[True][c][name], r, err_msg=f"chunk {c}, {name}")
    assert not np.array_equal(runs[True][0]["actions"], runs[True][1]["actions"])


def test_weights_changed_in_place_are_read_without_rebuilding_the_table():
    import torch
    from com_marl_amd import nets
    from com_marl_amd.rollout import RolloutEngine
    scen, params = CO_MAP20
    sizes, h, off = [3, 1, 3], 6, 5
    pols = _members(_env(scen, params, 1, 0), ["m0", "m1", "m2"])
    ps = nets.PolicySet(pols, any_sizes=True)
    eng = RolloutEngine(_env(scen, params, sum(sizes), off), ps, h, groups=sizes)
    before = _two_chunks(torch, eng, False, h)
    table = ps.forward_table(sizes)[0]
    assert table is not None
    with torch.no_grad():
        for p in pols[2].parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=torch.Generator().manual_seed(9)).to(p.device))
    eng2 = RolloutEngine(_env(scen, params, sum(sizes), off), ps, h, groups=sizes)
    after = _two_chunks(torch, eng2, False, h)             # (sync_weights() refreshes the flat copies in place)
    assert ps.forward_table(sizes)[0] is table and eng2.multi_forward == "set"
    lo = sizes[0] + sizes[1]
    assert not np.array_equal(after[1]["probs"][:, lo:], before[1]["probs"][:, lo:])
    for k, (lo, hi) in enumerate(eng2.groups):
        ref = _two_chunks(torch, RolloutEngine(_env(scen, params, hi - lo, off + lo), pols[k], h), False, h)
        for c in range(2):
            for name, r in ref[c].items():
                np.testing.assert_array_equal(after[c][name][:, lo:hi], r, err_msg=f"policy {k}, chunk {c}, {name}")


def test_eval_models_co_takes_the_set_forward(monkeypatch):
    from com_marl_amd import envs as E, evaluate, nets
    from com_marl_amd.evaluate import eval_model_co, eval_models_co
    params = _params("co", 20, 2, 24, 0, mpl=8)
    K, Bk = 3, 3
    wrap = lambda n, off: E.CoverageWrapper(True, params=params, n_envs=n, device="cuda:0", seed=3, env_id_offset=off)   # noqa: E731
    env = wrap(K * Bk, 0)
    pols = _members(env.batch, ["m0", "m1", "m2"])
    used = []

    class Recording(evaluate.RolloutEngine):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            used.append(self)

    monkeypatch.setattr(evaluate, "RolloutEngine", Recording)
    got = eval_models_co(env, nets.PolicySet(pols, any_sizes=True), 0, n_eval_episodes=4, max_env_steps=8)
    assert len(used) == 1 and (used[0].multi_form, used[0].multi_forward) == ("loop", "set")
    for k in range(K):
        ref = eval_model_co(wrap(Bk, k * Bk), pols[k], 0, n_eval_episodes=4, max_env_steps=8)
        assert got[k] == ref, f"policy {k}"


def test_eval_sweep_cells_equal_eval_summary_per_policy():
    from com_marl_amd import envs as E_, nets
    from com_marl_amd.evaluate import eval_summary, eval_sweep
    T, E, N_EPI, OFF = 10, 4, 6, 5                         # 6 episodes of 4 envs: a second round that takes 2
    params = cc.base_params("co", 20, 2, 24, 0, max_env_steps=T)
    conds = [dict(Rcom=3, Pgb=0.05, Pbg=0.3), dict(Rcom=19, Pgb=0.9, Pbg=0.9)]
    wrap = lambda p, n, **kw: E_.CoverageWrapper(True, params=p, n_envs=n, device="cuda:0", seed=3, env_id_offset=OFF,   # noqa: E731
                                                 channel="GE", **kw)
    K, Cn = 3, len(conds)
    env = wrap(params, K * Cn * E, conditions=conds)
    pols = _members(env.batch, ["m0", "m1", "m2"])
    got = eval_sweep(env, nets.PolicySet(pols, any_sizes=True), 0, n_eval_episodes=N_EPI, max_env_steps=T, paired=True,
                     comm_stats=True)
    assert len(got) == K and all(len(row) == Cn for row in got)
    for k in range(K):
        for c in range(Cn):
            w = wrap(cc.with_condition(params, conds[c]), E)
            ref = eval_summary(w, pols[k], 0, n_eval_episodes=N_EPI, max_env_steps=T, comm_stats=True)
            assert set(got[k][c]) == set(ref) | {"condition"} and got[k][c]["condition"] == conds[c]
            for key, v in ref.items():
                assert got[k][c][key] == v, f"policy {k}, condition {c}: {key}: {got[k][c][key]!r} != {v!r}"
    # the conditions and the members bite
    assert any(got[0][0][key] != got[0][1][key] for key in ("reward", "nodeDeg", "delivery", "reach"))
    assert any(got[0][0][key] != got[1][0][key] for key in ("reward", "success", "step_cnt", "variable"))
