"""The row-MLP set forward (cm_mlp_policy_forward_multi, RolloutEngine.multi_forward == "set" for Obs-DP / CENT sets): the acting
forward + mask + sample of every member of a DecCategoricalMLPPolicy / CentralizedCategoricalMLPPolicy set in ONE launch, each
member on its own contiguous envs, must equal - bit for bit - one cm_mlp_policy_forward per member on its slice with
env_id_offset + the slice's first env; at the C ABI, in the engine, through eval_models / eval_models_co and under a captured
hipGraph.  Every comparison is exact: a member's rows end in a ragged 32-row workgroup of their own, so the accumulation order of
each row is that of the member's own launch."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H = 12                    # steps per chunk; two chunks per run
MPL = 9                   # episode limit: every env auto-resets inside a chunk
BUFS = ("obs", "actions", "probs", "attn", "reward", "reward64", "done", "details", "prey_alive", "success", "path_len",
        "dist_adj", "channels")
GUARD = 64                # elements of guard band on either side of every output
ROWS = 32                 # rows per workgroup of the row-MLP kernels (csrc/cm_mlp.hip)


def _make(kind, spec, N, relu=False):
    import torch
    from com_marl_amd import nets
    cls = nets.DecCategoricalMLPPolicy if kind == "obsdp" else nets.CentralizedCategoricalMLPPolicy
    return cls(spec, n_agents=N, hidden_nonlinearity=torch.relu if relu else torch.tanh, device="cuda:0")


def _nets(kind, N, d, K, relu, seed0=20, rng=11):
    import torch
    from com_marl_amd import envs as E
    spec = E.EnvSpec(E._Box(np.zeros(d * N), np.ones(d * N)), E._Discrete(5))
    out = []
    for k in range(K):
        torch.manual_seed(seed0 + k)
        p = _make(kind, spec, N, relu)
        p.set_rng(rng)
        out.append(p)
    return out


def _guarded(torch, shape, dtype, fill):
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda:0")
    return flat, flat[GUARD:GUARD + n].view(*shape)


# (kind, N, d, group sizes in envs).  (4, 21): in_dim 21 / 84, below one 128-column chunk and no multiple of 16; (24, 77): CENT
# in_dim 1848 = 15 chunks with a ragged last one, and 120 logits = two column-tile rounds of the last layer.  Every member's rows
# end in a ragged workgroup, one group is a single env (Obs-DP N = 4: 36 / 4 / 68 rows).
ABI_CASES = [("obsdp", 4, 21, [9, 1, 17]), ("obsdp", 24, 77, [3, 1, 2]), ("cent", 4, 21, [33, 1, 40]), ("cent", 24, 77, [33, 1, 40])]


@pytest.mark.parametrize("avail", ["none", "explicit"])
@pytest.mark.parametrize("greedy", [True, False])
@pytest.mark.parametrize("act", ["tanh", "relu"])
@pytest.mark.parametrize("kind,N,d,sizes", ABI_CASES, ids=[f"{c[0]}_N{c[1]}_d{c[2]}" for c in ABI_CASES])
def test_one_launch_equals_a_launch_per_member(kind, N, d, sizes, act, greedy, avail):
    import torch
    from com_marl_amd import _lib as L, nets
    A, K, off, step = 5, 3, 1000, 7
    groups = 1 if kind == "obsdp" else N
    rows = [s * N // groups for s in sizes]
    assert all(r % ROWS for r in rows) and 1 in sizes and max(rows) > ROWS          # ragged ends, a single env, several blocks
    S = sum(sizes)
    pols = _nets(kind, N, d, K, act == "relu")
    assert pols[0].hidden_nonlinearity == act
    for p, q in ((pols[0], pols[1]), (pols[1], pols[2]), (pols[0], pols[2])):        # the members really are different nets
        assert all(not torch.equal(x, y) for x, y in zip(p.parameters(), q.parameters()) if x.dim() == 2)   # (biases start at 0)
    ps = nets.PolicySet(pols)
    ps.sync_weights()
    g = torch.Generator(device="cpu").manual_seed(5)
    obs = torch.rand(S, N * d, generator=g).cuda()
    av = None
    if avail == "explicit":
        av = (torch.rand(S, N, A, generator=g) < 0.5).float()
        av[..., 0] = torch.maximum(av[..., 0], (av.sum(-1) == 0).float())           # at least one action allowed per agent
        assert (av.sum(-1) >= 1).all() and (av == 0).any()
        av = av.cuda()
    base = torch.full((1,), 1000, dtype=torch.int32, device="cuda:0")

    ref_a, ref_p = [], []
    lo = 0
    for k, n in enumerate(sizes):
        a, p, _ = pols[k].act_device(obs[lo:lo + n], None if av is None else av[lo:lo + n], greedy=greedy, policy_step=step,
                                     step_base=base, env_id_offset=off + lo)
        ref_a.append(a); ref_p.append(p)
        lo += n
    ref_a, ref_p = (torch.cat(x).cpu().numpy() for x in (ref_a, ref_p))

    table, n_wg = ps.forward_table(sizes)
    assert table is not None and n_wg == sum(-(-r // ROWS) for r in rows)
    fa, actions = _guarded(torch, (S, N), torch.int32, -7)
    fp, probs = _guarded(torch, (S, N, A), torch.float32, float("nan"))
    w = pols[0]._mlp_struct()
    rc = L.lib().cm_mlp_policy_forward_multi(C.byref(w), L.ptr(table), n_wg, S, groups, A, N, L.ptr(obs), L.ptr(av), 11, off, step,
                                             L.ptr(base), int(greedy), L.ptr(actions), L.ptr(probs), L.current_stream())
    assert rc == 0, (rc, L.lib().cm_last_error())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(actions.cpu().numpy(), ref_a)
    np.testing.assert_array_equal(probs.cpu().numpy(), ref_p)
    assert not np.isnan(ref_p).any() and (ref_a >= 0).all() and (ref_a < A).all()
    for flat, fill in ((fa, -7), (fp, None)):
        for band in (flat[:GUARD], flat[-GUARD:]):
            b = band.cpu().numpy()
            assert np.isnan(b).all() if fill is None else (b == fill).all(), "guard band written"


# ---- engine level: the shape of test_multi_policy_forward._check_groups ------------------------------------------------------
def _params(scen, map_, sen, N, M, mpl=MPL):
    pp = scen == "pp"
    return dict(load=2, max_env_steps=mpl, capture_reward=10 if pp else 2, step_cost=0.1 if pp else 0, rm=0,
                penalty=0 if pp else 1, revisit_penalty=0.5, lazy_penalty=1, grid_size=map_, Rsen=sen, n_agents=N,
                n_preys=M, n_gcn_layers=2, mode="train", trRcom=9, trpl=0.0, obstComplex="Easy", add_clock=0)


PP_MAP10 = ("pp", _params("pp", 10, 1, 4, 4))
CO_MAP20 = ("co", _params("co", 20, 2, 24, 0))


def _env(scen, params, B, off):
    from com_marl_amd import envs as E
    return E.GridEnvBatch(scen, params, B, device="cuda:0", seed=3, env_id_offset=off,
                          max_steps=MPL if scen == "pp" else 400, max_path_length=params["max_env_steps"])


def _policies(batch, K, kind, seed0=10):
    import torch
    from com_marl_amd import envs as E
    spec = E.EnvSpec(E._Box(np.zeros(batch.d * batch.N), np.ones(batch.d * batch.N)), E._Discrete(5))
    out = []
    for k in range(K):
        torch.manual_seed(seed0 + k)
        p = _make(kind, spec, batch.N)
        p.set_rng(3)
        out.append(p)
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


def _check_groups(torch, case, kind, sizes, greedy, forward, pols=None, h=H, off=5):
    from com_marl_amd import nets
    from com_marl_amd.rollout import RolloutEngine
    scen, params = case
    env = _env(scen, params, sum(sizes), off)
    pols = pols or _policies(env, len(sizes), kind)
    eng = RolloutEngine(env, nets.PolicySet(pols), h, groups=sizes)
    assert (eng.multi_form, eng.multi_forward) == ("loop", forward)
    got = _two_chunks(torch, eng, greedy, h)
    assert (eng.multi_form, eng.multi_forward) == ("loop", forward)
    assert (got[0]["path_len"] > 0).any(0).all(), "an env did not end (and auto-reset) inside the chunk"
    for k, (lo, hi) in enumerate(eng.groups):
        ref_eng = RolloutEngine(_env(scen, params, hi - lo, off + lo), pols[k], h)
        assert ref_eng.multi_form is None and ref_eng.multi_forward is None
        ref = _two_chunks(torch, ref_eng, greedy, h)
        for c in range(2):
            assert set(ref[c]) == set(got[c])
            for name, r in ref[c].items():
                np.testing.assert_array_equal(got[c][name][:, lo:hi], r, err_msg=f"policy {k}, chunk {c}, {name}")


ENGINE_CASES = [(PP_MAP10, "obsdp", [5, 1, 11]), (PP_MAP10, "cent", [33, 1, 7]), (CO_MAP20, "obsdp", [3, 2, 4]),
                (CO_MAP20, "cent", [3, 2, 4])]


@pytest.mark.parametrize("greedy", [True, False])
@pytest.mark.parametrize("case,kind,sizes", ENGINE_CASES, ids=["pp_map10_obsdp", "pp_map10_cent", "co_map20_obsdp", "co_map20_cent"])
def test_set_forward_equals_per_policy_runs(case, kind, sizes, greedy):
    import torch
    _check_groups(torch, case, kind, sizes, greedy, "set")


@pytest.mark.parametrize("kind", ["obsdp", "cent"])
def test_members_with_their_own_seeds_step_member_by_member_and_still_match(kind):
    import torch
    sizes = [5, 1, 11]
    pols = _policies(_env(*PP_MAP10, 1, 0), len(sizes), kind)
    pols[1].set_rng(4)                                   # one launch keys one Philox stream
    _check_groups(torch, PP_MAP10, kind, sizes, False, "member", pols=pols)


@pytest.mark.parametrize("scen,kind", [("pp", "obsdp"), ("co", "cent")])
def test_eval_models_take_the_set_forward(monkeypatch, scen, kind):
    from com_marl_amd import envs as E, evaluate
    pp = scen == "pp"
    params = _params("pp", 10, 1, 4, 4, mpl=8) if pp else _params("co", 20, 2, 24, 0, mpl=8)
    cls = E.PredatorPreyWrapper if pp else E.CoverageWrapper
    one, many = (evaluate.eval_model, evaluate.eval_models) if pp else (evaluate.eval_model_co, evaluate.eval_models_co)
    K, Bk = 4, 3
    wrap = lambda n, off: cls(True, params=params, n_envs=n, device="cuda:0", seed=3, env_id_offset=off)   # noqa: E731
    env = wrap(K * Bk, 0)
    pols = _policies(env.batch, K, kind)
    used = []

    class Recording(evaluate.RolloutEngine):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            used.append(self)

    monkeypatch.setattr(evaluate, "RolloutEngine", Recording)
    got = many(env, pols, 0, n_eval_episodes=4, max_env_steps=8)
    assert len(used) == 1 and (used[0].multi_form, used[0].multi_forward) == ("loop", "set")
    for k in range(K):
        ref = one(wrap(Bk, k * Bk), pols[k], 0, n_eval_episodes=4, max_env_steps=8)
        assert got[k] == ref, f"policy {k}"


def test_captured_chunk_equals_eager_stepping_and_replays_draw_afresh():
    import torch
    from com_marl_amd import nets
    from com_marl_amd.rollout import RolloutEngine
    scen, params = PP_MAP10
    sizes, h = [5, 1, 11], H
    pols = _policies(_env(scen, params, 1, 0), len(sizes), "obsdp")
    ps = nets.PolicySet(pols)
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
    # the second replay starts from the slot the first one carried over and draws at Philox steps h .. 2h-1: were the base
    # not advanced on the device, a replay from the same observation would repeat the first chunk's draws
    a0, a1 = runs[True][0]["actions"], runs[True][1]["actions"]
    assert not np.array_equal(a0, a1)
