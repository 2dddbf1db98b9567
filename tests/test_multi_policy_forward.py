"""The set forward (cm_policy_forward_multi, RolloutEngine.multi_forward == "set"): the acting forward + sample of every member
of a Comm-DP policy set in ONE launch, each member on its own contiguous envs, must equal - bit for bit - one cm_policy_forward
per member on its slice with env_id_offset + the slice's first env; at the C ABI, in the engine, through eval_models_co and
under a captured hipGraph."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H = 50                    # steps per chunk; two chunks per run
MPL = 9                   # episode limit: every env auto-resets inside a chunk
BUFS = ("obs", "actions", "probs", "attn", "reward", "reward64", "done", "details", "prey_alive", "success", "path_len",
        "dist_adj", "channels")
GUARD = 64                # elements of guard band on either side of every output


def _pick_epb(N):
    """Envs per workgroup of the workgroup-tiled forward (csrc/cm_policy_mfma_dev.h pick_epb)."""
    if N % 4:
        return 1
    return max(1, ((2 * N) if 16 < N < 32 else 32) // N)


def _nets(N, d, K, hops=2, seed0=20):
    import torch
    from com_marl_amd import envs as E, nets
    spec = E.EnvSpec(E._Box(np.zeros(d * N), np.ones(d * N)), E._Discrete(5))
    out = []
    for k in range(K):
        torch.manual_seed(seed0 + k)
        p = nets.CommCategoricalMLPPolicy(spec, n_agents=N, n_gcn_layers=hops, device="cuda:0")
        p.set_rng(11)
        out.append(p)
    return out


def _guarded(torch, shape, dtype, fill):
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda:0")
    return flat, flat[GUARD:GUARD + n].view(*shape)


# (N, d, the family the shape must reach: KH = d rounded up to 32, MAXMK / waves by team size)
ABI_SHAPES = [(24, 77, "KH 96, MAXMK 25"), (72, 53, "KH 64, 8 waves"), (54, 77, "KH 96, 8 waves"), (8, 21, "KH 32, MAXMK 0"),
              (5, 40, "KH 64, MAXMK 0, one env per workgroup")]


@pytest.mark.parametrize("masks", ["const", "explicit"])
@pytest.mark.parametrize("greedy", [True, False])
@pytest.mark.parametrize("N,d,family", ABI_SHAPES, ids=[f"N{s[0]}_d{s[1]}" for s in ABI_SHAPES])
def test_one_launch_equals_a_launch_per_member(N, d, family, greedy, masks):
    import torch
    from com_marl_amd import _lib as L, nets
    epb, A, Lh, K, off, step = _pick_epb(N), 5, 2, 3, 1000, 7
    sizes = [2 * epb + 1, 1, 3 * epb + 1]                             # a group of 1; with epb > 1 every group ends ragged
    if epb > 1:
        assert all(s % epb for s in sizes)
    S = sum(sizes)
    pols = _nets(N, d, K)
    ps = nets.PolicySet(pols)
    ps.sync_weights()
    g = torch.Generator(device="cpu").manual_seed(5)
    obs = torch.rand(S, N, d, generator=g).cuda()
    adj = ch = None
    if masks == "explicit":
        eye = torch.eye(N)
        adj = torch.maximum((torch.rand(S, N, N, generator=g) < 0.6).float(), eye).cuda()
        ch = (torch.rand(S, Lh, N, N, generator=g) < 0.7).float().cuda()
    base = torch.full((1,), 1000, dtype=torch.int32, device="cuda:0")

    ref_a, ref_p, ref_m = [], [], []
    lo = 0
    for k, n in enumerate(sizes):
        a, p, m = pols[k].act_device(obs[lo:lo + n], None, None if adj is None else adj[lo:lo + n],
                                     None if ch is None else ch[lo:lo + n], greedy=greedy, policy_step=step, step_base=base,
                                     env_id_offset=off + lo)
        ref_a.append(a); ref_p.append(p); ref_m.append(m)
        lo += n
    ref_a, ref_p, ref_m = (torch.cat(x).cpu().numpy() for x in (ref_a, ref_p, ref_m))

    table, n_wg = ps.forward_table(sizes)
    assert table is not None and n_wg == sum(-(-n // epb) for n in sizes), family
    fa, act = _guarded(torch, (S, N), torch.int32, -7)
    fp, probs = _guarded(torch, (S, N, A), torch.float32, float("nan"))
    fm, attn = _guarded(torch, (S, N, N), torch.float32, float("nan"))
    w = pols[0]._weights_struct()
    rc = L.lib().cm_policy_forward_multi(C.byref(w), L.ptr(table), n_wg, S, L.ptr(obs), None, L.ptr(adj), L.ptr(ch), 11, off, step,
                                         L.ptr(base), int(greedy), L.ptr(act), L.ptr(probs), L.ptr(attn), L.current_stream())
    assert rc == 0, (rc, L.lib().cm_last_error())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(act.cpu().numpy(), ref_a)
    np.testing.assert_array_equal(probs.cpu().numpy(), ref_p)
    np.testing.assert_array_equal(attn.cpu().numpy(), ref_m)
    assert not np.isnan(ref_p).any() and not np.isnan(ref_m).any() and (ref_a >= 0).all()
    for flat, fill in ((fa, -7), (fp, None), (fm, None)):
        for band in (flat[:GUARD], flat[-GUARD:]):
            b = band.cpu().numpy()
            assert np.isnan(b).all() if fill is None else (b == fill).all(), "guard band written"
    # the members really are different nets
    assert not torch.equal(next(pols[0].parameters()), next(pols[1].parameters()))


def test_teams_above_80_agents_have_no_set_kernel():
    import torch
    from com_marl_amd import _lib as L, nets
    pols = _nets(96, 77, 2)
    ps = nets.PolicySet(pols)
    ps.sync_weights()
    assert ps.forward_table([1, 1]) == (None, 0)
    w = pols[0]._weights_struct()
    assert w.mfma_pack
    obs = torch.rand(2, 96, 77, device="cuda:0")
    act = torch.full((2, 96), -7, dtype=torch.int32, device="cuda:0")
    dummy = torch.zeros(256, dtype=torch.uint8, device="cuda:0")
    rc = L.lib().cm_policy_forward_multi(C.byref(w), L.ptr(dummy), 2, 2, L.ptr(obs), None, None, None, 11, 0, 0, None, 1,
                                         L.ptr(act), None, None, L.current_stream())
    torch.cuda.synchronize()
    assert rc == 1 and (act == -7).all()                # "not for this shape": nothing launched


# ---- engine level: the shape of test_multi_policy_rollout._check_groups ----------------------------------------------
def _params(scen, map_, sen, N, M, loss=0.0, rcom=9, mpl=MPL, hops=2, load=2):
    pp = scen == "pp"
    return dict(load=load, max_env_steps=mpl, capture_reward=10 if pp else 2, step_cost=0.1 if pp else 0, rm=0,
                penalty=0 if pp else 1, revisit_penalty=0.5, lazy_penalty=1, grid_size=map_, Rsen=sen, n_agents=N,
                n_preys=M, n_gcn_layers=hops, mode="train", trRcom=rcom, trpl=loss, obstComplex="Easy", add_clock=0)


CO_MAP20 = ("co", _params("co", 20, 2, 24, 0, mpl=6))
PP_MAP30 = ("pp", _params("pp", 30, 2, 72, 72, load=4))
CO_MAP30_IID = ("co", _params("co", 30, 2, 54, 0, loss=0.3, rcom=3, mpl=6))       # IID loss, range-limited adjacency
PP_MAP40 = ("pp", _params("pp", 40, 2, 128, 128, load=4))                         # N = 128: the layer-by-layer forward


def _env(scen, params, B, off):
    from com_marl_amd import envs as E
    return E.GridEnvBatch(scen, params, B, device="cuda:0", seed=3, env_id_offset=off,
                          max_steps=MPL if scen == "pp" else 400, max_path_length=params["max_env_steps"])


def _policies(env, K, seed0=10):
    import torch
    from com_marl_amd import envs as E, nets
    spec = E.EnvSpec(E._Box(np.zeros(env.d * env.N), np.ones(env.d * env.N)), E._Discrete(5))
    out = []
    for k in range(K):
        torch.manual_seed(seed0 + k)
        p = nets.CommCategoricalMLPPolicy(spec, n_agents=env.N, n_gcn_layers=env.Lh, device="cuda:0")
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


def _check_groups(torch, case, sizes, greedy, forward, h=H, off=5):
    from com_marl_amd import nets
    from com_marl_amd.rollout import RolloutEngine
    scen, params = case
    env = _env(scen, params, sum(sizes), off)
    pols = _policies(env, len(sizes))
    eng = RolloutEngine(env, nets.PolicySet(pols), h, groups=sizes)
    got = _two_chunks(torch, eng, greedy, h)
    assert eng.multi_form == "loop"
    assert eng.multi_forward == forward
    for k, (lo, hi) in enumerate(eng.groups):
        ref_eng = RolloutEngine(_env(scen, params, hi - lo, off + lo), pols[k], h)
        assert ref_eng.multi_form is None and ref_eng.multi_forward is None
        ref = _two_chunks(torch, ref_eng, greedy, h)
        for c in range(2):
            assert set(ref[c]) == set(got[c])
            for name, r in ref[c].items():
                np.testing.assert_array_equal(got[c][name][:, lo:hi], r, err_msg=f"policy {k}, chunk {c}, {name}")


@pytest.mark.parametrize("greedy", [True, False])
@pytest.mark.parametrize("case,sizes", [(CO_MAP20, [3, 2, 4]), (PP_MAP30, [2, 1, 3]), (CO_MAP30_IID, [2, 3, 1])],
                         ids=["co_map20", "pp_map30", "co_map30_iid"])
def test_set_forward_equals_per_policy_runs(case, sizes, greedy):
    import torch
    _check_groups(torch, case, sizes, greedy, "set")


@pytest.mark.parametrize("greedy", [True, False])
def test_teams_of_128_step_member_by_member_and_still_match(greedy):
    import torch
    _check_groups(torch, PP_MAP40, [1, 2], greedy, "member", h=8)


def test_members_with_their_own_seeds_step_member_by_member():
    import torch
    from com_marl_amd import nets
    from com_marl_amd.rollout import RolloutEngine
    scen, params = CO_MAP20
    env = _env(scen, params, 4, 0)
    pols = _policies(env, 2)
    pols[1].set_rng(4)                                   # one launch keys one Philox stream
    eng = RolloutEngine(env, nets.PolicySet(pols), 4, groups=[2, 2])
    assert (eng.multi_form, eng.multi_forward) == ("loop", "member")
    _two_chunks(torch, eng, False, 4)
    assert eng.multi_forward == "member"


def test_eval_models_co_takes_the_set_forward(monkeypatch):
    from com_marl_amd import envs as E, evaluate
    from com_marl_amd.evaluate import eval_model_co, eval_models_co
    params = _params("co", 20, 2, 24, 0, mpl=8)
    K, Bk = 4, 3
    wrap = lambda n, off: E.CoverageWrapper(True, params=params, n_envs=n, device="cuda:0", seed=3, env_id_offset=off)   # noqa: E731
    env = wrap(K * Bk, 0)
    pols = _policies(env.batch, K)
    used = []

    class Recording(evaluate.RolloutEngine):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            used.append(self)

    monkeypatch.setattr(evaluate, "RolloutEngine", Recording)
    got = eval_models_co(env, pols, 0, n_eval_episodes=4, max_env_steps=8)
    assert len(used) == 1 and (used[0].multi_form, used[0].multi_forward) == ("loop", "set")
    for k in range(K):
        ref = eval_model_co(wrap(Bk, k * Bk), pols[k], 0, n_eval_episodes=4, max_env_steps=8)
        assert got[k] == ref, f"policy {k}"


def test_captured_chunk_equals_eager_stepping_and_replays_draw_afresh():
    import torch
    from com_marl_amd import nets
    from com_marl_amd.rollout import RolloutEngine
    scen, params = CO_MAP20
    sizes, h = [3, 2, 4], 12
    pols = _policies(_env(scen, params, 1, 0), len(sizes))
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
