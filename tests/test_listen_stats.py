"""cm_listen_stats and its reductions (csrc/cm_listen_stats.hip) through ctypes, envs.listen_stats, RolloutEngine.replay_probs and
eval_summary / eval_sweep with listen_stats=True, against the numpy float64 restatement (tests/listen_stats_ref.py).  Both sides
compute in f64 from the same f32 inputs: rtol = 1e-10 with atol = 1e-12 N per graph and 1e-12 on episode rows, means and curves
(the reasoning is in the restatement's docstring); the flip columns of graph rows are compared exactly; every comparison prints
the largest error it saw.  Repeated launches are compared bit for bit.

Shapes: every team-size class of the kernel (N = 1, 2, 3-4, 5-8 on 1 / 2 / 4 / 8 lanes per graph; N >= 9 on one wave per graph with
1 .. 4 rows per lane), N A % 4 == 0 on the 16-byte loads and the others on the one-float loads, A = 5 (the policies'), 2 and 8,
S = 37 and 130 so that the last group, wave and workgroup are ragged.

The replays are judged three ways: with the recorded channels they reproduce the engine's recorded probabilities bit for bit (so
the factual and the counterfactual side of every statistic come from one arithmetic); with the counterfactual channels they lie
within the acting forward's float64 bound (tests/test_acting_forward_f64.py: TAU, the log-probability rule) of
tests/f64_commnet.policy_forward; and they are, bit for bit, what act_device gives on materialised masks - which is how the
expected values of the end-to-end tests are formed."""
import numpy as np
import pytest

from tests import conditions_common as cc, f64_commnet as F, listen_stats_ref as R
from tests.lib_spy import spy as lib_spy  # noqa: F401  (the fixture: a recording proxy around _lib.lib())

pytestmark = pytest.mark.gpu

SENTINEL = -77.0
GUARD = 3                                                       # guard rows in front of and behind each output
TAU = 1e-5                                                      # tests/test_acting_forward_f64.py


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch


def _close(got, want, atol, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want)
    rel = err / np.maximum(np.abs(want), 1e-300)
    print(f"{what}: max |error| {err.max(initial=0.0):.3e}, max relative error {rel[np.abs(want) > atol].max(initial=0.0):.3e} "
          f"(rtol {R.RTOL:g}, atol {atol:g})")
    np.testing.assert_allclose(got, want, rtol=R.RTOL, atol=atol, err_msg=what)


def _dev(torch, x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _launch(torch, S, N, A, probs, mute, lossless, strides=None):
    """One cm_listen_stats launch on device tensors (or None = NULL) into a sentinel-filled table with guard rows -> the whole table."""
    from com_marl_amd import _lib as L
    out = torch.full((S + 2 * GUARD, R.LISTEN_COLS), SENTINEL, dtype=torch.float64, device="cuda")
    p_st, m_st, l_st = strides or (N * A,) * 3
    L.check(L.lib().cm_listen_stats(S, N, A, L.ptr(probs), p_st, L.ptr(mute), m_st, L.ptr(lossless), l_st, L.ptr(out[GUARD:]),
                                    L.current_stream()), "cm_listen_stats")
    return out.cpu().numpy()


def _check(torch, S, N, A, probs, mute, lossless, want, what):
    """Host arrays (or None).  Two launches: the same bits, guards untouched, flips exact."""
    dev = [_dev(torch, x) for x in (probs, mute, lossless)]
    got = _launch(torch, S, N, A, *dev)
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + S:] == SENTINEL).all(), "guard rows written"
    rows = got[GUARD:GUARD + S]
    _close(rows, want, R.graph_atol(N), what)
    np.testing.assert_array_equal(rows[:, R.FLIP_COLS], want[:, R.FLIP_COLS], err_msg=what + ": flips")
    np.testing.assert_array_equal(_launch(torch, S, N, A, *dev), got)
    return rows


# every N class at A = 5, both S; A = 2 and 8 on the sub-wave and the wave kernel, with and without 16-byte loads
GRID = [(1, 5, 130), (2, 5, 130), (3, 5, 130), (4, 5, 130), (4, 5, 37), (5, 5, 130), (8, 5, 130), (8, 5, 37), (9, 5, 130), (24, 5, 130),
        (24, 5, 37), (72, 5, 37), (129, 5, 37), (255, 5, 37), (2, 2, 130), (3, 2, 37), (24, 2, 37), (4, 8, 37), (3, 8, 130), (9, 8, 130),
        (5, 3, 37), (6, 6, 37), (64, 7, 37), (65, 4, 37)]


@pytest.mark.parametrize("N,A,S", GRID, ids=[f"N{N}-A{A}-S{S}" for N, A, S in GRID])
def test_seeded_graphs_equal_the_restatement(gpu, N, A, S):
    """f32 softmax rows with a planted 0 in q under a positive p, one-hot rows, argmax ties and rows with q == p.  Each NULL
    counterfactual gives exact zeros and leaves the other's columns as they are; a prefix of the graphs gives the same rows."""
    probs, mute, lossless = R.seeded(S, N, A, seed=1000 * A + N)
    want = R.listen_stats(probs, mute, lossless)
    got = _check(gpu, S, N, A, probs, mute, lossless, want, f"N={N} A={A} S={S}")
    assert (got[3] == 0).all() and got[0, 0] > 10 and np.isfinite(got).all()       # q == p rows; the FLT_MIN term
    d = [_dev(gpu, x) for x in (probs, mute, lossless)]
    only_mute = _launch(gpu, S, N, A, d[0], d[1], None)[GUARD:GUARD + S]
    only_loss = _launch(gpu, S, N, A, d[0], None, d[2])[GUARD:GUARD + S]
    neither = _launch(gpu, S, N, A, d[0], None, None)[GUARD:GUARD + S]
    np.testing.assert_array_equal(only_mute, np.concatenate([got[:, :3], np.zeros((S, 3))], 1))
    np.testing.assert_array_equal(only_loss, np.concatenate([np.zeros((S, 3)), got[:, 3:]], 1))
    assert (neither == 0).all() and not np.signbit(neither).any()
    P = S // 2 + 1
    dp = [_dev(gpu, x[:P]) for x in (probs, mute, lossless)]
    np.testing.assert_array_equal(_launch(gpu, P, N, A, *dp)[GUARD:GUARD + P], got[:P])
    one = [_dev(gpu, x[S - 1:]) for x in (probs, mute, lossless)]
    np.testing.assert_array_equal(_launch(gpu, 1, N, A, *one)[GUARD:GUARD + 1], got[S - 1:])


@pytest.mark.parametrize("N,A", [(4, 5), (8, 5), (24, 5), (72, 5), (4, 8), (6, 2)])
def test_strides_past_the_block_and_buffers_off_16_byte_alignment(gpu, N, A):
    """Blocks 3 floats apart at an address 4 bytes past a 16-byte boundary take the one-float loads: the same bits as the 16-byte
    loads on the same values, aligned and packed."""
    torch = gpu
    S, blk = 11, N * A
    probs, mute, lossless = R.seeded(S, N, A, seed=80 + N)
    packed = _check(torch, S, N, A, probs, mute, lossless, R.listen_stats(probs, mute, lossless), "aligned")

    def spread(x):
        flat = torch.full((1 + S * (blk + 3),), 9.0, dtype=torch.float32, device="cuda")
        view = flat[1:].view(S, blk + 3)
        view[:, :blk] = torch.from_numpy(x.reshape(S, blk)).cuda()
        assert view.data_ptr() % 16 == 4
        return view
    sp = [spread(x) for x in (probs, mute, lossless)]
    np.testing.assert_array_equal(_launch(torch, S, N, A, *sp, strides=(blk + 3,) * 3)[GUARD:GUARD + S], packed)
    # only the counterfactuals off alignment; and aligned blocks a whole 16 bytes apart stay on the 16-byte loads
    np.testing.assert_array_equal(_launch(torch, S, N, A, _dev(torch, probs), sp[1], sp[2], strides=(blk, blk + 3, blk + 3))[GUARD:GUARD + S],
                                  packed)
    wide = torch.zeros(S, blk + 4, dtype=torch.float32, device="cuda")
    wide[:, :blk] = torch.from_numpy(probs.reshape(S, blk)).cuda()
    got = _launch(torch, S, N, A, wide, _dev(torch, mute), _dev(torch, lossless), strides=(blk + 4, blk, blk))
    np.testing.assert_array_equal(got[GUARD:GUARD + S], packed)


def test_no_graphs_write_nothing_and_refusals_set_the_error_text(gpu):
    torch = gpu
    from com_marl_amd import _lib as L
    lib = L.lib()
    d = [_dev(torch, x) for x in R.seeded(4, 4, 5, seed=3)]
    assert (_launch(torch, 0, 4, 5, *d) == SENTINEL).all()
    out = torch.full((4, R.LISTEN_COLS), SENTINEL, dtype=torch.float64, device="cuda")
    st = L.current_stream()
    for args in ((4, 0, 5, 20, 20, 20), (4, 256, 5, 20, 20, 20), (4, 4, 1, 20, 20, 20), (4, 4, 9, 36, 36, 36), (4, 4, 5, 19, 20, 20),
                 (4, 4, 5, 0, 20, 20), (4, 4, 5, 20, 19, 20), (4, 4, 5, 20, 20, 0), (-1, 4, 5, 20, 20, 20)):
        S, N, A, p_st, m_st, l_st = args
        assert lib.cm_listen_stats(S, N, A, L.ptr(d[0]), p_st, L.ptr(d[1]), m_st, L.ptr(d[2]), l_st, L.ptr(out), st) == -1, args
        assert b"cm_listen_stats" in lib.cm_last_error(), args
    for pr, o in ((None, L.ptr(out)), (L.ptr(d[0]), None)):
        assert lib.cm_listen_stats(4, 4, 5, pr, 20, L.ptr(d[1]), 20, L.ptr(d[2]), 20, o, st) == -1
        assert b"cm_listen_stats" in lib.cm_last_error()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()


def test_envs_listen_stats_takes_leading_shapes_and_none_counterfactuals(gpu):
    torch = gpu
    from com_marl_amd import envs
    S, N, A = 12, 5, 5
    probs, mute, lossless = R.seeded(S, N, A, seed=9)
    d_p, d_m, d_l = (_dev(torch, x) for x in (probs, mute, lossless))
    got = envs.listen_stats(d_p, d_m, d_l)
    assert got.shape == (S, 6) and got.dtype == torch.float64 and got.is_cuda
    _close(got.cpu().numpy(), R.listen_stats(probs, mute, lossless), R.graph_atol(N), "envs.listen_stats")
    two = envs.listen_stats(d_p.view(3, 4, N, A), lossless=d_l.view(3, 4, N, A))
    assert two.shape == (3, 4, 6)
    _close(two.cpu().numpy().reshape(S, 6), R.listen_stats(probs, None, lossless), R.graph_atol(N), "envs.listen_stats, no mute")
    out = torch.empty(S, 6, dtype=torch.float64, device="cuda")
    assert envs.listen_stats(d_p, d_m, out=out) is out
    _close(out.cpu().numpy(), R.listen_stats(probs, mute, None), R.graph_atol(N), "envs.listen_stats, no lossless")


# ---- the reductions -----------------------------------------------------------------------------------------------------------
def _groupings(B):
    out = [(1, 1, 2, 4)]
    for g in (3, 5, 13):
        if B % g == 0 and g < B:
            out.append((g, g - 1, 1, g + 2))
    if B > 1:
        out.append((B, B - 1, 3, B + 3))
    return out


def _stats_rows(T, B, N, seed):
    """Rows as cm_listen_stats writes them: kl up to N |ln FLT_MIN| and sometimes a hair below 0, tv up to N, whole flips."""
    rng = np.random.default_rng(seed)
    rows = rng.random((T, B, R.LISTEN_COLS)) * np.array([N * 87.0, N, N] * 2)
    rows[..., R.FLIP_COLS] = np.round(rows[..., R.FLIP_COLS])
    rows[::3, :, 3] = -1e-9 * rng.random((len(range(0, T, 3)), B))
    return rows


@pytest.mark.parametrize("T,B,N", [(7, 1, 4), (7, 3, 1), (7, 65, 4), (7, 130, 24), (70, 9, 5)])
@pytest.mark.parametrize("kind", ["none", "all0", "mixed"])
def test_episode_rows_and_curves_equal_the_restatement(gpu, T, B, N, kind):
    """take < group_size and row0 > 0 throughout; T = 70: an episode longer than one round of 64 lanes and more than one tile."""
    torch = gpu
    from com_marl_amd import _lib as L
    lib, st = L.lib(), L.current_stream()
    path_len = R.path_lens(T, B, seed=11 * T + B, kind=kind)
    stats = _stats_rows(T, B, N, seed=T + B)
    d_pl, d_st = torch.from_numpy(path_len).cuda(), torch.from_numpy(stats).cuda()
    for g, take, row0, epg in _groupings(B):
        rows, groups = B // g * epg, B // g
        want = np.full((rows, R.EPL_COLS), SENTINEL)
        R.episode_listen(path_len, stats, N, g, take, epg, row0, want)
        outs = []
        for _ in range(2):
            out = torch.full((rows + 2 * GUARD, R.EPL_COLS), SENTINEL, dtype=torch.float64, device="cuda")
            L.check(lib.cm_episode_listen(T, B, N, L.ptr(d_pl), L.ptr(d_st), g, take, epg, row0, L.ptr(out[GUARD:]), st),
                    "cm_episode_listen")
            outs.append(out.cpu().numpy())
        np.testing.assert_array_equal(outs[0], outs[1])
        got = outs[0]
        assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + rows:] == SENTINEL).all(), "guard rows written"
        named = want[:, 0] != SENTINEL
        assert named.sum() == groups * take
        np.testing.assert_array_equal(got[GUARD:GUARD + rows][~named], SENTINEL)          # the other rows keep the sentinel
        _close(got[GUARD:GUARD + rows][named], want[named], 1e-12, f"episode rows g={g}")

        # curves: a first launch overwrites, a second adds; then the means over 2 * take episodes
        want_sums = np.full((groups, T, R.LISTEN_COLS), SENTINEL)
        R.listen_curves(path_len, stats, g, take, 0, want_sums)
        R.listen_curves(path_len, stats, g, take, 1, want_sums)
        outs = []
        for _ in range(2):
            sums = torch.full((groups + 2, T, R.LISTEN_COLS), SENTINEL, dtype=torch.float64, device="cuda")
            for acc in (0, 1):
                L.check(lib.cm_listen_curves(T, B, N, L.ptr(d_pl), L.ptr(d_st), g, take, acc, L.ptr(sums[1:]), st), "cm_listen_curves")
            curves = torch.full((groups + 2, T, R.EPL_COLS), SENTINEL, dtype=torch.float64, device="cuda")
            L.check(lib.cm_listen_curve_means(groups, T, 2 * take, N, L.ptr(sums[1:]), L.ptr(curves[1:]), st), "cm_listen_curve_means")
            outs.append((sums.cpu().numpy(), curves.cpu().numpy()))
        for a, b in zip(outs[0], outs[1]):
            np.testing.assert_array_equal(a, b)
        sums, curves = outs[0]
        for t in (sums, curves):
            assert (t[0] == SENTINEL).all() and (t[-1] == SENTINEL).all(), "guard blocks written"
        _close(sums[1:-1], want_sums, 1e-12, f"curve sums g={g}")
        _close(curves[1:-1], R.listen_curve_means(want_sums, 2 * take, N), 1e-12, f"curve means g={g}")


@pytest.mark.parametrize("K,E", [(1, 1), (3, 5), (2, 65)])
def test_means_equal_the_restatement(gpu, K, E):
    torch = gpu
    from com_marl_amd import _lib as L
    table = np.random.default_rng(K * 1000 + E).random((K, E, R.EPL_COLS)) * 3.0
    dev = torch.from_numpy(table).cuda()
    outs = []
    for _ in range(2):
        out = torch.full((K + 2 * GUARD, R.EPL_COLS), SENTINEL, dtype=torch.float64, device="cuda")
        L.check(L.lib().cm_listen_means(K, E, L.ptr(dev), L.ptr(out[GUARD:]), L.current_stream()), "cm_listen_means")
        outs.append(out.cpu().numpy())
    np.testing.assert_array_equal(outs[0], outs[1])
    got = outs[0]
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + K:] == SENTINEL).all(), "guard rows written"
    _close(got[GUARD:GUARD + K], R.listen_means(table), 1e-12, "means")


# ---- the replay ---------------------------------------------------------------------------------------------------------------
T = 6


def _wrapper(scen, params, n_envs, channel=None, **kw):
    from com_marl_amd import envs as E_
    cls = E_.PredatorPreyWrapper if scen == "pp" else E_.CoverageWrapper
    return cls(True, params=params, n_envs=n_envs, device="cuda:0", seed=3, channel=channel, **kw)


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


def _members(eng):
    """-> [(policy, lo, hi)] of an engine."""
    if eng.multi_form is None:
        return [(eng.policy, 0, eng.env.B)]
    return [(pol, lo, hi) for pol, (lo, hi) in zip(eng.policy, eng.groups)]


def _masks(torch, kind, rows, Lh, N):
    """The counterfactual channels written out as a tensor [rows, Lh, N, N]."""
    if kind == "ones":
        return torch.ones(rows, Lh, N, N, device="cuda")
    return torch.eye(N, device="cuda").expand(rows, Lh, N, N).contiguous()


def _by_act_device(torch, members, obs, adj, kind, Lh):
    """obs [n,B,N,d], adj [n,B,N,N] | None (device) -> probs [n,B,N,A] under the counterfactual `kind`, member by member, by
    act_device on materialised masks - the definition of the counterfactual probabilities."""
    n, B, N = obs.shape[:3]
    out = None
    for pol, lo, hi in members:
        rows = n * (hi - lo)
        o = obs[:, lo:hi].reshape(rows, -1).contiguous()
        a = None if adj is None else adj[:, lo:hi].reshape(rows, N, N).contiguous()
        _, p, _ = pol.act_device(o, None, a, _masks(torch, kind, rows, Lh, N), greedy=True, want_actions=False, want_attn=False,
                                 policy_step=0)
        if out is None:
            out = torch.empty(n, B, N, p.shape[-1], device="cuda")
        out[:, lo:hi] = p.view(n, hi - lo, N, -1)
    return out


SCENARIOS = {
    # name: (scenario, params, envs, policies, the launch form the round takes)
    "pp4_chunk": ("pp", dict(map_=10, sen=1, N=4, M=4, teRcom=2, tepl=0.3), 32, 1),
    "pp4_multi": ("pp", dict(map_=10, sen=1, N=4, M=4, teRcom=2, tepl=0.3), 32, 2),
    "co24": ("co", dict(map_=20, sen=2, N=24, M=0, teRcom=6, tepl=0.3), 6, 1),
}


@pytest.fixture(scope="module")
def played(gpu):
    """name -> (engine after one greedy round of T slots, clones of its buffers, the policies): played once, shared, unchanged."""
    from com_marl_amd.nets import PolicySet
    from com_marl_amd.rollout import RolloutEngine
    out = {}
    for name, (scen, kw, B, K) in SCENARIOS.items():
        kw = dict(kw)
        params = cc.base_params(scen, kw.pop("map_"), kw.pop("sen"), kw.pop("N"), kw.pop("M"), max_env_steps=T, **kw)
        env = _wrapper(scen, params, B)
        batch = getattr(env, "env", env).batch
        pols = _policies(env, K)
        ps = pols[0] if K == 1 else PolicySet(pols)
        ps.sync_weights()
        ps.reset([True] * (B // K))
        eng = RolloutEngine(batch, ps, T, store_attn=False, store_probs=True, **({} if K == 1 else dict(groups=[B // K] * K)))
        eng.reset()
        eng.play(0, T, greedy=True, chunk=True)
        eng.bump(T)
        batch.check_status()
        gpu.cuda.synchronize()
        names = ("obs", "actions", "probs", "reward64", "done", "details", "success", "path_len", "dist_adj", "channels")
        keep = {k: getattr(eng, k).clone() for k in names}
        keep["step_base"] = eng.step_base.clone()
        out[name] = (eng, keep, pols, env)
    return out


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_replay_with_the_recorded_channels_reproduces_the_record_bit_for_bit(gpu, played, name):
    torch = gpu
    from com_marl_amd import rollout
    eng, keep, pols, _ = played[name]
    if name == "pp4_chunk":
        assert eng.multi_form is None and eng._fused is True                 # the round was the chunk launch
    if name == "pp4_multi":
        assert eng.multi_form == "wave"                                      # the multi-policy launch
    B, N = eng.env.B, eng.env.N
    steps = [p._policy_step for p in pols]
    out = torch.full((T, B, N, 5), SENTINEL, device="cuda")
    assert eng.replay_probs(0, T, "recorded", out) is out
    assert torch.equal(out, keep["probs"]), f"{name}: {int((out != keep['probs']).sum())} probabilities differ from the record"
    # a span in the middle; the identity block is allocated once and reused
    mid = torch.full((2, B, N, 5), SENTINEL, device="cuda")
    eng.replay_probs(3, 2, "recorded", mid)
    assert torch.equal(mid, keep["probs"][3:5])
    eng.replay_probs(0, T, "identity", out)
    block = eng._eye_rows
    eng.replay_probs(1, T - 1, "identity", out[1:])
    assert eng._eye_rows is block and block.numel() * 4 <= rollout.REPLAY_MASK_BYTES
    for k, v in keep.items():
        now = eng.step_base if k == "step_base" else getattr(eng, k)
        assert torch.equal(now, v), f"{name}: the replay changed {k}"
    assert [p._policy_step for p in pols] == steps
    for bad in (dict(t0=0, n=T + 1), dict(t0=-1, n=2), dict(t0=0, n=0)):
        with pytest.raises(ValueError, match="replay_probs"):
            eng.replay_probs(bad["t0"], bad["n"], "recorded", out)
    with pytest.raises(ValueError, match="replay_probs"):
        eng.replay_probs(0, T, "FL", out)
    with pytest.raises(ValueError, match="replay_probs"):
        eng.replay_probs(0, T, "ones", out[:, :, :, :4])


def test_the_identity_replay_in_several_launches_gives_the_same_bits(gpu, played, monkeypatch):
    """A mask bound that holds 40 env states: the 192 rows of the round take five launches on one block of 40 rows."""
    torch = gpu
    from com_marl_amd import rollout
    eng, keep, _, _ = played["pp4_chunk"]
    B, N, Lh = eng.env.B, eng.env.N, eng.env.Lh
    whole = torch.empty(T, B, N, 5, device="cuda")
    eng.replay_probs(0, T, "identity", whole)
    monkeypatch.setattr(rollout, "REPLAY_MASK_BYTES", 40 * 4 * Lh * N * N)
    monkeypatch.setattr(eng, "_eye_rows", None)
    parts = torch.empty_like(whole)
    eng.replay_probs(0, T, "identity", parts)
    assert eng._eye_rows.shape[0] == 40 and torch.equal(parts, whole)


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_counterfactual_replays_equal_act_device_and_lie_within_the_float64_bound(gpu, played, name):
    torch = gpu
    eng, keep, pols, _ = played[name]
    B, N, Lh = eng.env.B, eng.env.N, eng.env.Lh
    obs, adj = keep["obs"][:T], keep["dist_adj"][:T]
    for kind in ("identity", "ones"):
        got = torch.empty(T, B, N, 5, device="cuda")
        eng.replay_probs(0, T, kind, got)
        want = _by_act_device(torch, _members(eng), obs, adj, kind, Lh)
        assert torch.equal(got, want), f"{name} {kind}: the replay is not act_device on the materialised mask"
        assert not torch.equal(got, keep["probs"])                          # the channel mattered somewhere
        for pol, lo, hi in _members(eng):
            rows = T * (hi - lo)
            p64 = F.params({k: v.detach().cpu() for k, v in pol.state_dict().items()}, requires_grad=False)
            t64 = lambda x: x.double().cpu()                                # noqa: E731
            with torch.no_grad():
                lg64, pr64, _ = F.policy_forward(p64, t64(obs[:, lo:hi].reshape(rows, -1)), None, t64(adj[:, lo:hi].reshape(rows, N, N)),
                                                 t64(_masks(torch, kind, rows, Lh, N)), N)
            p, ref = got[:, lo:hi].reshape(rows, N, 5).double().cpu().numpy(), pr64.numpy()
            r = F.ratio(p, pr64)
            big = ref >= 1e-30
            bound = 2 * TAU * float(lg64.abs().max())
            err = float(np.abs(np.log(p[big]) - np.log(ref[big])).max())
            print(f"{name} {kind} envs {lo}..{hi - 1}: probs off by {r:.3g} of their scale (TAU {TAU}), log-probabilities by {err:.3g} "
                  f"(bound {bound:.3g})")
            assert r <= TAU and err <= bound and (p[~big] <= 1e-29).all()


# ---- eval_summary / eval_sweep ------------------------------------------------------------------------------------------------
@pytest.fixture
def spy(monkeypatch):
    """-> the list of engines the evaluation built; each keeps device copies of what every round left in its buffers."""
    from com_marl_amd import evaluate
    used = []

    class Spy(evaluate.RolloutEngine):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.rounds = []
            used.append(self)

        def bump(self, *a, **kw):
            out = super().bump(*a, **kw)
            keep = lambda x: None if x is None else x.clone()               # noqa: E731
            self.rounds.append({name: keep(getattr(self, name)) for name in ("obs", "probs", "dist_adj", "channels", "path_len")})
            return out

    monkeypatch.setattr(evaluate, "RolloutEngine", Spy)
    return used


def _expected(torch, eng, E, n_epi):
    """The rounds a spied engine played -> (episode table [cells, n_epi, 6], curve means [cells, T, 6]) by the restatement, from
    the engine's own probs and counterfactual probabilities computed here by act_device on materialised masks."""
    batch = eng.env
    B, N, Lh = batch.B, batch.N, batch.Lh
    cells = B // E
    table = np.zeros((cells * n_epi, R.EPL_COLS))
    sums = np.zeros((cells, T, R.LISTEN_COLS))
    done = 0
    for r in eng.rounds:
        probs = r["probs"][:T]
        adj = None if r["dist_adj"] is None else r["dist_adj"][:T]
        cf = [_by_act_device(torch, _members(eng), r["obs"][:T], adj, kind, Lh).cpu().numpy().reshape(T * B, N, -1)
              for kind in ("identity", "ones")]
        stats = R.listen_stats(probs.cpu().numpy().reshape(T * B, N, -1), *cf).reshape(T, B, R.LISTEN_COLS)
        take = min(E, n_epi - done)
        pl = r["path_len"][:T].cpu().numpy()
        R.episode_listen(pl, stats, N, E, take, n_epi, done, table)
        R.listen_curves(pl, stats, E, take, int(done > 0), sums)
        done += take
    assert done == n_epi
    return table.reshape(cells, n_epi, R.EPL_COLS), R.listen_curve_means(sums, n_epi, N)


def _check_cell(d, table, curves, what):
    from com_marl_amd.evaluate import LISTEN_KEYS
    assert set(LISTEN_KEYS) <= set(d)
    ep = d["listen_episodes"]
    assert ep.is_cuda and tuple(ep.shape) == table.shape
    _close(ep.cpu().numpy(), table, 1e-12, what + " listen_episodes")
    _close([d[k] for k in LISTEN_KEYS], R.listen_means(table[None])[0], 1e-12, what + " keys")
    _close(np.stack([d["curves"][k] for k in LISTEN_KEYS], 1), curves, 1e-12, what + " curves")
    assert all(d["curves"][k].shape == (T,) for k in LISTEN_KEYS)
    assert 0 <= d["listen_tv"] <= 1 and 0 <= d["listen_flip"] <= 1 and 0 <= d["loss_tv"] <= 1 and 0 <= d["loss_flip"] <= 1


CONDS = [dict(Rcom=9, pl=0), dict(Rcom=2, pl=0.3)]
ALL = dict(listen_stats=True, comm_stats=True, curves=True, episodes=True)


def test_eval_summary_of_two_policies_equals_the_restatement_on_the_engines_buffers(gpu, spy):
    """PP map 10, teams of 4, 32 envs = 2 policies x 16, IID pl = 0.3 with Rcom = 2, 24 episodes each: a full round and one of 8."""
    from com_marl_amd.evaluate import eval_summary
    params = cc.base_params("pp", 10, 1, 4, 4, max_env_steps=T, teRcom=2, tepl=0.3)
    env = _wrapper("pp", params, 32)
    got = eval_summary(env, _policies(env, 2), 0, n_eval_episodes=24, max_env_steps=T, **ALL)
    assert len(spy) == 1 and len(spy[0].rounds) == 2 and spy[0].probs is not None
    table, curves = _expected(gpu, spy[0], 16, 24)
    for k in range(2):
        _check_cell(got[k], table[k], curves[k], f"policy {k}")
        assert got[k]["listen_kl"] > 0 and got[k]["listen_tv"] > 0 and got[k]["loss_kl"] > 0 and got[k]["loss_tv"] > 0


def test_eval_sweep_of_two_conditions_equals_the_restatement_and_a_lossless_condition_loses_nothing(gpu, spy):
    """2 policies x 2 conditions x 8 envs, 12 episodes per cell: a full round and one of 4.  The first condition loses nothing:
    its recorded channels are all ones, so the lossless replay repeats the round's forward bit for bit."""
    from com_marl_amd.evaluate import LISTEN_KEYS, eval_sweep
    params = cc.base_params("pp", 10, 1, 4, 4, max_env_steps=T)
    env = _wrapper("pp", params, 32, "IID", conditions=CONDS)
    got = eval_sweep(env, _policies(env, 2), 0, n_eval_episodes=12, max_env_steps=T, **ALL)
    assert len(spy) == 1 and len(spy[0].rounds) == 2
    table, curves = _expected(gpu, spy[0], 8, 12)
    for k in range(2):
        for c in range(2):
            _check_cell(got[k][c], table[2 * k + c], curves[2 * k + c], f"cell {k},{c}")
        full, lossy = got[k]
        for key in LISTEN_KEYS[3:]:
            assert full[key] == 0.0 and (full["curves"][key] == 0.0).all(), key
        assert (full["listen_episodes"][:, 3:] == 0).all()
        assert lossy["loss_kl"] > 0 and lossy["loss_tv"] > 0 and lossy["listen_kl"] > 0


def test_eval_summary_coverage_teams_of_24(gpu, spy):
    """Coverage map 20, N = 24 (one wave per graph), 6 envs, one policy, 9 episodes: a full round and one of 3."""
    from com_marl_amd.evaluate import eval_summary
    params = cc.base_params("co", 20, 2, 24, 0, max_env_steps=T, teRcom=6, tepl=0.3)
    env = _wrapper("co", params, 6)
    got = eval_summary(env, _policies(env, 1)[0], 0, n_eval_episodes=9, max_env_steps=T, **ALL)
    assert isinstance(got, dict) and len(spy) == 1 and len(spy[0].rounds) == 2
    table, curves = _expected(gpu, spy[0], 6, 9)
    _check_cell(got, table[0], curves[0], "coverage")


FORWARDS = ("cm_policy_forward", "cm_policy_forward_any", "cm_policy_forward_multi", "cm_policy_forward_any_multi")


def test_a_constant_channel_skips_its_replay(gpu, spy, lib_spy):  # noqa: F811
    """FC (tepl = 0): no lossless replay - loss_* exactly 0 and ONE replay forward per slot's envs, not two; FL (tepl = 1): no
    mute replay - listen_* exactly 0.  One policy, 16 envs, 16 episodes: one round.  Counted: the env states that went through
    a forward-only launch, with the keyword and without it."""
    from com_marl_amd.evaluate import LISTEN_KEYS, eval_summary

    def forwards(tepl, **kw):
        params = cc.base_params("pp", 10, 1, 4, 4, max_env_steps=T, teRcom=2, tepl=tepl)
        env = _wrapper("pp", params, 16)
        pol = _policies(env, 1)[0]
        lib_spy.calls.clear()
        got = eval_summary(env, pol, 0, n_eval_episodes=16, max_env_steps=T, episodes=True, curves=True, **kw)
        rows = sum(c.args[1] for c in lib_spy.calls if c in FORWARDS)       # env states that went through a forward launch
        return got, rows, spy[-1]

    _, base_rows, _ = forwards(0.0)
    fc, fc_rows, eng = forwards(0.0, listen_stats=True)
    assert eng.channels is None and eng.env.channelType == "FC"
    assert fc_rows - base_rows == T * 16                                    # one replay forward per slot's envs, not two
    for key in LISTEN_KEYS[3:]:
        assert fc[key] == 0.0 and (fc["curves"][key] == 0.0).all(), key
    assert (fc["listen_episodes"][:, 3:] == 0).all() and fc["listen_kl"] > 0 and fc["listen_tv"] > 0
    _, lossy_rows, _ = forwards(0.3, listen_stats=True)
    _, lossy_base, _ = forwards(0.3)
    assert lossy_rows - lossy_base == 2 * T * 16                            # both replays under a channel that varies
    fl, fl_rows, eng = forwards(1.0, listen_stats=True)
    assert eng.channels is None and eng.env.channelType == "FL"
    for key in LISTEN_KEYS[:3]:
        assert fl[key] == 0.0 and (fl["curves"][key] == 0.0).all(), key
    assert (fl["listen_episodes"][:, :3] == 0).all()


def test_switched_off_nothing_is_kept_launched_or_returned_and_the_rest_is_bit_equal(gpu, spy, lib_spy):  # noqa: F811
    import torch
    from com_marl_amd.evaluate import LISTEN_KEYS, eval_summary
    params = cc.base_params("pp", 10, 1, 4, 4, max_env_steps=T, teRcom=2, tepl=0.3)
    kw = dict(n_eval_episodes=24, max_env_steps=T, comm_stats=True, attn_stats=True, curves=True, episodes=True)
    env = _wrapper("pp", params, 32)
    pols = _policies(env, 2)
    off = eval_summary(env, pols, 0, **kw)
    assert len(spy) == 1 and spy[0].probs is None
    assert not [c for c in lib_spy.calls if "listen" in c]
    on = eval_summary(_wrapper("pp", params, 32), pols, 0, listen_stats=True, **kw)
    assert spy[1].probs is not None
    n_rounds = 2
    for name, n in (("cm_listen_stats", n_rounds), ("cm_episode_listen", n_rounds), ("cm_listen_curves", n_rounds), ("cm_listen_means", 1),
                    ("cm_listen_curve_means", 1)):
        assert lib_spy.count(name) == n, name
    for a, b in zip(off, on):
        assert not set(LISTEN_KEYS) & set(a) and "listen_episodes" not in a and not set(LISTEN_KEYS) & set(a["curves"])
        assert set(b) == set(a) | set(LISTEN_KEYS) | {"listen_episodes"} and set(b["curves"]) == set(a["curves"]) | set(LISTEN_KEYS)
        for key, v in a.items():
            if key in ("episodes", "comm_episodes", "attn_episodes"):
                assert torch.equal(v, b[key]), key
            elif key == "curves":
                for name, curve in v.items():
                    np.testing.assert_array_equal(curve, b[key][name], err_msg=name)
            else:
                assert v == b[key], key


def test_a_policy_without_a_comm_trunk_is_refused(gpu, spy):
    from com_marl_amd import nets
    from com_marl_amd.evaluate import eval_summary, eval_sweep
    params = cc.base_params("pp", 10, 1, 4, 4, max_env_steps=T)
    env = _wrapper("pp", params, 32)
    dec = nets.DecCategoricalMLPPolicy(env.spec, n_agents=env.n_agents, device="cuda:0")
    with pytest.raises(ValueError, match="listen_stats"):
        eval_summary(env, dec, 0, n_eval_episodes=8, max_env_steps=T, listen_stats=True)
    with pytest.raises(ValueError, match="listen_stats"):
        eval_summary(env, [dec, dec], 0, n_eval_episodes=8, max_env_steps=T, listen_stats=True)
    cenv = _wrapper("pp", params, 32, "IID", conditions=CONDS)
    with pytest.raises(ValueError, match="listen_stats"):
        eval_sweep(cenv, dec, 0, n_eval_episodes=8, max_env_steps=T, listen_stats=True)
    assert spy == []                                             # refused before anything is built
