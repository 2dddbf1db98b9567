"""cm_value_stats and its reductions (csrc/cm_value_stats.hip) through ctypes, envs.value_stats, RolloutEngine.replay_values and
eval_summary / eval_sweep with value_stats=True, against the numpy float64 restatement (tests/value_stats_ref.py).  Both sides
compute in f64 from the same inputs: rtol = 1e-10 with the per-env atol 1e-12 max(1, sum_t |r_t|, max |v|), squared for the two
squared columns (the reasoning is in the restatement's docstring); every comparison prints the largest error it saw.  Repeated
launches are compared bit for bit.

Shapes: one lane (B = 1), ragged waves (B = 63, 65), a ragged last workgroup and several of them (B = 300), T = 1 and 7 inside one
batch of loaded steps, T = 70 and 130 past one and two batches of the length search (32 steps) and four and eight of the
recurrence (16 steps), each with no episode ending, all ending at step 0 and a mix, at gamma = 0.99, 1 and 0.

The replays are judged against critic.values_device itself: with the recorded channels slot by slot, with the counterfactual
channels on materialised masks, bit for bit - which is how the expected values of the end-to-end tests are formed."""
import math

import numpy as np
import pytest

from tests import conditions_common as cc, value_stats_ref as R
from tests.lib_spy import spy as lib_spy  # noqa: F401  (the fixture: a recording proxy around _lib.lib())

pytestmark = pytest.mark.gpu

SENTINEL = -77.0
GUARD = 3                                                       # guard rows in front of and behind each output


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch


def _close(got, want, atol, what):
    """|got - want| <= atol + RTOL |want| elementwise (atol broadcast against the arrays), printing the largest errors."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    atol = np.broadcast_to(np.asarray(atol, np.float64), want.shape)
    err = np.abs(got - want)
    bound = atol + R.RTOL * np.abs(want)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(err > 0, err / bound, 0.0)             # (a bound of 0 asks for equality)
    print(f"{what}: max |error| {err.max(initial=0.0):.3e}, max error / bound {ratio.max(initial=0.0):.3e} (rtol {R.RTOL:g}, "
          f"atol up to {atol.max(initial=0.0):.3g})")
    assert np.isfinite(got).all(), what
    bad = err > bound
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values off; worst error / bound {ratio.max():.3e}"


def _dev(torch, x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _launch(torch, T, B, rewards, path_len, values, mute, lossless, gamma):
    """One cm_value_stats launch on device tensors (or None = NULL) into a sentinel-filled table with guard rows -> the whole table."""
    from com_marl_amd import _lib as L
    out = torch.full((T * B + 2 * GUARD, R.VALUE_COLS), SENTINEL, dtype=torch.float64, device="cuda")
    L.check(L.lib().cm_value_stats(T, B, L.ptr(rewards), L.ptr(path_len), L.ptr(values), L.ptr(mute), L.ptr(lossless), gamma,
                                   L.ptr(out[GUARD:]), L.current_stream()), "cm_value_stats")
    return out.cpu().numpy()


def _rows(table, T, B):
    assert (table[:GUARD] == SENTINEL).all() and (table[GUARD + T * B:] == SENTINEL).all(), "guard rows written"
    return table[GUARD:GUARD + T * B].reshape(T, B, R.VALUE_COLS)


GRID = [(1, 1), (7, 1), (7, 63), (7, 65), (7, 300), (70, 9), (130, 5)]


@pytest.mark.parametrize("gamma", [0.99, 1.0, 0.0])
@pytest.mark.parametrize("kind", ["none", "all0", "mixed"])
@pytest.mark.parametrize("T,B", GRID, ids=[f"T{T}-B{B}" for T, B in GRID])
def test_seeded_steps_equal_the_restatement(gpu, T, B, kind, gamma):
    """Two launches give equal bits, the guard rows stay untouched, a prefix of the envs on re-packed inputs gives the same rows, and
    each NULL counterfactual gives exact +0.0 and leaves the other columns' bits as they are."""
    host = R.seeded(T, B, kind, seed=100 * T + B)
    rewards, path_len, values, mute, lossless = host
    want = R.value_stats(rewards, path_len, values, mute, lossless, gamma)
    d = [_dev(gpu, x) for x in host]
    table = _launch(gpu, T, B, *d, gamma)
    got = _rows(table, T, B)
    _close(got, want, R.env_atol(rewards, values)[None], f"T={T} B={B} {kind} gamma={gamma}")
    np.testing.assert_array_equal(_launch(gpu, T, B, *d, gamma), table)
    for b in range(B):
        n = R.episode_length(path_len[:, b])
        assert (got[n:, b] == 0).all() and not np.signbit(got[n:, b]).any()              # exact zeros behind the episode
        assert got[n - 1, b, 1] == rewards[n - 1, b]                                     # G[n-1] = r[n-1]
        assert (got[:n, b, 0] == values[:n, b].astype(np.float64)).all()
    if gamma == 0.0:
        assert (got[..., 1] == want[..., 1]).all()                                       # G = r: nothing to round
    if B > 1:
        assert (got[:, 1, 5] == 0).all()                                                 # lossless == values on env 1
    # NULL counterfactuals
    zeros = np.zeros((T, B))
    only_mute = _rows(_launch(gpu, T, B, *d[:4], None, gamma), T, B)
    only_loss = _rows(_launch(gpu, T, B, *d[:3], None, d[4], gamma), T, B)
    neither = _rows(_launch(gpu, T, B, *d[:3], None, None, gamma), T, B)
    for rows, cols in ((only_mute, [5]), (only_loss, [4]), (neither, [4, 5])):
        keep = [c for c in range(R.VALUE_COLS) if c not in cols]
        np.testing.assert_array_equal(rows[..., keep], got[..., keep])
        for c in cols:
            np.testing.assert_array_equal(rows[..., c], zeros)
            assert not np.signbit(rows[..., c]).any()
    # a prefix of the envs, re-packed
    P = B // 2 + 1
    dp = [_dev(gpu, x[:, :P]) for x in host]
    np.testing.assert_array_equal(_rows(_launch(gpu, T, P, *dp, gamma), T, P), got[:, :P])
    last = [_dev(gpu, x[:, B - 1:]) for x in host]
    np.testing.assert_array_equal(_rows(_launch(gpu, T, 1, *last, gamma), T, 1), got[:, B - 1:])


def test_nothing_to_do_writes_nothing_and_refusals_set_the_error_text(gpu):
    torch = gpu
    from com_marl_amd import _lib as L
    lib, st = L.lib(), L.current_stream()
    d = [_dev(torch, x) for x in R.seeded(4, 5, "mixed", seed=3)]
    out = torch.full((20, R.VALUE_COLS), SENTINEL, dtype=torch.float64, device="cuda")
    call = lambda T, B, gamma, ptrs, o: lib.cm_value_stats(T, B, *ptrs, gamma, o, st)       # noqa: E731
    ptrs = [L.ptr(x) for x in d]
    assert call(0, 5, 0.99, ptrs, L.ptr(out)) == 0 and call(4, 0, 0.99, ptrs, L.ptr(out)) == 0
    for T, B, gamma in ((-1, 5, 0.99), (4, -1, 0.99), (4, 5, 1.01), (4, 5, -0.5), (4, 5, float("nan")), (4, 5, float("inf"))):
        assert call(T, B, gamma, ptrs, L.ptr(out)) == -1, (T, B, gamma)
        assert b"cm_value_stats" in lib.cm_last_error()
    for i in range(3):                                           # a NULL required array
        assert call(4, 5, 0.99, ptrs[:i] + [None] + ptrs[i + 1:], L.ptr(out)) == -1
        assert b"cm_value_stats" in lib.cm_last_error()
    assert call(4, 5, 0.99, ptrs, None) == -1
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()


def test_envs_value_stats_takes_none_counterfactuals_and_out(gpu):
    torch = gpu
    from com_marl_amd import envs
    T, B = 9, 7
    host = R.seeded(T, B, "mixed", seed=9)
    rewards, path_len, values, mute, lossless = host
    d = [_dev(torch, x) for x in host]
    atol = R.env_atol(rewards, values)[None]
    got = envs.value_stats(*d)
    assert got.shape == (T, B, 6) and got.dtype == torch.float64 and got.is_cuda
    _close(got.cpu().numpy(), R.value_stats(*host, 0.99), atol, "envs.value_stats")
    got = envs.value_stats(*d[:3], lossless=d[4], discount=0.5)
    _close(got.cpu().numpy(), R.value_stats(rewards, path_len, values, None, lossless, 0.5), atol, "envs.value_stats, no mute")
    out = torch.empty(T, B, 6, dtype=torch.float64, device="cuda")
    assert envs.value_stats(*d[:4], discount=1.0, out=out) is out
    _close(out.cpu().numpy(), R.value_stats(rewards, path_len, values, mute, None, 1.0), atol, "envs.value_stats, no lossless")


# ---- the reductions -----------------------------------------------------------------------------------------------------------
def _groupings(B):
    out = [(1, 1, 2, 4)]
    for g in (3, 5, 13):
        if B % g == 0 and g < B:
            out.append((g, g - 1, 1, g + 2))
    if B > 1:
        out.append((B, B - 1, 3, B + 3))
    return out


@pytest.mark.parametrize("T,B", [(7, 1), (7, 3), (7, 65), (7, 130), (70, 9)])
@pytest.mark.parametrize("kind", ["none", "all0", "mixed"])
def test_episode_rows_and_curves_equal_the_restatement(gpu, T, B, kind):
    """tests/test_listen_stats.py's grid with one agent: take < group_size and row0 > 0 throughout, accumulate 0 then 1; T = 70: an
    episode longer than one round of 64 lanes and more than one tile.  The rows are cm_value_stats' own (signed, of mixed scale):
    a sum of at most T of them, in whatever order, is off by at most T 2^-53 of their largest: atol = 1e-12 of it."""
    torch = gpu
    from com_marl_amd import _lib as L
    lib, st = L.lib(), L.current_stream()
    rewards, path_len, values, mute, lossless = R.seeded(T, B, kind, seed=11 * T + B)
    stats = R.value_stats(rewards, path_len, values, mute, lossless, 0.99)
    rng = np.random.default_rng(T + B)
    stats = np.where(stats == 0, rng.standard_normal(stats.shape), stats)                 # rows behind the end must not be read
    atol = 1e-12 * max(1.0, float(np.abs(stats).max()))
    d_pl, d_st = torch.from_numpy(path_len).cuda(), torch.from_numpy(stats).cuda()
    for g, take, row0, epg in _groupings(B):
        rows, groups = B // g * epg, B // g
        want = np.full((rows, R.EPV_COLS), SENTINEL)
        R.episode_value(path_len, stats, g, take, epg, row0, want)
        outs = []
        for _ in range(2):
            out = torch.full((rows + 2 * GUARD, R.EPV_COLS), SENTINEL, dtype=torch.float64, device="cuda")
            L.check(lib.cm_episode_value(T, B, L.ptr(d_pl), L.ptr(d_st), g, take, epg, row0, L.ptr(out[GUARD:]), st), "cm_episode_value")
            outs.append(out.cpu().numpy())
        np.testing.assert_array_equal(outs[0], outs[1])
        got = outs[0]
        assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + rows:] == SENTINEL).all(), "guard rows written"
        named = (want != SENTINEL).any(1)
        assert named.sum() == groups * take
        np.testing.assert_array_equal(got[GUARD:GUARD + rows][~named], SENTINEL)          # the other rows keep the sentinel
        _close(got[GUARD:GUARD + rows][named], want[named], atol, f"episode rows g={g}")

        # curves: a first launch overwrites, a second adds; then the means over 2 * take episodes
        want_sums = np.full((groups, T, R.VALUE_COLS), SENTINEL)
        R.value_curves(path_len, stats, g, take, 0, want_sums)
        R.value_curves(path_len, stats, g, take, 1, want_sums)
        outs = []
        for _ in range(2):
            sums = torch.full((groups + 2, T, R.VALUE_COLS), SENTINEL, dtype=torch.float64, device="cuda")
            for acc in (0, 1):
                L.check(lib.cm_value_curves(T, B, L.ptr(d_pl), L.ptr(d_st), g, take, acc, L.ptr(sums[1:]), st), "cm_value_curves")
            curves = torch.full((groups + 2, T, R.EPV_COLS), SENTINEL, dtype=torch.float64, device="cuda")
            L.check(lib.cm_value_curve_means(groups, T, 2 * take, L.ptr(sums[1:]), L.ptr(curves[1:]), st), "cm_value_curve_means")
            outs.append((sums.cpu().numpy(), curves.cpu().numpy()))
        for a, b in zip(outs[0], outs[1]):
            np.testing.assert_array_equal(a, b)
        sums, curves = outs[0]
        for t in (sums, curves):
            assert (t[0] == SENTINEL).all() and (t[-1] == SENTINEL).all(), "guard blocks written"
        _close(sums[1:-1], want_sums, atol * 2 * take, f"curve sums g={g}")
        _close(curves[1:-1], R.value_curve_means(want_sums, 2 * take), atol, f"curve means g={g}")


@pytest.mark.parametrize("K,E", [(1, 1), (3, 5), (2, 65)])
def test_means_equal_the_restatement(gpu, K, E):
    torch = gpu
    from com_marl_amd import _lib as L
    table = np.random.default_rng(K * 1000 + E).standard_normal((K, E, R.EPV_COLS)) * 3.0
    dev = torch.from_numpy(table).cuda()
    outs = []
    for _ in range(2):
        out = torch.full((K + 2 * GUARD, R.EPV_COLS), SENTINEL, dtype=torch.float64, device="cuda")
        L.check(L.lib().cm_value_means(K, E, L.ptr(dev), L.ptr(out[GUARD:]), L.current_stream()), "cm_value_means")
        outs.append(out.cpu().numpy())
    np.testing.assert_array_equal(outs[0], outs[1])
    got = outs[0]
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + K:] == SENTINEL).all(), "guard rows written"
    _close(got[GUARD:GUARD + K], R.value_means(table), 1e-12 * float(np.abs(table).max()), "means")


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


def _critics(env, n, **kw):
    """n CommBaseCritics of seeded weights; the output layer scaled up so that the values are of the returns' size."""
    import torch
    from com_marl_amd import nets
    out = []
    for k in range(n):
        torch.manual_seed(70 + k)
        c = nets.CommBaseCritic(env.spec, n_agents=env.n_agents, n_gcn_layers=env.GCNHops, device="cuda:0", **kw)
        with torch.no_grad():
            for p in c.baseline_aggregator._mean_module._output_layers[0].linear.parameters():
                p.mul_(8.0)
        c.sync_weights()
        out.append(c)
    return out


def _members(eng, critics):
    """-> [(critic, lo, hi)] of an engine and what replay_values takes."""
    if not isinstance(critics, list):
        return [(critics, 0, eng.env.B)]
    return [(c, lo, hi) for c, (lo, hi) in zip(critics, eng.groups)]


def _masks(torch, kind, rows, Lh, N):
    """The counterfactual channels written out as a tensor [rows, Lh, N, N]."""
    if kind == "ones":
        return torch.ones(rows, Lh, N, N, device="cuda")
    return torch.eye(N, device="cuda").expand(rows, Lh, N, N).contiguous()


def _by_values_device(torch, members, obs, adj, chan, kind, Lh):
    """obs [n,B,N,d], adj [n,B,N,N] | None, chan [n,B,Lh,N,N] | None (device) -> values [n,B] under `kind`, member by member, by
    values_device on the member's rows of all n slots - for a counterfactual kind on materialised masks: the definition."""
    n, B, N = obs.shape[:3]
    out = torch.empty(n, B, device="cuda")
    for critic, lo, hi in members:
        rows = n * (hi - lo)
        o = obs[:, lo:hi].reshape(rows, -1).contiguous()
        if not hasattr(critic, "comm"):
            out[:, lo:hi] = critic.values_device(o).view(n, hi - lo)
            continue
        a = None if adj is None else adj[:, lo:hi].reshape(rows, N, N).contiguous()
        if kind == "recorded":
            ch = None if chan is None else chan[:, lo:hi].reshape(rows, Lh, N, N).contiguous()
        else:
            ch = _masks(torch, kind, rows, Lh, N)
        out[:, lo:hi] = critic.values_device(o, a, ch).view(n, hi - lo)
    return out


SCENARIOS = {
    # name: (scenario, params, envs, policies)
    "pp4_chunk": ("pp", dict(map_=10, sen=1, N=4, M=4, teRcom=2, tepl=0.3), 32, 1),
    "pp4_multi": ("pp", dict(map_=10, sen=1, N=4, M=4, teRcom=2, tepl=0.3), 32, 2),
    "co24": ("co", dict(map_=20, sen=2, N=24, M=0, teRcom=6, tepl=0.3), 6, 1),
}
KEPT = ("obs", "actions", "probs", "reward64", "done", "details", "success", "path_len", "dist_adj", "channels")


@pytest.fixture(scope="module")
def played(gpu):
    """name -> (engine after one greedy round of T slots, clones of its buffers, what replay_values takes as critics): played once,
    shared, unchanged."""
    from com_marl_amd.nets import PolicySet
    from com_marl_amd.rollout import RolloutEngine
    out = {}
    for name, (scen, kw, B, K) in SCENARIOS.items():
        kw = dict(kw)
        params = cc.base_params(scen, kw.pop("map_"), kw.pop("sen"), kw.pop("N"), kw.pop("M"), max_env_steps=T, **kw)
        env = _wrapper(scen, params, B)
        batch = getattr(env, "env", env).batch
        pols = _policies(env, K)
        crit = _critics(env, K)
        ps = pols[0] if K == 1 else PolicySet(pols)
        ps.sync_weights()
        ps.reset([True] * (B // K))
        eng = RolloutEngine(batch, ps, T, store_attn=False, store_probs=True, **({} if K == 1 else dict(groups=[B // K] * K)))
        eng.reset()
        eng.play(0, T, greedy=True, chunk=True)
        eng.bump(T)
        batch.check_status()
        gpu.cuda.synchronize()
        keep = {k: getattr(eng, k).clone() for k in KEPT}
        keep["step_base"] = eng.step_base.clone()
        out[name] = (eng, keep, crit[0] if K == 1 else crit, pols, env)
    return out


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_replay_with_the_recorded_channels_equals_values_device_slot_by_slot(gpu, played, name):
    torch = gpu
    eng, keep, critics, pols, _ = played[name]
    B = eng.env.B
    steps = [p._policy_step for p in pols]
    out = torch.full((T, B), SENTINEL, device="cuda")
    assert eng.replay_values(0, T, "recorded", critics, out) is out
    for t in range(T):
        for critic, lo, hi in _members(eng, critics):
            want = critic.values_device(keep["obs"][t, lo:hi].reshape(hi - lo, -1), keep["dist_adj"][t, lo:hi], keep["channels"][t, lo:hi])
            assert torch.equal(out[t, lo:hi], want), f"{name}: slot {t}, envs {lo}..{hi - 1}: the replay is not values_device on the slot"
    assert float(out.std()) > 0
    mid = torch.full((2, B), SENTINEL, device="cuda")            # a span in the middle
    eng.replay_values(3, 2, "recorded", critics, mid)
    assert torch.equal(mid, out[3:5])
    eng.replay_values(0, T, "identity", critics, torch.empty_like(out))
    for k, v in keep.items():
        now = eng.step_base if k == "step_base" else getattr(eng, k)
        assert torch.equal(now, v), f"{name}: the replay changed {k}"
    assert [p._policy_step for p in pols] == steps
    for bad in (dict(t0=0, n=T + 1), dict(t0=-1, n=2), dict(t0=0, n=0)):
        with pytest.raises(ValueError, match="replay_values"):
            eng.replay_values(bad["t0"], bad["n"], "recorded", critics, out)
    with pytest.raises(ValueError, match="replay_values"):
        eng.replay_values(0, T, "FL", critics, out)
    with pytest.raises(ValueError, match="replay_values"):
        eng.replay_values(0, T, "ones", critics, out[:, :B - 1])
    with pytest.raises(ValueError, match="replay_values"):
        eng.replay_values(0, T, "ones", [critics] * 3 if not isinstance(critics, list) else critics[:1], out)


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_counterfactual_replays_equal_values_device_on_materialised_masks(gpu, played, name):
    torch = gpu
    eng, keep, critics, _, _ = played[name]
    B, Lh = eng.env.B, eng.env.Lh
    obs, adj, chan = keep["obs"][:T], keep["dist_adj"][:T], keep["channels"][:T]
    recorded = torch.empty(T, B, device="cuda")
    eng.replay_values(0, T, "recorded", critics, recorded)
    for kind in ("identity", "ones"):
        got = torch.full((T, B), SENTINEL, device="cuda")
        eng.replay_values(0, T, kind, critics, got)
        want = _by_values_device(torch, _members(eng, critics), obs, adj, chan, kind, Lh)
        assert torch.equal(got, want), f"{name} {kind}: the replay is not values_device on the materialised mask"
        assert not torch.equal(got, recorded)                               # the channel mattered somewhere


def test_the_identity_replay_in_several_launches_gives_the_same_bits(gpu, played, monkeypatch):
    """A mask bound that holds 40 env states: the 192 rows of the round take five launches on one block of 40 rows."""
    torch = gpu
    from com_marl_amd import rollout
    eng, _, critic, _, _ = played["pp4_chunk"]
    B, N, Lh = eng.env.B, eng.env.N, eng.env.Lh
    whole = torch.empty(T, B, device="cuda")
    eng.replay_values(0, T, "identity", critic, whole)
    monkeypatch.setattr(rollout, "REPLAY_MASK_BYTES", 40 * 4 * Lh * N * N)
    monkeypatch.setattr(eng, "_eye_rows", None)
    parts = torch.empty_like(whole)
    eng.replay_values(0, T, "identity", critic, parts)
    assert eng._eye_rows.shape[0] == 40 and torch.equal(parts, whole)


@pytest.mark.parametrize("kw", [dict(aggregator_type="direct"), dict(encoder_hidden_sizes=(32,), embedding_dim=32, decoder_hidden_sizes=(16,)),
                                dict(decoder_hidden_sizes=(32, 16))], ids=["direct", "small", "two-layer-head"])
def test_critics_of_other_aggregators_and_layer_sizes_take_values_devices_routes(gpu, played, kw):
    torch = gpu
    eng, keep, _, _, env = played["pp4_chunk"]
    critic = _critics(env, 1, **kw)[0]
    B, Lh = eng.env.B, eng.env.Lh
    for kind in ("recorded", "identity", "ones"):
        got = torch.full((T, B), SENTINEL, device="cuda")
        eng.replay_values(0, T, kind, critic, got)
        want = _by_values_device(torch, [(critic, 0, B)], keep["obs"][:T], keep["dist_adj"][:T], keep["channels"][:T], kind, Lh)
        assert torch.equal(got, want), (kw, kind)
        assert torch.isfinite(got).all() and float(got.std()) > 0


def test_a_baseline_without_a_graph_input_replays_the_recorded_slots_only(gpu, played):
    torch = gpu
    from com_marl_amd import nets
    eng, keep, _, _, env = played["pp4_chunk"]
    torch.manual_seed(5)
    base = nets.GaussianMLPBaseline(env.spec, device="cuda:0")
    base.sync_weights()
    B = eng.env.B
    got = torch.full((T, B), SENTINEL, device="cuda")
    eng.replay_values(0, T, "recorded", base, got)
    for t in range(T):
        assert torch.equal(got[t], base.values_device(keep["obs"][t].reshape(B, -1)))
    for kind in ("identity", "ones"):
        with pytest.raises(ValueError, match="replay_values"):
            eng.replay_values(0, T, kind, base, got)


# ---- eval_summary / eval_sweep ------------------------------------------------------------------------------------------------
TE = 12                                                         # max_env_steps of the end-to-end scenarios


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
            self.rounds.append({name: keep(getattr(self, name)) for name in ("obs", "dist_adj", "channels", "path_len", "reward64")})
            return out

    monkeypatch.setattr(evaluate, "RolloutEngine", Spy)
    return used


def _expected(torch, eng, critics, E, n_epi, gamma):
    """The rounds a spied engine played -> (episode table [cells, n_epi, 6], curve means [cells, TE, 6], atol [6]) by the
    restatement, from the engine's own rewards and path_len and the critics' values computed here by values_device (the
    counterfactual ones on materialised masks; none for critics without a graph input)."""
    batch = eng.env
    B, Lh = batch.B, batch.Lh
    cells = B // E
    table = np.zeros((cells * n_epi, R.EPV_COLS))
    sums = np.zeros((cells, TE, R.VALUE_COLS))
    atol = np.zeros(R.VALUE_COLS)
    members = _members(eng, critics)
    graph = hasattr(members[0][0], "comm")
    done = 0
    for r in eng.rounds:
        cut = lambda x: None if x is None else x[:TE]                        # noqa: E731
        v, mute, lossless = ((_by_values_device(torch, members, cut(r["obs"]), cut(r["dist_adj"]), cut(r["channels"]), kind, Lh).cpu().numpy()
                              if kind == "recorded" or graph else None) for kind in ("recorded", "identity", "ones"))
        rewards, pl = r["reward64"][:TE].cpu().numpy(), r["path_len"][:TE].cpu().numpy()
        stats = R.value_stats(rewards, pl, v, mute, lossless, gamma)
        atol = np.maximum(atol, R.env_atol(rewards, v).max(0))
        take = min(E, n_epi - done)
        R.episode_value(pl, stats, E, take, n_epi, done, table)
        R.value_curves(pl, stats, E, take, int(done > 0), sums)
        done += take
    assert done == n_epi
    return table.reshape(cells, n_epi, R.EPV_COLS), R.value_curve_means(sums, n_epi), atol


def _key_atols(row, atol):
    """What the column tolerances `atol` [6] of a row of means allow the VALUE_KEYS to differ by: bias is a difference of two
    columns; rmse = sqrt(m2) moves by d / (2 rmse) (by sqrt(d) at 0); ev = 1 - resid / var with resid = m2 - bias^2 and
    var = m3 - m1^2 moves by (d_resid + |1 - ev| d_var) / var, d_resid = a2 + 4 |bias| a and d_var = a2 + 2 |m1| a; on the
    degenerate branch (var <= eps) the two sides must agree exactly unless resid is within d_resid of eps."""
    k = R.keys(row)
    a, a2 = float(atol[0]), float(atol[2])
    rmse = k["value_rmse"]
    var = row[3] - row[1] * row[1]
    eps = 1e-12 * max(1.0, row[3])
    d_resid, d_var = a2 + 4 * abs(k["value_bias"]) * a, a2 + 2 * abs(row[1]) * a
    ev = 0.0 if var <= eps else (d_resid + abs(1 - k["value_ev"]) * d_var) / var * 2
    return dict(value_mean=a, value_return=a, value_bias=2 * a, value_rmse=a2 / (2 * rmse) if rmse * rmse > a2 else math.sqrt(a2) + a2,
                value_ev=ev, msg_value=a, loss_value=a)


def _check_cell(d, table, curves, atol, what):
    from com_marl_amd.evaluate import VALUE_KEYS
    assert set(VALUE_KEYS) <= set(d)
    ep = d["value_episodes"]
    assert ep.is_cuda and tuple(ep.shape) == table.shape
    _close(ep.cpu().numpy(), table, atol, what + " value_episodes")
    row = R.value_means(table[None])[0]
    want, tol = R.keys(row), _key_atols(row, atol)
    for k in VALUE_KEYS:
        _close(d[k], want[k], tol[k], f"{what} {k}")
    step_cnt = d["curves"]["step_cnt"]
    want = R.curve_keys(curves, step_cnt)
    for t in range(TE):
        s = step_cnt[t]
        tol = _key_atols(curves[t] / s, atol / s) if s > 0 else dict.fromkeys(VALUE_KEYS, 0.0)
        for k in VALUE_KEYS:
            zero_padded = k not in ("value_rmse", "value_ev")
            _close(d["curves"][k][t], want[k][t], atol[0] * (2 if k == "value_bias" else 1) if zero_padded else tol[k], f"{what} curve {k}[{t}]")
    assert all(d["curves"][k].shape == (TE,) for k in VALUE_KEYS)
    assert d["value_rmse"] >= 0 and d["value_bias"] == d["value_mean"] - d["value_return"]


CONDS = [dict(Rcom=9, pl=0), dict(Rcom=2, pl=0.3)]
ALL = dict(value_stats=True, curves=True, episodes=True)


def test_eval_summary_of_two_policies_equals_the_restatement_on_the_engines_buffers(gpu, spy):
    """PP map 10, teams of 4, 32 envs = 2 policies x 16, IID pl = 0.3 with Rcom = 2, 24 episodes each: a full round and one of 8."""
    from com_marl_amd.evaluate import eval_summary
    params = cc.base_params("pp", 10, 1, 4, 4, max_env_steps=TE, teRcom=2, tepl=0.3)
    env = _wrapper("pp", params, 32)
    critics = _critics(env, 2)
    got = eval_summary(env, _policies(env, 2), 0, n_eval_episodes=24, max_env_steps=TE, baselines=critics, discount=0.95, **ALL)
    assert len(spy) == 1 and len(spy[0].rounds) == 2
    table, curves, atol = _expected(gpu, spy[0], critics, 16, 24, 0.95)
    for k in range(2):
        _check_cell(got[k], table[k], curves[k], atol, f"policy {k}")
        assert got[k]["msg_value"] != 0 and got[k]["loss_value"] != 0 and got[k]["value_rmse"] > 0
    assert got[0]["value_mean"] != got[1]["value_mean"]                     # critic k judged policy k's envs


def test_eval_sweep_of_two_conditions_equals_the_restatement_and_a_lossless_condition_loses_nothing(gpu, spy):
    """2 policies x 2 conditions x 8 envs, 12 episodes per cell: a full round and one of 4.  The first condition loses nothing:
    its recorded channels are all ones, so the lossless replay repeats the recorded one bit for bit."""
    from com_marl_amd.evaluate import eval_sweep
    params = cc.base_params("pp", 10, 1, 4, 4, max_env_steps=TE)
    env = _wrapper("pp", params, 32, "IID", conditions=CONDS)
    critics = _critics(env, 2)
    got = eval_sweep(env, _policies(env, 2), 0, n_eval_episodes=12, max_env_steps=TE, baselines=critics, **ALL)
    assert len(spy) == 1 and len(spy[0].rounds) == 2
    table, curves, atol = _expected(gpu, spy[0], critics, 8, 12, 0.99)
    for k in range(2):
        for c in range(2):
            _check_cell(got[k][c], table[2 * k + c], curves[2 * k + c], atol, f"cell {k},{c}")
        full, lossy = got[k]
        assert full["loss_value"] == 0.0 and (full["curves"]["loss_value"] == 0.0).all()
        assert (full["value_episodes"][:, 5] == 0).all()
        assert lossy["loss_value"] != 0 and lossy["msg_value"] != 0 and full["msg_value"] != 0


def test_eval_summary_coverage_teams_of_24(gpu, spy):
    """Coverage map 20, N = 24, 6 envs, one policy and its critic, 9 episodes: a full round and one of 3."""
    from com_marl_amd.evaluate import eval_summary
    params = cc.base_params("co", 20, 2, 24, 0, max_env_steps=TE, teRcom=6, tepl=0.3)
    env = _wrapper("co", params, 6)
    critic = _critics(env, 1)[0]
    got = eval_summary(env, _policies(env, 1)[0], 0, n_eval_episodes=9, max_env_steps=TE, baselines=critic, **ALL)
    assert isinstance(got, dict) and len(spy) == 1 and len(spy[0].rounds) == 2
    table, curves, atol = _expected(gpu, spy[0], critic, 6, 9, 0.99)
    _check_cell(got, table[0], curves[0], atol, "coverage")


CRITIC_FORWARDS = ("cm_critic_forward", "cm_critic_forward_any")


@pytest.mark.parametrize("kind", ["cent", "dec"])
def test_a_policy_without_messages_and_its_mlp_baseline(gpu, spy, lib_spy, kind):  # noqa: F811
    """A CENT / an Obs-DP policy with a GaussianMLPBaseline: msg_value and loss_value exactly 0 and ONE baseline forward per round."""
    import torch
    from com_marl_amd import nets
    from com_marl_amd.evaluate import eval_summary
    params = cc.base_params("pp", 10, 1, 4, 4, max_env_steps=TE, teRcom=2, tepl=0.3)
    env = _wrapper("pp", params, 16)
    torch.manual_seed(11)
    cls = nets.CentralizedCategoricalMLPPolicy if kind == "cent" else nets.DecCategoricalMLPPolicy
    pol = cls(env.spec, n_agents=env.n_agents, device="cuda:0")
    pol.set_rng(3)
    base = nets.GaussianMLPBaseline(env.spec, device="cuda:0")
    lib_spy.calls.clear()
    got = eval_summary(env, pol, 0, n_eval_episodes=24, max_env_steps=TE, baselines=base, **ALL)
    assert len(spy[0].rounds) == 2
    assert lib_spy.count("cm_mlp_value_forward") == 2 and not [c for c in lib_spy.calls if c in CRITIC_FORWARDS]
    assert [c.args[1] for c in lib_spy.calls if c == "cm_mlp_value_forward"] == [TE * 16] * 2
    assert [(c.args[5], c.args[6]) for c in lib_spy.calls if c == "cm_value_stats"] == [(None, None)] * 2     # NULL counterfactuals
    table, curves, atol = _expected(gpu, spy[0], base, 16, 24, 0.99)
    _check_cell(got, table[0], curves[0], atol, kind)
    assert got["msg_value"] == 0.0 and got["loss_value"] == 0.0 and (got["value_episodes"][:, 4:] == 0).all()
    assert (got["curves"]["msg_value"] == 0).all() and (got["curves"]["loss_value"] == 0).all()


def test_a_constant_channel_skips_its_replay(gpu, spy, lib_spy):  # noqa: F811
    """FC (tepl = 0): no lossless replay - loss_value exactly 0 and TWO critic forwards per slot's envs, not three; FL (tepl = 1):
    no mute replay - msg_value exactly 0.  One policy, 16 envs, 16 episodes: one round.  Counted: the env states that went through
    a critic forward."""
    from com_marl_amd.evaluate import eval_summary

    def forwards(tepl):
        params = cc.base_params("pp", 10, 1, 4, 4, max_env_steps=TE, teRcom=2, tepl=tepl)
        env = _wrapper("pp", params, 16)
        lib_spy.calls.clear()
        got = eval_summary(env, _policies(env, 1)[0], 0, n_eval_episodes=16, max_env_steps=TE, baselines=_critics(env, 1)[0], **ALL)
        rows = sum(c.args[1] for c in lib_spy.calls if c in CRITIC_FORWARDS)
        return got, rows, spy[-1]

    fc, fc_rows, eng = forwards(0.0)
    assert eng.channels is None and eng.env.channelType == "FC"
    assert fc_rows == 2 * TE * 16                                            # recorded and mute
    assert fc["loss_value"] == 0.0 and (fc["curves"]["loss_value"] == 0.0).all() and (fc["value_episodes"][:, 5] == 0).all()
    assert fc["msg_value"] != 0
    lossy, lossy_rows, _ = forwards(0.3)
    assert lossy_rows == 3 * TE * 16                                         # all three under a channel that varies
    fl, fl_rows, eng = forwards(1.0)
    assert eng.channels is None and eng.env.channelType == "FL"
    assert fl_rows == 2 * TE * 16                                            # recorded and lossless
    assert fl["msg_value"] == 0.0 and (fl["curves"]["msg_value"] == 0.0).all() and (fl["value_episodes"][:, 4] == 0).all()


def test_switched_off_nothing_is_launched_or_returned_and_the_rest_is_bit_equal(gpu, spy, lib_spy):  # noqa: F811
    import torch
    from com_marl_amd.evaluate import VALUE_KEYS, eval_summary
    params = cc.base_params("pp", 10, 1, 4, 4, max_env_steps=TE, teRcom=2, tepl=0.3)
    kw = dict(n_eval_episodes=24, max_env_steps=TE, comm_stats=True, attn_stats=True, listen_stats=True, curves=True, episodes=True)
    pols = _policies(_wrapper("pp", params, 32), 2)
    plain = eval_summary(_wrapper("pp", params, 32), pols, 0, **kw)
    off = eval_summary(_wrapper("pp", params, 32), pols, 0, value_stats=False, baselines=None, **kw)
    assert not [c for c in lib_spy.calls if "value" in c or c in CRITIC_FORWARDS]
    env = _wrapper("pp", params, 32)
    on = eval_summary(env, pols, 0, value_stats=True, baselines=_critics(env, 2), **kw)
    n_rounds = 2
    for name, n in (("cm_value_stats", n_rounds), ("cm_episode_value", n_rounds), ("cm_value_curves", n_rounds), ("cm_value_means", 1),
                    ("cm_value_curve_means", 1), ("cm_critic_forward", 3 * 2 * n_rounds)):
        assert lib_spy.count(name) == n, name
    for a, b, c in zip(plain, off, on):
        assert not set(VALUE_KEYS) & set(a) and "value_episodes" not in a and not set(VALUE_KEYS) & set(a["curves"])
        assert set(b) == set(a) and set(b["curves"]) == set(a["curves"])
        assert set(c) == set(a) | set(VALUE_KEYS) | {"value_episodes"} and set(c["curves"]) == set(a["curves"]) | set(VALUE_KEYS)
        for key, v in a.items():
            for other in (b, c):
                if key.endswith("episodes") and key != "n_episodes":
                    assert torch.equal(v, other[key]), key
                elif key == "curves":
                    for name, curve in v.items():
                        np.testing.assert_array_equal(curve, other[key][name], err_msg=name)
                else:
                    assert v == other[key], key


def test_refusals_come_before_anything_is_built(gpu, spy):
    from com_marl_amd import nets
    from com_marl_amd.evaluate import eval_summary, eval_sweep
    params = cc.base_params("pp", 10, 1, 4, 4, max_env_steps=TE)
    env = _wrapper("pp", params, 32)
    pols, crit = _policies(env, 2), _critics(env, 2)
    base = nets.GaussianMLPBaseline(env.spec, device="cuda:0")
    co = _wrapper("co", cc.base_params("co", 20, 2, 24, 0, max_env_steps=TE, teRcom=6), 6)
    for policies, kw in ((pols, dict(value_stats=True)), (pols, dict(baselines=crit)), (pols, dict(value_stats=True, baselines=crit[:1])),
                         (pols[0], dict(value_stats=True, baselines=crit)), (pols, dict(value_stats=True, baselines=[crit[0], base])),
                         (pols, dict(value_stats=True, baselines=[crit[0], pols[1]])),
                         (pols[0], dict(value_stats=True, baselines=_critics(co, 1)[0]))):
        with pytest.raises(ValueError, match="value_stats"):
            eval_summary(env, policies, 0, n_eval_episodes=8, max_env_steps=TE, **kw)
    cenv = _wrapper("pp", params, 32, "IID", conditions=CONDS)
    with pytest.raises(ValueError, match="value_stats"):
        eval_sweep(cenv, pols, 0, n_eval_episodes=8, max_env_steps=TE, value_stats=True)
    assert spy == []
