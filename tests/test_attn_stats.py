"""cm_attn_stats and its reductions (csrc/cm_attn_stats.hip) through ctypes, envs.attn_stats and eval_summary / eval_sweep with
attn_stats=True, against the numpy float64 restatement (tests/attn_stats_ref.py).  Both sides compute in f64 from the same f32
inputs: rtol = 1e-10 with atol = 1e-12 N L per graph and 1e-12 on episode rows, means and curves (the reasoning is in the
restatement's docstring); every comparison prints the largest error it saw.  Repeated launches are compared bit for bit.

Shapes: every team-size class of the kernel (N = 1, 2, 3-4, 5-8 on 1 / 2 / 4 / 8 lanes per graph; N >= 9 on one wave per graph with
1 .. 4 rows per lane), N % 4 == 0 on the 16-byte loads and the others on the one-float loads, the three hop classes (L <= 2, <= 4,
<= 8), S = 37 and 130 so that the last workgroup and the last wave are ragged."""
import numpy as np
import pytest

from tests import attn_stats_ref as R, conditions_common as cc

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
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want)
    rel = err / np.maximum(np.abs(want), 1e-300)
    print(f"{what}: max |error| {err.max():.3e}, max relative error {rel[np.abs(want) > atol].max(initial=0.0):.3e} "
          f"(rtol {R.RTOL:g}, atol {atol:g})")
    np.testing.assert_allclose(got, want, rtol=R.RTOL, atol=atol, err_msg=what)


def _dev(torch, x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _launch(torch, S, N, Lh, attn, adj, chan, attn_stride=None, adj_stride=None, chan_stride=None):
    """One cm_attn_stats launch on device tensors (or None = NULL) into a sentinel-filled table with guard rows -> the whole table."""
    from com_marl_amd import _lib as L
    out = torch.full((S + 2 * GUARD, R.ATTN_COLS), SENTINEL, dtype=torch.float64, device="cuda")
    t_st = N * N if attn_stride is None else attn_stride
    a_st = N * N if adj_stride is None else adj_stride
    c_st = Lh * N * N if chan_stride is None else chan_stride
    L.check(L.lib().cm_attn_stats(S, N, Lh, L.ptr(attn), t_st, L.ptr(adj), a_st, L.ptr(chan), c_st, L.ptr(out[GUARD:]),
                                  L.current_stream()), "cm_attn_stats")
    return out.cpu().numpy()


def _check(torch, S, N, Lh, attn, adj, chan, want, what, **strides):
    """Host arrays (adj / chan: [S,...], one block with stride 0, or None).  Two launches: the same bits, guards untouched."""
    dev = [_dev(torch, x) for x in (attn, adj, chan)]
    got = _launch(torch, S, N, Lh, *dev, **strides)
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + S:] == SENTINEL).all(), "guard rows written"
    _close(got[GUARD:GUARD + S], want, R.graph_atol(N, Lh), what)
    np.testing.assert_array_equal(_launch(torch, S, N, Lh, *dev, **strides), got)
    return got[GUARD:GUARD + S]


# every N class, both L extremes at small and large N, each hop class on the wave kernel
GRID = [(1, 1, 130), (2, 2, 130), (3, 8, 130), (4, 2, 130), (4, 1, 37), (5, 3, 130), (8, 8, 130), (8, 2, 37), (9, 1, 130), (24, 3, 130),
        (24, 2, 37), (64, 2, 37), (65, 8, 37), (72, 2, 37), (129, 1, 37), (255, 2, 37), (255, 8, 37)]


@pytest.mark.parametrize("N,Lh,S", GRID, ids=[f"N{N}-L{Lh}-S{S}" for N, Lh, S in GRID])
def test_seeded_graphs_equal_the_restatement(gpu, N, Lh, S):
    """f32 softmax rows of logits scaled by 8 with a planted zero, one-hot rows and a row whose kept set is empty; masks at
    density 0.5.  A prefix of the graphs gives the same rows as the full launch."""
    attn, adj, chan = R.seeded(S, N, Lh, seed=1000 * Lh + N)
    want = R.attn_stats(attn, adj, chan, N, Lh)
    got = _check(gpu, S, N, Lh, attn, adj, chan, want, f"N={N} L={Lh} S={S}")
    if S > 4 and N > 1:
        assert want[1, 1] == 0 and want[1, 5] == 0 and want[1, 0] == N          # one-hot rows on the diagonal
        assert got[1, 1] == 0 and got[1, 0] == N
    P = S // 2 + 1
    d = [_dev(gpu, x[:P]) for x in (attn, adj, chan)]
    np.testing.assert_array_equal(_launch(gpu, P, N, Lh, *d)[GUARD:GUARD + P], got[:P])
    one = [_dev(gpu, x[S - 1:]) for x in (attn, adj, chan)]
    np.testing.assert_array_equal(_launch(gpu, 1, N, Lh, *one)[GUARD:GUARD + 1], got[S - 1:])


@pytest.mark.parametrize("N", [3, 4, 8, 24, 72, 129])
def test_null_arrays_are_ones_and_stride_zero_shares_a_block(gpu, N):
    torch = gpu
    S, Lh = 9, 2
    attn, adj, chan = R.seeded(S, N, Lh, seed=50 + N)
    ones_a, ones_c = np.ones((S, N, N), np.float32), np.ones((S, Lh, N, N), np.float32)
    _check(torch, S, N, Lh, attn, None, chan, R.attn_stats(attn, ones_a, chan, N, Lh), "NULL dist_adj")
    _check(torch, S, N, Lh, attn, adj, None, R.attn_stats(attn, adj, ones_c, N, Lh), "NULL channels")
    both = _check(torch, S, N, Lh, attn, None, None, R.attn_stats(attn, ones_a, ones_c, N, Lh), "both NULL")
    np.testing.assert_allclose(both[:, 2], N, rtol=1e-5)                  # every row's whole mass is in range and kept
    np.testing.assert_allclose(both[:, 3], N * Lh, rtol=1e-5)
    np.testing.assert_allclose(both[:, 4], Lh * both[:, 0], rtol=1e-5)    # nothing masked: the weights are M, renormalised to 1
    # stride 0: every graph reads graph 1's block
    _check(torch, S, N, Lh, attn, adj[1], chan, R.attn_stats(attn, np.stack([adj[1]] * S), chan, N, Lh), "adj stride 0", adj_stride=0)
    _check(torch, S, N, Lh, attn, adj, chan[1], R.attn_stats(attn, adj, np.stack([chan[1]] * S), N, Lh), "chan stride 0",
           chan_stride=0)
    # the identity as the shared block - a constant FL channel: every agent attends to itself alone
    eye = np.ascontiguousarray(np.broadcast_to(np.eye(N, dtype=np.float32), (Lh, N, N)))
    fl = _check(torch, S, N, Lh, attn, None, eye, R.attn_stats(attn, None, eye, N, Lh), "FL channel", chan_stride=0)
    np.testing.assert_allclose(fl[:, 3], Lh * fl[:, 0], rtol=1e-12)
    np.testing.assert_allclose(fl[:, 5], 0.0, atol=R.graph_atol(N, Lh))      # one kept entry has no entropy
    assert (fl[:, 4] <= N * Lh).all() and (fl[:, 4] >= N * Lh - 2 * Lh).all()     # 1 per row and hop, bar the rows with M[i][i] == 0


@pytest.mark.parametrize("N", [4, 8, 24])
def test_strides_past_the_block_and_buffers_off_16_byte_alignment(gpu, N):
    """Blocks 3 floats apart at an address 4 bytes past a 16-byte boundary take the one-float loads: the same bits as the 16-byte
    loads on the same values, aligned and packed."""
    torch = gpu
    from com_marl_amd import _lib as L
    S, Lh = 11, 2
    attn, adj, chan = R.seeded(S, N, Lh, seed=80 + N)
    want = R.attn_stats(attn, adj, chan, N, Lh)
    packed = _check(torch, S, N, Lh, attn, adj, chan, want, "aligned")

    def spread(x, block):
        flat = torch.full((1 + S * (block + 3),), 9.0, dtype=torch.float32, device="cuda")
        view = flat[1:].view(S, block + 3)
        view[:, :block] = torch.from_numpy(x.reshape(S, block)).cuda()
        assert view.data_ptr() % 16 == 4
        return view
    d_attn, d_adj, d_chan = spread(attn, N * N), spread(adj, N * N), spread(chan, Lh * N * N)
    out = torch.full((S, R.ATTN_COLS), SENTINEL, dtype=torch.float64, device="cuda")
    L.check(L.lib().cm_attn_stats(S, N, Lh, d_attn.data_ptr(), N * N + 3, d_adj.data_ptr(), N * N + 3, d_chan.data_ptr(),
                                  Lh * N * N + 3, L.ptr(out), L.current_stream()), "cm_attn_stats")
    np.testing.assert_array_equal(out.cpu().numpy(), packed)
    # only the attention off alignment; and aligned blocks a whole 16 bytes apart stay on the 16-byte loads
    out.fill_(SENTINEL)
    p_adj, p_chan = _dev(torch, adj), _dev(torch, chan)
    L.check(L.lib().cm_attn_stats(S, N, Lh, d_attn.data_ptr(), N * N + 3, L.ptr(p_adj), N * N, L.ptr(p_chan), Lh * N * N, L.ptr(out),
                                  L.current_stream()), "cm_attn_stats")
    np.testing.assert_array_equal(out.cpu().numpy(), packed)
    wide = torch.zeros(S, N * N + 4, dtype=torch.float32, device="cuda")
    wide[:, :N * N] = torch.from_numpy(attn.reshape(S, N * N)).cuda()
    got = _launch(torch, S, N, Lh, wide, p_adj, p_chan, attn_stride=N * N + 4)
    np.testing.assert_array_equal(got[GUARD:GUARD + S], packed)


def test_no_graphs_write_nothing_and_refusals_set_the_error_text(gpu):
    torch = gpu
    from com_marl_amd import _lib as L
    lib = L.lib()
    attn, adj, chan = R.seeded(4, 4, 2, seed=3)
    d = [_dev(torch, x) for x in (attn, adj, chan)]
    assert (_launch(torch, 0, 4, 2, *d) == SENTINEL).all()
    out = torch.full((4, R.ATTN_COLS), SENTINEL, dtype=torch.float64, device="cuda")
    st = L.current_stream()
    for args in ((4, 0, 2, 16, 16, 32), (4, 256, 2, 16, 16, 32), (4, 4, 0, 16, 16, 32), (4, 4, 9, 16, 16, 32), (4, 4, 2, 15, 16, 32),
                 (4, 4, 2, 0, 16, 32), (4, 4, 2, 16, 15, 32), (4, 4, 2, 16, 16, 31), (-1, 4, 2, 16, 16, 32)):
        S, N, Lh, t_st, a_st, c_st = args
        assert lib.cm_attn_stats(S, N, Lh, L.ptr(d[0]), t_st, L.ptr(d[1]), a_st, L.ptr(d[2]), c_st, L.ptr(out), st) == -1, args
        assert b"cm_attn_stats" in lib.cm_last_error(), args
    for at, o in ((None, L.ptr(out)), (L.ptr(d[0]), None)):
        assert lib.cm_attn_stats(4, 4, 2, at, 16, L.ptr(d[1]), 16, L.ptr(d[2]), 32, o, st) == -1
        assert b"cm_attn_stats" in lib.cm_last_error()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()


def test_envs_attn_stats_takes_leading_shapes_and_none_masks(gpu):
    torch = gpu
    from com_marl_amd import envs
    S, N, Lh = 12, 5, 3
    attn, adj, chan = R.seeded(S, N, Lh, seed=9)
    d_attn, d_adj, d_chan = (_dev(torch, x) for x in (attn, adj, chan))
    got = envs.attn_stats(d_attn, d_adj, d_chan, Lh)
    assert got.shape == (S, 6) and got.dtype == torch.float64 and got.is_cuda
    _close(got.cpu().numpy(), R.attn_stats(attn, adj, chan, N, Lh), R.graph_atol(N, Lh), "envs.attn_stats")
    two = envs.attn_stats(d_attn.view(3, 4, N, N), None, d_chan.view(3, 4, Lh, N, N), Lh)
    assert two.shape == (3, 4, 6)
    _close(two.cpu().numpy().reshape(S, 6), R.attn_stats(attn, None, chan, N, Lh), R.graph_atol(N, Lh), "envs.attn_stats, no adj")
    out = torch.empty(S, 6, dtype=torch.float64, device="cuda")
    assert envs.attn_stats(d_attn, d_adj, None, Lh, out=out) is out
    _close(out.cpu().numpy(), R.attn_stats(attn, adj, None, N, Lh), R.graph_atol(N, Lh), "envs.attn_stats, no channels")


# ---- the reductions -----------------------------------------------------------------------------------------------------------
def _groupings(B):
    out = [(1, 1, 2, 4)]
    for g in (3, 5, 13):
        if B % g == 0 and g < B:
            out.append((g, g - 1, 1, g + 2))
    if B > 1:
        out.append((B, B - 1, 3, B + 3))
    return out


def _stats_rows(T, B, N, Lh, seed):
    """Rows as cm_attn_stats writes them: non-negative, up to N (columns 0-2) or N L (columns 3-5) times ln N."""
    rng = np.random.default_rng(seed)
    return rng.random((T, B, R.ATTN_COLS)) * np.array([N] * 3 + [N * Lh] * 3) * max(1.0, np.log(N))


@pytest.mark.parametrize("T,B,N,Lh", [(7, 1, 4, 2), (7, 3, 1, 1), (7, 65, 4, 2), (7, 130, 24, 3), (70, 9, 5, 8)])
@pytest.mark.parametrize("kind", ["none", "all0", "mixed"])
def test_episode_rows_and_curves_equal_the_restatement(gpu, T, B, N, Lh, kind):
    """take < group_size and row0 > 0 throughout; T = 70: an episode longer than one round of 64 lanes and more than one tile."""
    torch = gpu
    from com_marl_amd import _lib as L
    lib, st = L.lib(), L.current_stream()
    path_len = R.path_lens(T, B, seed=11 * T + B, kind=kind)
    stats = _stats_rows(T, B, N, Lh, seed=T + B)
    d_pl, d_st = torch.from_numpy(path_len).cuda(), torch.from_numpy(stats).cuda()
    for g, take, row0, epg in _groupings(B):
        rows, groups = B // g * epg, B // g
        want = np.full((rows, R.EPA_COLS), SENTINEL)
        R.episode_attn(path_len, stats, N, Lh, g, take, epg, row0, want)
        outs = []
        for _ in range(2):
            out = torch.full((rows + 2 * GUARD, R.EPA_COLS), SENTINEL, dtype=torch.float64, device="cuda")
            L.check(lib.cm_episode_attn(T, B, N, Lh, L.ptr(d_pl), L.ptr(d_st), g, take, epg, row0, L.ptr(out[GUARD:]), st),
                    "cm_episode_attn")
            outs.append(out.cpu().numpy())
        np.testing.assert_array_equal(outs[0], outs[1])
        got = outs[0]
        assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + rows:] == SENTINEL).all(), "guard rows written"
        named = want[:, 0] != SENTINEL
        assert named.sum() == groups * take
        np.testing.assert_array_equal(got[GUARD:GUARD + rows][~named], SENTINEL)          # the other rows keep the sentinel
        _close(got[GUARD:GUARD + rows][named], want[named], 1e-12, f"episode rows g={g}")

        # curves: a first launch overwrites, a second adds; then the means over 2 * take episodes
        want_sums = np.full((groups, T, R.ATTN_COLS), SENTINEL)
        R.attn_curves(path_len, stats, g, take, 0, want_sums)
        R.attn_curves(path_len, stats, g, take, 1, want_sums)
        outs = []
        for _ in range(2):
            sums = torch.full((groups + 2, T, R.ATTN_COLS), SENTINEL, dtype=torch.float64, device="cuda")
            for acc in (0, 1):
                L.check(lib.cm_attn_curves(T, B, N, Lh, L.ptr(d_pl), L.ptr(d_st), g, take, acc, L.ptr(sums[1:]), st), "cm_attn_curves")
            curves = torch.full((groups + 2, T, R.EPA_COLS), SENTINEL, dtype=torch.float64, device="cuda")
            L.check(lib.cm_attn_curve_means(groups, T, 2 * take, N, Lh, L.ptr(sums[1:]), L.ptr(curves[1:]), st), "cm_attn_curve_means")
            outs.append((sums.cpu().numpy(), curves.cpu().numpy()))
        for a, b in zip(outs[0], outs[1]):
            np.testing.assert_array_equal(a, b)
        sums, curves = outs[0]
        for t in (sums, curves):
            assert (t[0] == SENTINEL).all() and (t[-1] == SENTINEL).all(), "guard blocks written"
        _close(sums[1:-1], want_sums, 1e-12, f"curve sums g={g}")
        _close(curves[1:-1], R.attn_curve_means(want_sums, 2 * take, N, Lh), 1e-12, f"curve means g={g}")


@pytest.mark.parametrize("K,E", [(1, 1), (3, 5), (2, 65)])
def test_means_equal_the_restatement(gpu, K, E):
    torch = gpu
    from com_marl_amd import _lib as L
    table = np.random.default_rng(K * 1000 + E).random((K, E, R.EPA_COLS)) * 3.0
    dev = torch.from_numpy(table).cuda()
    outs = []
    for _ in range(2):
        out = torch.full((K + 2 * GUARD, R.EPA_COLS), SENTINEL, dtype=torch.float64, device="cuda")
        L.check(L.lib().cm_attn_means(K, E, L.ptr(dev), L.ptr(out[GUARD:]), L.current_stream()), "cm_attn_means")
        outs.append(out.cpu().numpy())
    np.testing.assert_array_equal(outs[0], outs[1])
    got = outs[0]
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + K:] == SENTINEL).all(), "guard rows written"
    _close(got[GUARD:GUARD + K], R.attn_means(table), 1e-12, "means")


# ---- eval_summary / eval_sweep ------------------------------------------------------------------------------------------------
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


@pytest.fixture
def spy(monkeypatch):
    """-> the list of engines the evaluation built; each keeps host copies of what every round left in its buffers."""
    from com_marl_amd import evaluate
    used = []

    class Spy(evaluate.RolloutEngine):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.rounds = []
            used.append(self)

        def bump(self, *a, **kw):
            out = super().bump(*a, **kw)
            host = lambda x: None if x is None else x.cpu().numpy().copy()   # noqa: E731
            self.rounds.append({name: host(getattr(self, name)) for name in ("attn", "dist_adj", "channels", "path_len")})
            return out

    monkeypatch.setattr(evaluate, "RolloutEngine", Spy)
    return used


def _expected(eng, E, n_epi):
    """The rounds a spied engine played -> (episode table [cells, n_epi, 6], curve means [cells, T, 6]) by the restatement, from
    the engine's own attn / dist_adj / channels / path_len buffers."""
    batch = eng.env
    B, N, Lh = batch.B, batch.N, batch.Lh
    cells = B // E
    table = np.zeros((cells * n_epi, R.EPA_COLS))
    sums = np.zeros((cells, T, R.ATTN_COLS))
    done = 0
    for r in eng.rounds:
        attn = r["attn"][:T].reshape(T * B, N, N)
        np.testing.assert_allclose(attn.sum(-1), 1.0, rtol=0, atol=(N + 4) * 2.0 ** -23)     # the buffer holds M, before any mask
        adj = None if r["dist_adj"] is None else r["dist_adj"][:T].reshape(T * B, N, N)
        if r["channels"] is not None:
            chan = r["channels"][:T].reshape(T * B, Lh, N, N)
        else:
            chan = None if batch.channelType == "FC" else batch.channels[0].cpu().numpy()
        stats = R.attn_stats(attn, adj, chan, N, Lh).reshape(T, B, R.ATTN_COLS)
        take = min(E, n_epi - done)
        R.episode_attn(r["path_len"][:T], stats, N, Lh, E, take, n_epi, done, table)
        R.attn_curves(r["path_len"][:T], stats, E, take, int(done > 0), sums)
        done += take
    assert done == n_epi
    return table.reshape(cells, n_epi, R.EPA_COLS), R.attn_curve_means(sums, n_epi, N, Lh)


def _check_cell(d, table, curves, what):
    from com_marl_amd.evaluate import ATTN_KEYS, COMM_KEYS
    assert set(ATTN_KEYS) <= set(d) and set(COMM_KEYS) <= set(d)
    ep = d["attn_episodes"]
    assert ep.is_cuda and tuple(ep.shape) == table.shape
    _close(ep.cpu().numpy(), table, 1e-12, what + " attn_episodes")
    _close([d[k] for k in ATTN_KEYS], R.attn_means(table[None])[0], 1e-12, what + " keys")
    _close(np.stack([d["curves"][k] for k in ATTN_KEYS], 1), curves, 1e-12, what + " curves")
    assert all(d["curves"][k].shape == (T,) for k in ATTN_KEYS)
    assert 0 < d["attn_self"] < 1 and 0 < d["attn_kept_mass"] <= d["attn_range_mass"] <= 1 + 1e-6
    assert d["attn_eff_entropy"] <= d["attn_entropy"] + 1e-6     # fewer links, sharper weights


CONDS = [dict(Rcom=9, pl=0), dict(Rcom=2, pl=0.3)]
ALL = dict(attn_stats=True, comm_stats=True, curves=True, episodes=True)


def test_eval_summary_of_two_policies_equals_the_restatement_on_the_engines_buffers(gpu, spy):
    """PP map 10, teams of 4, 32 envs = 2 policies x 16, IID pl = 0.3 with Rcom = 2, 24 episodes each: a full round and one of 8."""
    from com_marl_amd.evaluate import eval_summary
    params = cc.base_params("pp", 10, 1, 4, 4, max_env_steps=T, teRcom=2, tepl=0.3)
    env = _wrapper("pp", params, 32)
    got = eval_summary(env, _policies(env, 2), 0, n_eval_episodes=24, max_env_steps=T, **ALL)
    assert len(spy) == 1 and len(spy[0].rounds) == 2 and spy[0].attn is not None
    table, curves = _expected(spy[0], 16, 24)
    for k in range(2):
        _check_cell(got[k], table[k], curves[k], f"policy {k}")
        assert got[k]["attn_kept_mass"] < got[k]["attn_range_mass"] < 1 and got[k]["attn_eff_entropy"] < got[k]["attn_entropy"]


def test_eval_sweep_of_two_conditions_equals_the_restatement_on_the_engines_buffers(gpu, spy):
    """2 policies x 2 conditions x 8 envs, 12 episodes per cell: a full round and one of 4.  The first condition loses nothing."""
    from com_marl_amd.evaluate import eval_sweep
    params = cc.base_params("pp", 10, 1, 4, 4, max_env_steps=T)
    env = _wrapper("pp", params, 32, "IID", conditions=CONDS)
    got = eval_sweep(env, _policies(env, 2), 0, n_eval_episodes=12, max_env_steps=T, **ALL)
    assert len(spy) == 1 and len(spy[0].rounds) == 2
    table, curves = _expected(spy[0], 8, 12)
    for k in range(2):
        for c in range(2):
            _check_cell(got[k][c], table[2 * k + c], curves[2 * k + c], f"cell {k},{c}")
        full, lossy = got[k]
        assert full["attn_kept_mass"] == pytest.approx(1.0, abs=1e-6) and full["attn_eff_self"] == pytest.approx(full["attn_self"], rel=1e-6)
        assert lossy["attn_kept_mass"] < 1 - 1e-3 and lossy["attn_eff_entropy"] < full["attn_eff_entropy"]


def test_eval_summary_coverage_teams_of_24(gpu, spy):
    """Coverage map 20, N = 24 (one wave per graph), 6 envs, one policy, 9 episodes: a full round and one of 3."""
    from com_marl_amd.evaluate import eval_summary
    params = cc.base_params("co", 20, 2, 24, 0, max_env_steps=T, teRcom=6, tepl=0.3)
    env = _wrapper("co", params, 6)
    got = eval_summary(env, _policies(env, 1)[0], 0, n_eval_episodes=9, max_env_steps=T, **ALL)
    assert isinstance(got, dict) and len(spy) == 1 and len(spy[0].rounds) == 2
    table, curves = _expected(spy[0], 6, 9)
    _check_cell(got, table[0], curves[0], "coverage")


def test_switched_off_nothing_is_kept_or_returned_and_the_rest_is_bit_equal(gpu, spy):
    import torch
    from com_marl_amd.evaluate import ATTN_KEYS, eval_summary
    params = cc.base_params("pp", 10, 1, 4, 4, max_env_steps=T, teRcom=2, tepl=0.3)
    kw = dict(n_eval_episodes=24, max_env_steps=T, comm_stats=True, curves=True, episodes=True)
    env = _wrapper("pp", params, 32)
    pols = _policies(env, 2)
    off = eval_summary(env, pols, 0, attn_stats=False, **kw)
    assert len(spy) == 1 and spy[0].attn is None
    on = eval_summary(_wrapper("pp", params, 32), pols, 0, attn_stats=True, **kw)
    assert spy[1].attn is not None
    for a, b in zip(off, on):
        assert not set(ATTN_KEYS) & set(a) and "attn_episodes" not in a and not set(ATTN_KEYS) & set(a["curves"])
        assert set(b) == set(a) | set(ATTN_KEYS) | {"attn_episodes"} and set(b["curves"]) == set(a["curves"]) | set(ATTN_KEYS)
        for key, v in a.items():
            if key in ("episodes", "comm_episodes"):
                assert torch.equal(v, b[key]), key
            elif key == "curves":
                for name, curve in v.items():
                    np.testing.assert_array_equal(curve, b[key][name], err_msg=name)
            else:
                assert v == b[key], key


def test_a_policy_without_attention_is_refused(gpu, spy):
    from com_marl_amd import nets
    from com_marl_amd.evaluate import eval_summary, eval_sweep
    params = cc.base_params("pp", 10, 1, 4, 4, max_env_steps=T)
    env = _wrapper("pp", params, 32)
    dec = nets.DecCategoricalMLPPolicy(env.spec, n_agents=env.n_agents, device="cuda:0")
    with pytest.raises(ValueError, match="attn_stats"):
        eval_summary(env, dec, 0, n_eval_episodes=8, max_env_steps=T, attn_stats=True)
    with pytest.raises(ValueError, match="attn_stats"):
        eval_summary(env, [dec, dec], 0, n_eval_episodes=8, max_env_steps=T, attn_stats=True)
    cenv = _wrapper("pp", params, 32, "IID", conditions=CONDS)
    with pytest.raises(ValueError, match="attn_stats"):
        eval_sweep(cenv, dec, 0, n_eval_episodes=8, max_env_steps=T, attn_stats=True)
    assert spy == []                                             # refused before anything is built
