"""cm_comm_stats / cm_episode_comm / cm_comm_means (csrc/cm_comm_stats.hip) through ctypes, and envs.comm_stats, against their
restatement with Python ints (tests/comm_ref.py).  The columns are integers and the episode rows integer sums divided once: all
compared with ==; the means within episode_ref.mean_bound.

Shapes: every team-size class of the kernel (N = 1, 2, 3-4, 5-8 on 1 / 2 / 4 / 8 lanes per graph; N >= 9 on one wave per graph
with 1 .. 4 words per row, even N on the 16-byte walk and odd N on the one-float walk), the sizes next to each boundary, S = 37 (a
ragged last wave / workgroup in every class), S = 1, and an S just past a whole workgroup of each class."""
import numpy as np
import pytest

from tests import comm_ref as R, episode_ref as ER

pytestmark = pytest.mark.gpu

SENTINEL = -77
GUARD = 3                                                       # guard rows in front of and behind each output


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch


def _launch(torch, S, N, Lh, adj, chan, adj_stride=None, chan_stride=None):
    """One cm_comm_stats launch into a sentinel-filled table with guard rows -> the whole table on the host.  adj / chan: device
    tensors or None (NULL)."""
    from com_marl_amd import _lib as L
    out = torch.full((S + 2 * GUARD, R.COMM_COLS), SENTINEL, dtype=torch.int32, device="cuda")
    a_st = N * N if adj_stride is None else adj_stride
    c_st = Lh * N * N if chan_stride is None else chan_stride
    L.check(L.lib().cm_comm_stats(S, N, Lh, L.ptr(adj), a_st, L.ptr(chan), c_st, L.ptr(out[GUARD:]), L.current_stream()),
            "cm_comm_stats")
    return out.cpu().numpy()


def _check(torch, S, N, Lh, adj, chan, adj_stride=None, chan_stride=None, want=None, dev=None):
    """adj / chan: host arrays ([S,...], one block for stride 0, or None).  Launches twice: the same bits, guards untouched."""
    if want is None:
        want = R.comm_stats(adj, chan, N, Lh, S)
    d_adj, d_chan = dev if dev is not None else (None if adj is None else torch.from_numpy(adj).cuda(),
                                                 None if chan is None else torch.from_numpy(chan).cuda())
    got = _launch(torch, S, N, Lh, d_adj, d_chan, adj_stride, chan_stride)
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + S:] == SENTINEL).all(), "guard rows written"
    np.testing.assert_array_equal(got[GUARD:GUARD + S], want)
    again = _launch(torch, S, N, Lh, d_adj, d_chan, adj_stride, chan_stride)
    assert got.tobytes() == again.tobytes()
    return want


GRID = [(N, 2) for N in (1, 2, 3, 4, 5, 8, 16, 24, 33, 63, 64, 65, 72, 128, 129, 255)] + [(N, Lh) for N in (4, 65) for Lh in (1, 3, 8)]


@pytest.mark.parametrize("N,Lh", GRID, ids=[f"N{N}-L{Lh}" for N, Lh in GRID])
def test_seeded_graphs_equal_the_restatement(gpu, N, Lh):
    """Asymmetric adj and channels at densities 0, 0.1, 0.5 and 1 with entries 1, 0.5, -2, 0 and -0.0 and garbage diagonals."""
    adj, chan = R.seeded(37, N, Lh, seed=1000 * Lh + N)
    want = _check(gpu, 37, N, Lh, adj, chan)
    if N > 1:
        assert want[:, 0].min() == 0 and want[:, 0].max() == N * (N - 1)           # densities 0 and 1 are in
        assert (want[:, 1] < Lh * want[:, 0]).any() and (want[:, 2] < want[:, 3]).any()
    _check(gpu, 1, N, Lh, adj[5:6], chan[5:6], want=want[5:6])                      # S = 1


# graphs per workgroup: 256 / P lanes in the small classes, four waves otherwise
RAGGED = [(1, 259), (2, 130), (4, 70), (8, 35), (24, 6), (72, 5), (129, 6), (255, 5)]


@pytest.mark.parametrize("N,S", RAGGED, ids=[f"N{N}-S{S}" for N, S in RAGGED])
def test_a_last_workgroup_that_is_not_full(gpu, N, S):
    adj, chan = R.seeded(S, N, 2, seed=7 * N + S, densities=(0.1, 0.5))
    _check(gpu, S, N, 2, adj, chan)


@pytest.mark.parametrize("N", [3, 4, 8, 24, 72, 129])
def test_null_arrays_are_ones_and_stride_zero_shares_a_block(gpu, N):
    torch = gpu
    S, Lh = 9, 2
    adj, chan = R.seeded(S, N, Lh, seed=50 + N, densities=(0.1, 0.5, 1.0))
    ones_a, ones_c = np.ones((S, N, N), np.float32), np.ones((S, Lh, N, N), np.float32)
    np.testing.assert_array_equal(_check(torch, S, N, Lh, None, chan), R.comm_stats(ones_a, chan, N, Lh))
    np.testing.assert_array_equal(_check(torch, S, N, Lh, adj, None), R.comm_stats(adj, ones_c, N, Lh))
    both = _check(torch, S, N, Lh, None, None)
    assert (both == [N * (N - 1), Lh * N * (N - 1), N * (N - 1), N * (N - 1)]).all()
    # stride 0: every graph reads graph 1's block
    np.testing.assert_array_equal(_check(torch, S, N, Lh, adj[1], chan, adj_stride=0),
                                  R.comm_stats(np.stack([adj[1]] * S), chan, N, Lh))
    np.testing.assert_array_equal(_check(torch, S, N, Lh, adj, chan[1], chan_stride=0),
                                  R.comm_stats(adj, np.stack([chan[1]] * S), N, Lh))
    # the identity as the shared block - a constant FL channel: nothing is delivered
    eye = np.ascontiguousarray(np.broadcast_to(np.eye(N, dtype=np.float32), (Lh, N, N)))
    fl = _check(torch, S, N, Lh, adj, eye, chan_stride=0)
    assert (fl[:, 1] == 0).all() and (fl[:, 2] == 0).all() and (fl[:, 3] > 0).any()


@pytest.mark.parametrize("N", [4, 8, 24])
def test_strides_past_the_block_and_buffers_off_16_byte_alignment(gpu, N):
    """Blocks 3 floats apart at an address 4 bytes past a 16-byte boundary: N = 4 and 8 take the one-float loads."""
    torch = gpu
    S, Lh = 11, 2
    adj, chan = R.seeded(S, N, Lh, seed=80 + N, densities=(0.1, 0.5))
    want = R.comm_stats(adj, chan, N, Lh)

    def spread(x, block):
        flat = torch.full((1 + S * (block + 3),), 9.0, dtype=torch.float32, device="cuda")
        view = flat[1:].view(S, block + 3)
        view[:, :block] = torch.from_numpy(x.reshape(S, block)).cuda()
        assert view.data_ptr() % 16 == 4
        return view
    d_adj, d_chan = spread(adj, N * N), spread(chan, Lh * N * N)
    from com_marl_amd import _lib as L
    out = torch.full((S, R.COMM_COLS), SENTINEL, dtype=torch.int32, device="cuda")
    L.check(L.lib().cm_comm_stats(S, N, Lh, d_adj.data_ptr(), N * N + 3, d_chan.data_ptr(), Lh * N * N + 3, L.ptr(out),
                                  L.current_stream()), "cm_comm_stats")
    np.testing.assert_array_equal(out.cpu().numpy(), want)


def test_hop_order_and_path_graphs(gpu):
    first, second = R.hop_order_pair()
    for adj, chan, want in (first, second):
        _check(gpu, 1, 3, 2, adj[None], chan[None], want=np.array([want], np.int32))
    for N, Lh in ((2, 1), (5, 2), (8, 3), (9, 3), (33, 8), (70, 2), (130, 3)):
        adj, chan, want = R.path_graph(N, Lh)
        _check(gpu, 1, N, Lh, adj[None], chan[None], want=np.array([want], np.int32))
        _check(gpu, 1, N, Lh, adj[None], None, want=np.array([want], np.int32))


def test_no_graphs_write_nothing_and_refusals_set_the_error_text(gpu):
    torch = gpu
    from com_marl_amd import _lib as L
    lib = L.lib()
    adj, chan = R.seeded(4, 4, 2, seed=3)
    d_adj, d_chan = torch.from_numpy(adj).cuda(), torch.from_numpy(chan).cuda()
    assert (_launch(torch, 0, 4, 2, d_adj, d_chan) == SENTINEL).all()
    out = torch.full((4, 4), SENTINEL, dtype=torch.int32, device="cuda")
    st = L.current_stream()
    for args in ((4, 0, 2, 16, 32), (4, 256, 2, 16, 32), (4, 4, 0, 16, 32), (4, 4, 9, 16, 32), (4, 4, 2, 15, 32), (4, 4, 2, 16, 31),
                 (-1, 4, 2, 16, 32)):
        S, N, Lh, a_st, c_st = args
        assert lib.cm_comm_stats(S, N, Lh, L.ptr(d_adj), a_st, L.ptr(d_chan), c_st, L.ptr(out), st) == -1, args
        assert b"cm_comm_stats" in lib.cm_last_error(), args
    assert lib.cm_comm_stats(4, 4, 2, L.ptr(d_adj), 16, L.ptr(d_chan), 32, None, st) == -1 and b"cm_comm_stats" in lib.cm_last_error()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()


# ---- cm_episode_comm, cm_comm_means -------------------------------------------------------------------------------------------
def _groupings(B):
    out = [(1, 1, 2, 4)]
    for g in (3, 5, 13):
        if B % g == 0 and g < B:
            out.append((g, g - 1, 1, g + 2))
    if B > 1:
        out.append((B, B - 1, 3, B + 3))
    return out


@pytest.mark.parametrize("T,B,N,Lh", [(7, 1, 4, 2), (7, 3, 1, 1), (7, 65, 4, 2), (7, 130, 24, 3), (70, 9, 5, 8)])
def test_episode_rows_equal_the_restatement(gpu, T, B, N, Lh):
    """The seeded trajectories of episode_ref (episodes that end at step 0, in the middle, at T-1, never, twice); take < group_size
    and row0 > 0 throughout.  T = 70: an episode longer than one round of 64 lanes."""
    torch = gpu
    from com_marl_amd import _lib as L
    buf = ER.buffers(T, B, N, seed=11 * T + B, with_adj=False, shift=B)
    if B >= 4:
        assert set(buf["kinds"]) == set(ER.KINDS)
    rng = np.random.default_rng(T + B)
    stats = rng.integers(0, Lh * N * N + 1, (T + 1, B, R.COMM_COLS)).astype(np.int32)
    d_pl, d_st = torch.from_numpy(buf["path_len"]).cuda(), torch.from_numpy(stats).cuda()
    for g, take, row0, epg in _groupings(B):
        rows = B // g * epg
        want = np.full((rows, R.EPC_COLS), float(SENTINEL))
        R.episode_comm(buf["path_len"], stats, N, Lh, g, take, epg, row0, want)
        outs = []
        for _ in range(2):
            out = torch.full((rows + 2 * GUARD, R.EPC_COLS), float(SENTINEL), dtype=torch.float64, device="cuda")
            L.check(L.lib().cm_episode_comm(T, B, N, Lh, L.ptr(d_pl), L.ptr(d_st), g, take, epg, row0, L.ptr(out[GUARD:]),
                                            L.current_stream()), "cm_episode_comm")
            outs.append(out.cpu().numpy())
        assert outs[0].tobytes() == outs[1].tobytes()
        got = outs[0]
        assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + rows:] == SENTINEL).all(), "guard rows written"
        assert (want[:, 0] != SENTINEL).sum() == B // g * take
        np.testing.assert_array_equal(got[GUARD:GUARD + rows], want)          # named rows exact, the others keep the sentinel


@pytest.mark.parametrize("K,E", [(1, 1), (3, 5), (5, 64), (2, 65), (6, 130)])
def test_means_equal_the_restatement(gpu, K, E):
    torch = gpu
    from com_marl_amd import _lib as L
    rng = np.random.default_rng(K * 1000 + E)
    table = rng.integers(0, 1000, (K, E, R.EPC_COLS)) / rng.integers(1, 60, (K, E, 1))
    want = R.comm_means(table)
    dev = torch.from_numpy(table).cuda()
    outs = []
    for _ in range(2):
        out = torch.full((K + 2 * GUARD, R.EPC_COLS), float(SENTINEL), dtype=torch.float64, device="cuda")
        L.check(L.lib().cm_comm_means(K, E, L.ptr(dev), L.ptr(out[GUARD:]), L.current_stream()), "cm_comm_means")
        outs.append(out.cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes()
    got = outs[0]
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + K:] == SENTINEL).all(), "guard rows written"
    for k in range(K):
        for c in range(R.EPC_COLS):
            assert abs(got[GUARD + k, c] - want[k, c]) <= ER.mean_bound(table[k, :, c]), (k, c)


# ---- envs.comm_stats ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scen,map_,sen,N,M,B", [("pp", 10, 1, 4, 4, 40), ("co", 20, 2, 24, 0, 6)], ids=["pp4", "co24"])
def test_envs_comm_stats_on_a_stepped_batch(gpu, scen, map_, sen, N, M, B):
    torch = gpu
    from com_marl_amd import envs
    from tests import conditions_common as cc
    params = cc.base_params(scen, map_, sen, N, M, teRcom=3, tepl=0.3)
    env = cc.make_batch(scen, params, B, 0, "IID", max_steps=6)
    env.reset_all()
    for a in cc.random_actions(4, B, N, seed=2):
        env.step_device(a.contiguous())
    env.check_status()
    got = envs.comm_stats(env.dist_adj, env.channels, env.Lh)
    assert got.shape == (B, 4) and got.dtype == torch.int32 and got.is_cuda
    adj, chan = env.dist_adj.cpu().numpy(), env.channels.cpu().numpy()
    want = R.comm_stats(adj, chan, N, env.Lh)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert 0 < want[:, 0].sum() < B * N * (N - 1) and 0 < want[:, 1].sum() < env.Lh * want[:, 0].sum()
    # None = ones, and a leading shape of more than one axis
    np.testing.assert_array_equal(envs.comm_stats(env.dist_adj, None, env.Lh).cpu().numpy(), R.comm_stats(adj, None, N, env.Lh))
    two = envs.comm_stats(None, env.channels.view(B // 2, 2, env.Lh, N, N), env.Lh)
    assert two.shape == (B // 2, 2, 4)
    np.testing.assert_array_equal(two.cpu().numpy().reshape(B, 4), R.comm_stats(None, chan, N, env.Lh))
