"""cm_episode_curves / cm_curve_means / cm_comm_curves / cm_comm_curve_means (csrc/cm_episode_curves.hip) through ctypes against
their numpy restatement (tests/curves_ref.py) on the seeded trajectory buffers of tests/episode_ref.py: T in {1, 5, 70} (70 crosses
a tile of steps and the 64 lanes), N in {2, 3, 4, 5} and dist_adj = NULL (16-byte and 4-byte adjacency positions, N = 3 with odd
strides), 70 envs as ten groups of 7 (take 5), seven groups of 10 (take 1) and one group of 70 with take 67 (the lanes loop over
the group's envs).  Every buffer set holds envs that end at step 0, at T-1, never and twice.  Each table is filled by TWO launches
on different buffers with different `take` - accumulate = 0, then 1 - and compared after each.

Asserts: the guard blocks around the tables keep their sentinel; every column but the reward is EQUAL to the restatement (both
sides hold the same exact integer and divide it once by the same exact product); the reward is within n_episodes 2^-53 sum|x| of
it (two f64 sums of the same terms in different orders), the mean within that / n_episodes; the same launches again write the
same bits.  Every launch goes to the current stream."""
import numpy as np
import pytest

from tests import comm_ref, curves_ref as V, episode_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
GUARD = 2                                                       # guard blocks of [T, cols] in front of and behind each table
B = 70
GROUPINGS = [(7, 5, 7), (10, 1, 10), (70, 67, 3)]               # (group_size, take of the first round, take of the second)


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch


def _device(torch, buf):
    dev = {k: torch.from_numpy(buf[k]).cuda() for k in ("reward", "details", "success", "path_len")}
    dev["dist_adj"] = None if buf["dist_adj"] is None else torch.from_numpy(buf["dist_adj"]).cuda()
    return dev


def _table(torch, groups, T, cols):
    return torch.full((groups + 2 * GUARD, T, cols), SENTINEL, dtype=torch.float64, device="cuda")


def _curves(dev, N, scenario, g, take, acc, table):
    from com_marl_amd import _lib as L
    T, n_envs = dev["reward"].shape
    L.check(L.lib().cm_episode_curves(T, n_envs, N, scenario, L.ptr(dev["reward"]), L.ptr(dev["details"]), L.ptr(dev["success"]),
                                      L.ptr(dev["path_len"]), L.ptr(dev["dist_adj"]), g, take, acc, L.ptr(table[GUARD:]),
                                      L.current_stream()), "cm_episode_curves")
    return table.cpu().numpy()


def _guards_kept(host, groups):
    return (host[:GUARD] == SENTINEL).all() and (host[GUARD + groups:] == SENTINEL).all()


def _compare_sums(got, want, abs_reward, n_episodes):
    ints = [c for c in range(R.EPI_COLS) if c != 1]
    assert (got[..., ints] == want[..., ints]).all(), np.abs(got - want).max((0, 1))
    err, bound = np.abs(got[..., 1] - want[..., 1]), n_episodes * R.U * abs_reward
    assert (err <= bound).all(), (err.max(), bound[err > bound])


CASES = [(T, N) for T in (1, 5, 70) for N in (2, 3, 4, 5, None)]


@pytest.mark.parametrize("T,N", CASES, ids=[f"T{T}-N{N}" for T, N in CASES])
def test_curves_equal_the_restatement_over_two_rounds(gpu, T, N):
    torch = gpu
    from com_marl_amd import _lib as L
    i = CASES.index((T, N))
    scenario = (R.PP, R.CO)[i % 2]
    n_agents = 3 if N is None else N
    bufs = [R.buffers(T, B, n_agents, seed=300 + 2 * i + r, with_adj=N is not None, shift=i + r) for r in range(2)]
    if T >= 3:
        assert set(bufs[0]["kinds"]) == set(R.KINDS)
    devs = [_device(torch, b) for b in bufs]
    for g, take1, take2 in GROUPINGS:
        groups = B // g
        want, abs_rew = np.full((groups, T, R.EPI_COLS), SENTINEL), np.zeros((groups, T))
        runs = []
        for _ in range(2):                                      # the same two launches twice: the same bits
            table = _table(torch, groups, T, R.EPI_COLS)
            hosts = [_curves(devs[r], n_agents, scenario, g, take, r, table) for r, take in enumerate((take1, take2))]
            means = _table(torch, groups, T, R.EPI_COLS)
            n_epi = take1 + take2
            L.check(L.lib().cm_curve_means(groups, T, n_epi, scenario, n_agents, L.ptr(table[GUARD:]), L.ptr(means[GUARD:]),
                                           L.current_stream()), "cm_curve_means")
            runs.append(hosts + [means.cpu().numpy()])
        for a, b in zip(*runs):
            assert a.tobytes() == b.tobytes()
        first, second, means = runs[0]
        for r, (host, take) in enumerate(((first, take1), (second, take2))):
            buf = bufs[r]
            V.episode_curves(buf["reward"], buf["details"], buf["success"], buf["path_len"], buf["dist_adj"], n_agents, g, take, r,
                             want, abs_rew)
            assert _guards_kept(host, groups), "guard blocks written"
            _compare_sums(host[GUARD:GUARD + groups], want, abs_rew, take1 + (take2 if r else 0))
        assert (want[:, 0, 3] == n_epi).all() and (want[..., 3] >= 0).all()
        assert _guards_kept(means, groups), "guard blocks written"
        got, ref = means[GUARD:GUARD + groups], V.curve_means(want, n_epi, scenario, n_agents)
        # the device divided ITS sums: equal to the restatement's division of the same sums, the reward within its bound
        assert (got == V.curve_means(second[GUARD:GUARD + groups], n_epi, scenario, n_agents)).all()
        ints = [c for c in range(R.EPI_COLS) if c != 1]
        assert (got[..., ints] == ref[..., ints]).all()
        assert (np.abs(got[..., 1] - ref[..., 1]) <= V.reward_bound(n_epi, abs_rew)).all()
        assert (got[:, 0, 3] == 1.0).all() and (np.diff(got[..., 3], axis=1) <= 0).all()
        if scenario == R.PP:
            assert (got[..., 8] == 0.0).all()


def test_an_adjacency_buffer_off_16_byte_alignment_takes_the_4_byte_walk(gpu):
    """N = 4 at an address that is 4 bytes past a 16-byte boundary: the same bits, from the one-float positions."""
    torch = gpu
    T, N = 5, 4
    dev = _device(torch, R.buffers(T, B, N, seed=9))
    flat = torch.zeros(dev["dist_adj"].numel() + 1, dtype=torch.float32, device="cuda")
    flat[1:].copy_(dev["dist_adj"].reshape(-1))
    moved = dict(dev, dist_adj=flat[1:].view(T + 1, B, N, N))
    assert moved["dist_adj"].data_ptr() % 16 == 4
    a = _curves(dev, N, R.CO, 7, 6, 0, _table(torch, 10, T, R.EPI_COLS))
    b = _curves(moved, N, R.CO, 7, 6, 0, _table(torch, 10, T, R.EPI_COLS))
    assert a.tobytes() == b.tobytes() and (a[GUARD:GUARD + 10, 0, 3] == 6).all() and (a[GUARD:GUARD + 10, 0, 6] > 0).all()


def test_take_zero_and_no_envs_write_nothing(gpu):
    torch = gpu
    from com_marl_amd import _lib as L
    dev = _device(torch, R.buffers(5, B, 4, seed=1))
    assert (_curves(dev, 4, R.PP, 7, 0, 0, _table(torch, 10, 5, R.EPI_COLS)) == SENTINEL).all()
    table = _table(torch, 10, 5, V.COMM_COLS)
    stats = torch.zeros(6, B, V.COMM_COLS, dtype=torch.int32, device="cuda")
    L.check(L.lib().cm_comm_curves(5, B, 4, 2, L.ptr(dev["path_len"]), L.ptr(stats), 7, 0, 1, L.ptr(table[GUARD:]),
                                   L.current_stream()), "cm_comm_curves")
    assert (table.cpu().numpy() == SENTINEL).all()


def test_a_corrupted_path_len_entry_changes_the_result(gpu):
    """Negative control: the comparison above can fail.  An end planted at step 2 of an env that never ends empties its later steps."""
    torch = gpu
    T, N = 8, 4
    buf = R.buffers(T, B, N, seed=5)
    b = buf["kinds"].index("never ends")
    good = _curves(_device(torch, buf), N, R.PP, B, B, 0, _table(torch, 1, T, R.EPI_COLS))[GUARD]
    buf["path_len"][2, b] = 3
    bad = _curves(_device(torch, buf), N, R.PP, B, B, 0, _table(torch, 1, T, R.EPI_COLS))[GUARD]
    assert (bad[:3, 3] == good[:3, 3]).all() and (bad[3:, 3] == good[3:, 3] - 1).all()
    assert bad[:2].tobytes() == good[:2].tobytes() and (bad[3:, 1] != good[3:, 1]).all()


@pytest.mark.parametrize("T,N,Lh", [(1, 2, 1), (5, 3, 2), (70, 4, 2), (5, 5, 3)])
def test_comm_curves_equal_the_restatement_over_two_rounds(gpu, T, N, Lh):
    """The rows are cm_comm_stats's restatement (tests/comm_ref.py) of seeded graphs; every column an integer: equality."""
    torch = gpu
    from com_marl_amd import _lib as L
    rounds = []
    for r in range(2):
        adj, chan = comm_ref.seeded((T + 1) * B, N, Lh, seed=40 + 2 * T + r)
        stats = comm_ref.comm_stats(adj, chan, N, Lh).reshape(T + 1, B, V.COMM_COLS)
        path_len = R.buffers(T, B, N, seed=50 + T + r, with_adj=False, shift=r)["path_len"]
        rounds.append((path_len, stats, torch.from_numpy(path_len).cuda(), torch.from_numpy(stats).cuda()))
    assert rounds[0][1].max() > 0
    for g, take1, take2 in GROUPINGS:
        groups, n_epi = B // g, take1 + take2
        want = np.full((groups, T, V.COMM_COLS), SENTINEL)
        runs = []
        for _ in range(2):
            table, hosts = _table(torch, groups, T, V.COMM_COLS), []
            for r, take in enumerate((take1, take2)):
                L.check(L.lib().cm_comm_curves(T, B, N, Lh, L.ptr(rounds[r][2]), L.ptr(rounds[r][3]), g, take, r, L.ptr(table[GUARD:]),
                                               L.current_stream()), "cm_comm_curves")
                hosts.append(table.cpu().numpy())
            means = _table(torch, groups, T, V.EPC_COLS)
            L.check(L.lib().cm_comm_curve_means(groups, T, n_epi, N, Lh, L.ptr(table[GUARD:]), L.ptr(means[GUARD:]),
                                                L.current_stream()), "cm_comm_curve_means")
            runs.append(hosts + [means.cpu().numpy()])
        for a, b in zip(*runs):
            assert a.tobytes() == b.tobytes()
        for r, take in enumerate((take1, take2)):
            V.comm_curves(rounds[r][0], rounds[r][1], g, take, r, want)
            assert _guards_kept(runs[0][r], groups), "guard blocks written"
            assert (runs[0][r][GUARD:GUARD + groups] == want).all()
        means = runs[0][2]
        assert _guards_kept(means, groups), "guard blocks written"
        assert (means[GUARD:GUARD + groups] == V.comm_curve_means(want, n_epi, N, Lh)).all()
