"""cm_episode_stats / cm_episode_means (csrc/cm_episode.hip) through ctypes against their numpy restatement (tests/episode_ref.py)
on seeded crafted trajectory buffers: T in {1, 5, 33}, B in {1, 3, 65, 130} (a ragged last wave of four, more than one
workgroup), N in {1, 4, 5, 24, 72} and dist_adj = NULL (16-byte and 4-byte adjacency positions, slots smaller and larger than one
load instruction's 64 positions), both scenarios.  Every buffer set of four or more envs holds an env that ends at step 0, one
that ends at T-1, one that never ends and one that ends twice (T = 1 has a single step to end at); the sets of one and three
envs take the kinds in turn (`shift`).

Bounds (tests/episode_ref.py): integer-valued columns exact; sums within 2 n 2^-53 sum|x_t|; means within 2 E 2^-53 mean|x|;
the standard deviation within that bound scaled by range / std, plus E 2^-53 std for its own sum; min and max exact.
Rows that are not named - other envs' rows, rows below row0, guard rows around both outputs - keep their sentinel.
Every launch goes to the current stream (the one eval_summary launches on); no case takes a stream of its own."""
import numpy as np
import pytest

from tests import episode_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
GUARD = 3                                                       # guard rows in front of and behind each output


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch


def _groupings(B):
    """(group_size, take, row0, episodes_per_group): group_size 1 (take can only be 1), every shape with a proper divisor of B
    as group_size and take < group_size, and the whole batch as one group; row0 > 0 throughout."""
    out = [(1, 1, 2, 4)]
    for g in (3, 5, 13, 26):
        if B % g == 0 and g < B:
            out.append((g, g - 1, 1, g + 2))
    if B > 1:
        out.append((B, B - 1, 3, B + 3))
    return out


def _device(torch, buf):
    dev = {k: torch.from_numpy(buf[k]).cuda() for k in ("reward", "details", "success", "path_len")}
    dev["dist_adj"] = None if buf["dist_adj"] is None else torch.from_numpy(buf["dist_adj"]).cuda()
    return dev


def _stats(torch, dev, N, scenario, g, take, row0, epg):
    """One cm_episode_stats launch into a sentinel-filled table with guard rows -> the whole table on the host."""
    from com_marl_amd import _lib as L
    T, B = dev["reward"].shape
    rows = B // g * epg
    out = torch.full((rows + 2 * GUARD, R.EPI_COLS), SENTINEL, dtype=torch.float64, device="cuda")
    L.check(L.lib().cm_episode_stats(T, B, N, scenario, L.ptr(dev["reward"]), L.ptr(dev["details"]), L.ptr(dev["success"]),
                                     L.ptr(dev["path_len"]), L.ptr(dev["dist_adj"]), g, take, epg, row0, L.ptr(out[GUARD:]),
                                     L.current_stream()), "cm_episode_stats")
    return out.cpu().numpy()


CASES = [(T, B, N) for T in (1, 5, 33) for B in (1, 3, 65, 130) for N in (1, 4, 5, 24, 72, None)]


@pytest.mark.parametrize("T,B,N", CASES, ids=[f"T{T}-B{B}-N{N}" for T, B, N in CASES])
def test_stats_equal_the_restatement(gpu, T, B, N):
    torch = gpu
    i = CASES.index((T, B, N))
    scenario = (R.PP, R.CO)[(i + i // 6) % 2]                    # both scenarios for every T, B and N over the list
    n_agents = 3 if N is None else N
    buf = R.buffers(T, B, n_agents, seed=100 + i, with_adj=N is not None, shift=i)
    if B >= 4 and T >= 3:
        assert set(buf["kinds"]) == set(R.KINDS)
    dev = _device(torch, buf)
    for g, take, row0, epg in _groupings(B):
        rows = B // g * epg
        want = np.full((rows, R.EPI_COLS), SENTINEL)
        bound = np.zeros_like(want)
        R.episode_stats(buf["reward"], buf["details"], buf["success"], buf["path_len"], buf["dist_adj"], n_agents, scenario, g,
                        take, epg, row0, want, bound)
        got = _stats(torch, dev, n_agents, scenario, g, take, row0, epg)
        assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + rows:] == SENTINEL).all(), "guard rows written"
        got = got[GUARD:GUARD + rows]
        named = want[:, 3] != SENTINEL
        assert named.sum() == B // g * take
        assert (got[~named] == SENTINEL).all(), "a row that was not named was written"
        exact = bound == 0.0
        assert (got[exact] == want[exact]).all()
        assert (np.abs(got - want) <= bound).all(), np.abs(got - want)[named].max(0)
        # two launches on the same inputs: the same bits
        again = _stats(torch, dev, n_agents, scenario, g, take, row0, epg)[GUARD:GUARD + rows]
        assert got.tobytes() == again.tobytes()


def test_an_adjacency_buffer_off_16_byte_alignment_takes_the_4_byte_walk(gpu):
    """N = 4 at an address that is 4 bytes past a 16-byte boundary: the same answers, from the one-float positions."""
    torch = gpu
    T, B, N = 5, 7, 4
    buf = R.buffers(T, B, N, seed=9)
    dev = _device(torch, buf)
    flat = torch.zeros(dev["dist_adj"].numel() + 1, dtype=torch.float32, device="cuda")
    flat[1:].copy_(dev["dist_adj"].reshape(-1))
    moved = dict(dev, dist_adj=flat[1:].view(T + 1, B, N, N))
    assert moved["dist_adj"].data_ptr() % 16 == 4
    a = _stats(torch, dev, N, R.CO, B, B, 0, B)
    b = _stats(torch, moved, N, R.CO, B, B, 0, B)
    assert a.tobytes() == b.tobytes() and (a[GUARD:GUARD + B, 3] >= 1).all()


def test_take_zero_and_no_envs_write_nothing(gpu):
    torch = gpu
    dev = _device(torch, R.buffers(5, 6, 4, seed=1))
    got = _stats(torch, dev, 4, R.PP, 3, 0, 1, 4)
    assert (got == SENTINEL).all()


def test_a_corrupted_path_len_entry_changes_the_result(gpu):
    """Negative control: the comparison above can fail.  An end planted at step 2 of an env that never ends shortens its episode."""
    torch = gpu
    T, B, N = 33, 8, 4
    buf = R.buffers(T, B, N, seed=5)
    b = buf["kinds"].index("never ends")
    good = _stats(torch, _device(torch, buf), N, R.PP, B, B, 0, B)[GUARD:GUARD + B]
    want = np.zeros((B, R.EPI_COLS))
    R.episode_stats(buf["reward"], buf["details"], buf["success"], buf["path_len"], buf["dist_adj"], N, R.PP, B, B, B, 0, want)
    assert good[b, 3] == T and np.abs(good - want).max() < 1e-9
    buf["path_len"][2, b] = 3
    bad = _stats(torch, _device(torch, buf), N, R.PP, B, B, 0, B)[GUARD:GUARD + B]
    assert bad[b, 3] == 3 and bad[b, 1] != good[b, 1] and bad[b, 6] != good[b, 6]
    others = np.arange(B) != b
    assert bad[others].tobytes() == good[others].tobytes()


@pytest.mark.parametrize("K,E", [(1, 1), (3, 5), (5, 64), (2, 65), (6, 130)])
def test_means_equal_the_restatement(gpu, K, E):
    torch = gpu
    from com_marl_amd import _lib as L
    rng = np.random.default_rng(K * 1000 + E)
    table = rng.normal(0.0, 5.0, (K, E, R.EPI_COLS))
    table[:, :, 0] = rng.integers(0, 2, (K, E))
    table[:, :, 3] = rng.integers(1, 200, (K, E))
    if K > 1:
        table[1, :, 1] = table[1, 0, 1]                          # a group whose returns are all the same
    want = R.episode_means(table)
    dev = torch.from_numpy(table).cuda()
    outs = []
    for _ in range(2):                                           # two launches on the same inputs: the same bits
        out = torch.full((K + 2 * GUARD, R.SUM_COLS), SENTINEL, dtype=torch.float64, device="cuda")
        L.check(L.lib().cm_episode_means(K, E, L.ptr(dev), L.ptr(out[GUARD:]), L.current_stream()), "cm_episode_means")
        outs.append(out.cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes()
    got = outs[0]
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + K:] == SENTINEL).all(), "guard rows written"
    got = got[GUARD:GUARD + K]
    for k in range(K):
        for c in range(R.EPI_COLS):
            assert abs(got[k, c] - want[k, c]) <= R.mean_bound(table[k, :, c]), (k, c)
        assert abs(got[k, 9] - want[k, 9]) <= R.std_bound(table[k, :, 1]), k
        assert got[k, 10] == table[k, :, 1].min() and got[k, 11] == table[k, :, 1].max()
