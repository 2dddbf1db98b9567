"""Not a test: cm_attn_stats / cm_episode_attn / cm_attn_means / cm_attn_curves / cm_attn_curve_means (include/commarl.h) restated
in numpy float64 with plain loops over hops and rows: what the tests of csrc/cm_attn_stats.hip and of
evaluate.eval_summary(attn_stats=True) compare against.  Also the seeded inputs those tests share.

Tolerance.  Both sides compute in f64 from the same f32 inputs and the masked products are exact.  A column is a sum of at most
L N^2 <= 520 200 non-negative terms: two orders differ by about terms * 2^-53 relative, at most 6e-11.  The one cancellation is
ln W - S / W in column 5, exactly the entropy of one kept entry: a few ulp of |ln M| <= 103, about 2e-14 per row and hop.  So
rtol = 1e-10 and atol = 1e-12 N L per graph; episode rows, means and curves (already divided by N, or N L): rtol = 1e-10, atol = 1e-12."""
import numpy as np

from tests.episode_ref import episode_length

ATTN_COLS, EPA_COLS = 6, 6
COLS = ['self', 'entropy', 'range_mass', 'kept_mass', 'eff_self', 'eff_entropy']
KEYS = ['attn_' + name for name in COLS]
RTOL = 1e-10


def graph_atol(N, L):
    return 1e-12 * N * L


def graph_stats(attn, adj, chan, N, L):
    """One graph: attn [N,N] f32, adj [N,N] or None (ones), chan [L,N,N] or None (ones) -> the six sums."""
    M = np.asarray(attn, np.float32).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        MlnM = np.where(M != 0, M * np.log(np.where(M != 0, M, 1.0)), 0.0)
    a = np.ones((N, N), bool) if adj is None else np.asarray(adj) != 0
    out = [0.0] * ATTN_COLS
    for i in range(N):
        out[0] += M[i, i]
        out[1] += -MlnM[i].sum()
        out[2] += M[i][a[i]].sum()
    for l in range(L):
        K = a if chan is None else a & (np.asarray(chan[l]) != 0)
        for i in range(N):
            W = M[i][K[i]].sum()
            out[3] += W
            if W != 0:
                out[4] += (M[i, i] if K[i, i] else 0.0) / W
                out[5] += np.log(W) - MlnM[i][K[i]].sum() / W
    return out


def attn_stats(attn, adj, chan, N, L):
    """cm_attn_stats on host arrays: attn [S,N,N]; adj [S,N,N], a single [N,N] (stride 0) or None; chan [S,L,N,N], a single
    [L,N,N] or None.  -> float64 [S, 6]."""
    S = attn.shape[0]
    out = np.zeros((S, ATTN_COLS))
    for s in range(S):
        a = None if adj is None else (adj if adj.ndim == 2 else adj[s])
        c = None if chan is None else (chan if chan.ndim == 3 else chan[s])
        out[s] = graph_stats(attn[s], a, c, N, L)
    return out


def _divisors(n, N, L):
    return np.array([n * N] * 3 + [n * N * L] * 3, np.float64)


def episode_attn(path_len, stats, N, L, group_size, take, episodes_per_group, row0, episodes):
    """cm_episode_attn on host arrays (path_len [T,B], stats [T,B,6]): writes the named rows of `episodes`
    [B / group_size * episodes_per_group, 6] in place."""
    T, B = path_len.shape
    assert B % group_size == 0 and 0 <= take <= group_size and row0 >= 0 and row0 + take <= episodes_per_group
    for b in range(B):
        k, j = divmod(b, group_size)
        if j >= take:
            continue
        n = episode_length(path_len[:, b])
        episodes[k * episodes_per_group + row0 + j] = stats[:n, b].sum(0) / _divisors(n, N, L)
    return episodes


def attn_means(episodes):
    """cm_attn_means: [K,E,6] -> [K,6]."""
    return np.asarray(episodes, np.float64).mean(1)


def attn_curves(path_len, stats, group_size, take, accumulate, sums):
    """cm_attn_curves on host arrays (path_len [T,B], stats [T,B,6]): the groups' blocks of `sums` [B / group_size, T, 6]; an
    episode that has ended adds nothing."""
    T, B = path_len.shape
    assert accumulate in (0, 1) and B % group_size == 0 and 0 <= take <= group_size
    if take == 0:
        return sums
    new = np.zeros((B // group_size, T, ATTN_COLS))
    for k in range(B // group_size):
        for j in range(take):
            b = k * group_size + j
            n = episode_length(path_len[:, b])
            new[k, :n] += stats[:n, b]
    sums[...] = sums + new if accumulate else new
    return sums


def attn_curve_means(sums, n_episodes, N, L):
    """cm_attn_curve_means: [cells,T,6] sums -> [cells,T,6] curves."""
    return np.asarray(sums, np.float64) / _divisors(n_episodes, N, L)


# ---- seeded inputs ------------------------------------------------------------------------------------------------------------
def softmax_rows(logits):
    """f32 softmax over the last axis, as a forward would record it."""
    x = np.asarray(logits, np.float32)
    ex = np.exp(x - x.max(-1, keepdims=True), dtype=np.float32)
    return (ex / ex.sum(-1, keepdims=True, dtype=np.float32)).astype(np.float32)


def seeded(S, N, L, seed, density=0.5):
    """attn [S,N,N]: f32 softmax rows of seeded logits scaled by 8 (weights from 1e-30 to nearly 1; the seed leaves no exact 0),
    with, where the team allows it: a planted exact 0 (graph 0, row 0), one-hot rows on the diagonal (graph 1) and off it (graph 2, row 0);
    adj [S,N,N] and chan [S,L,N,N] 0 / 1 at `density`, with graph 3's row 0 out of everybody's range (an empty kept set, the
    diagonal cleared too) and graph 4's row 0 kept nowhere by hop 0."""
    rng = np.random.default_rng(seed)
    attn = softmax_rows(8.0 * rng.standard_normal((S, N, N)))
    adj = (rng.random((S, N, N)) < density).astype(np.float32)
    chan = (rng.random((S, L, N, N)) < density).astype(np.float32)
    if N >= 2:
        attn[0, 0, 0] += attn[0, 0, 1]                                   # the row still sums to 1 within f32 rounding
        attn[0, 0, 1] = 0.0
    if S > 1:
        attn[1] = np.eye(N, dtype=np.float32)
    if S > 2:
        attn[2, 0] = 0.0
        attn[2, 0, N - 1] = 1.0
    if S > 3:
        adj[3, 0] = 0.0
    if S > 4:
        chan[4, 0, 0] = 0.0
    return attn, adj, chan


def path_lens(T, B, seed, kind="mixed"):
    """path_len [T,B] int32.  kind "none": no episode ends; "all0": every episode ends at step 0; "mixed": seeded - a third of
    the envs never end, the others end at a random step (some of them a second time later)."""
    rng = np.random.default_rng(seed)
    pl = np.zeros((T, B), np.int32)
    if kind == "all0":
        pl[0] = 1
    elif kind == "mixed":
        for b in range(B):
            if b % 3 != 2:
                t = int(rng.integers(0, T))
                pl[t, b] = t + 1
                if b % 2 and t + 2 < T:
                    pl[int(rng.integers(t + 1, T)), b] = 1
    return pl
