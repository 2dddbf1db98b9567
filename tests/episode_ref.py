"""numpy restatement of cm_episode_stats / cm_episode_means (include/commarl.h), with sequential f64 sums: what the tests of
csrc/cm_episode.hip and of evaluate.eval_summary compare against.  Also the seeded trajectory buffers those tests share, and the
error bounds they assert.

Bounds.  With u = 2^-53, an n-term f64 sum carries at most (n - 1) u sum|x_t| whatever its order, so two sums of the same terms in
different orders differ by less than 2 n u sum|x_t| (`sum_bound`); a column that is a sum divided once (or a sum of terms each
divided) stays inside the same bound.  A mean over E rows likewise: 2 E u mean|x| (`mean_bound`).  The population standard
deviation is sqrt(q / E), q = sum (x - m)^2: moving every x and m by at most delta moves q by at most 2 E range delta and std by
range delta / std (delta where the column is constant), and the sum q itself adds 2 E u q, i.e. E u std (`std_bound`)."""
import numpy as np

EPI_COLS, SUM_COLS = 9, 12
COLS = ['success', 'reward', 'capture_cnt', 'step_cnt', 'move_cnt', 'penalty_cnt', 'nodeDeg', 'variable', 'vars2']
PP, CO = 0, 1
U = 2.0 ** -53


def seq_sum(xs):
    acc = 0.0
    for x in xs:
        acc += float(x)
    return acc


def episode_length(path_len_b):
    """t + 1 for the first t with path_len[t] > 0, else T."""
    ends = np.nonzero(np.asarray(path_len_b) > 0)[0]
    return int(ends[0]) + 1 if len(ends) else len(path_len_b)


def episode_terms(reward_b, details_b, path_len_b, adj_b, N, scenario):
    """-> n, {column: its n per-step terms (f64)} for the summed / averaged columns."""
    n = episode_length(path_len_b)
    nA = float(N)
    det = np.asarray(details_b[:n], np.int64)
    ints = {c: [int(v) for v in det[:, c]] for c in range(5)}
    if adj_b is None:
        deg = [float(N)] * n
    else:
        slot = [float(np.asarray(adj_b[t], np.float64).sum()) / nA for t in range(n)]   # 0 / 1 entries: an exact integer / N
        deg = slot[1:n] + slot[n - 1:n]                                                 # deg[1], ..., deg[n-1], deg[n-1]; n = 1: deg[0]
    return n, dict(reward=[float(x) for x in reward_b[:n]], ints=ints, nodeDeg=deg)


def episode_row(reward_b, details_b, success_b, path_len_b, adj_b, N, scenario, with_abs=False):
    """One env's [T] trajectory (adj_b: [T+1,N,N] or None) -> its row of EPI_COLS doubles; with_abs also the row of sum|x_t| of
    every column's terms (0 for the integer-valued columns) and n."""
    n, tm = episode_terms(reward_b, details_b, path_len_b, adj_b, N, scenario)
    nA = float(N)
    s = {c: sum(tm["ints"][c]) for c in range(5)}                                       # integers, divided once
    pp = scenario == PP
    row = [float(success_b[n - 1]), seq_sum(tm["reward"]), float(s[0]) if pp else s[0] / nA, float(n), s[1] / nA,
           float(s[2]) if pp else s[2] / nA, seq_sum(tm["nodeDeg"]) / n, s[4] / nA, 0.0 if pp else s[3] / nA]
    if not with_abs:
        return row
    a = {c: sum(abs(v) for v in tm["ints"][c]) / nA for c in range(5)}
    absrow = [0.0, seq_sum(abs(x) for x in tm["reward"]), 0.0 if pp else a[0], 0.0, a[1], 0.0 if pp else a[2],
              seq_sum(tm["nodeDeg"]) / n, a[4], 0.0 if pp else a[3]]
    return row, absrow, n


def sum_bound(n, abs_sum):
    return 2.0 * n * U * abs_sum


def episode_stats(reward, details, success, path_len, dist_adj, N, scenario, group_size, take, episodes_per_group, row0, episodes,
                  bounds=None):
    """cm_episode_stats on host arrays ([T,B], [T,B,6], [T+1,B,N,N] or None): writes the named rows of `episodes`
    [B / group_size * episodes_per_group, EPI_COLS] in place, and of `bounds` (same shape) the assertable error of every entry."""
    T, B = reward.shape
    assert B % group_size == 0 and 0 <= take <= group_size and row0 >= 0 and row0 + take <= episodes_per_group
    for b in range(B):
        k, j = divmod(b, group_size)
        if j >= take:
            continue
        adj_b = None if dist_adj is None else dist_adj[:, b]
        row, absrow, n = episode_row(reward[:, b], details[:, b], success[:, b], path_len[:, b], adj_b, N, scenario, True)
        episodes[k * episodes_per_group + row0 + j] = row
        if bounds is not None:
            bounds[k * episodes_per_group + row0 + j] = [sum_bound(n, a) for a in absrow]
    return episodes


def episode_means(episodes):
    """cm_episode_means: [K,E,EPI_COLS] -> [K,SUM_COLS]."""
    ep = np.asarray(episodes, np.float64)
    K, E, _ = ep.shape
    out = np.zeros((K, SUM_COLS))
    for k in range(K):
        for c in range(EPI_COLS):
            out[k, c] = seq_sum(ep[k, :, c]) / E
        x, m = ep[k, :, 1], out[k, 1]
        out[k, 9] = np.sqrt(seq_sum((v - m) * (v - m) for v in x) / E)
        out[k, 10], out[k, 11] = x.min(), x.max()
    return out


def mean_bound(col, delta=0.0):
    """Two E-term means of `col` in different orders, the entries themselves known to `delta`."""
    col = np.asarray(col, np.float64)
    return 2.0 * len(col) * U * float(np.abs(col).mean()) + float(np.mean(delta))


def std_bound(col, delta=0.0):
    col = np.asarray(col, np.float64)
    d = 2.0 * len(col) * U * float(np.abs(col).mean()) + float(np.max(delta))
    rng, std = float(col.max() - col.min()), float(col.std())
    return d * max(1.0, rng / std if std > 0 else 1.0) + 2.0 * len(col) * U * std


# ---- seeded buffers ----------------------------------------------------------------------------------------------------------
KINDS = ("ends at step 0", "ends at T-1", "never ends", "ends twice")


def buffers(T, B, N, seed, with_adj=True, shift=0):
    """Trajectory buffers of T steps x B envs.  Env b is of kind KINDS[(b + shift) % 4] (a set of four or more envs holds every
    kind; T = 1 has one step to end at, T = 2 no room for two ends apart from 0 and 1); envs 8 and up of kind "ends twice" end
    at random steps instead.  -> dict(reward, details, success, path_len, dist_adj or None, kinds)."""
    rng = np.random.default_rng(seed)
    reward = rng.normal(0.0, 3.0, (T, B))
    details = rng.integers(0, 3 * N + 1, (T, B, 6)).astype(np.int32)
    success = rng.integers(0, 2, (T, B)).astype(np.int32)
    path_len = np.zeros((T, B), np.int32)
    kinds = []
    for b in range(B):
        kind = (b + shift) % 4
        kinds.append(KINDS[kind])
        if kind == 0:
            ends = [0]
        elif kind == 1:
            ends = [T - 1]
        elif kind == 2:
            ends = []
        elif b < 8 or T < 3:
            ends = sorted({min(1, T - 1), T - 1})
        else:
            ends = sorted(set(rng.integers(0, T, 2).tolist()))
        prev = -1
        for t in ends:
            path_len[t, b] = t - prev
            prev = t
    adj = None
    if with_adj:
        adj = (rng.random((T + 1, B, N, N)) < rng.random((T + 1, B, 1, 1))).astype(np.float32)
    return dict(reward=reward, details=details, success=success, path_len=path_len, dist_adj=adj, kinds=kinds)
