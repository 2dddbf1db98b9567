"""Not a test: cm_comm_stats / cm_episode_comm / cm_comm_means (include/commarl.h) restated with plain loops over Python ints
(a row of a graph is one int, bit j = entry j is set): what the tests of csrc/cm_comm_stats.hip and of
evaluate.eval_summary(comm_stats=True) compare against.  Also the crafted and seeded graphs those tests share.

Every column of cm_comm_stats is an integer and every episode column an integer sum divided once by an exact integer, so both
are compared with ==.  The means of cm_comm_means are E-term f64 sums in another order: within episode_ref.mean_bound."""
import numpy as np

from tests.episode_ref import episode_length, seq_sum

COMM_COLS, EPC_COLS = 4, 4
COLS = ['in_range', 'delivered', 'reach', 'range_reach']
EPC = ['range_degree', 'heard_degree', 'reach', 'range_reach']


def _rows(block, N):
    """[N,N] (None: ones) -> N ints, bit j of int i = (entry [i][j] != 0); the diagonal cleared."""
    if block is None:
        return [((1 << N) - 1) & ~(1 << i) for i in range(N)]
    bits = np.packbits(np.asarray(block) != 0, axis=1, bitorder="little")
    return [int.from_bytes(bits[i].tobytes(), "little") & ~(1 << i) for i in range(N)]


def _reach(heard, N, L):
    """heard[l][i]: bit j set when i hears j != i at hop l -> #{(i,k), i != k : X_L[i][k]}, X_0 = I, hop 0 applied first."""
    full = (1 << N) - 1
    X = [1 << i for i in range(N)]
    for l in range(L):
        new = []
        for i in range(N):
            row, h = X[i], heard[l][i]
            while h and row != full:                              # (a full row gains nothing more)
                low = h & -h
                row |= X[low.bit_length() - 1]
                h ^= low
            new.append(row)
        X = new
    return sum(bin(X[i]).count("1") - 1 for i in range(N))


def graph_stats(adj, chan, N, L):
    """One graph: adj [N,N] or None (ones), chan [L,N,N] or None (ones) -> [in_range, delivered, reach, range_reach]."""
    a = _rows(adj, N)
    m = [[a[i] & c for i, c in enumerate(_rows(None if chan is None else chan[l], N))] for l in range(L)]
    in_range = sum(bin(r).count("1") for r in a)
    delivered = sum(bin(r).count("1") for hop in m for r in hop)
    return [in_range, delivered, _reach(m, N, L), _reach([a] * L, N, L)]


def comm_stats(adj, chan, N, L, S=None):
    """cm_comm_stats on host arrays: adj [S,N,N], a single [N,N] (stride 0) or None; chan [S,L,N,N], a single [L,N,N] or None.
    -> int32 [S, 4]."""
    if S is None:
        S = adj.shape[0] if adj is not None and adj.ndim == 3 else chan.shape[0]
    out = np.zeros((S, COMM_COLS), np.int32)
    for s in range(S):
        a = None if adj is None else (adj if adj.ndim == 2 else adj[s])
        c = None if chan is None else (chan if chan.ndim == 3 else chan[s])
        out[s] = graph_stats(a, c, N, L)
    return out


def episode_comm(path_len, stats, N, L, group_size, take, episodes_per_group, row0, episodes):
    """cm_episode_comm on host arrays (path_len [T,B], stats [T+1,B,4]): writes the named rows of `episodes`
    [B / group_size * episodes_per_group, 4] in place."""
    T, B = path_len.shape
    assert B % group_size == 0 and 0 <= take <= group_size and row0 >= 0 and row0 + take <= episodes_per_group
    for b in range(B):
        k, j = divmod(b, group_size)
        if j >= take:
            continue
        n = episode_length(path_len[:, b])
        c = [sum(int(stats[t, b, col]) for t in range(n)) for col in range(COMM_COLS)]
        episodes[k * episodes_per_group + row0 + j] = [c[0] / (n * N), c[1] / (n * N * L), c[2] / (n * N), c[3] / (n * N)]
    return episodes


def comm_means(episodes):
    """cm_comm_means: [K,E,4] -> [K,4]."""
    ep = np.asarray(episodes, np.float64)
    K, E, _ = ep.shape
    return np.array([[seq_sum(ep[k, :, c]) / E for c in range(EPC_COLS)] for k in range(K)])


def summary_keys(means):
    """One row of cm_comm_means -> the keys eval_summary(comm_stats=True) adds."""
    d = {name: float(means[i]) for i, name in enumerate(EPC)}
    d["delivery"] = d["heard_degree"] / d["range_degree"] if d["range_degree"] != 0 else 1.0
    return d


# ---- crafted graphs: (adj, chan, N, L, expected) ------------------------------------------------------------------------------
def path_graph(N, L):
    """0-1-...-(N-1), ones channels: agent i reaches min(i, L) + min(N-1-i, L) others."""
    adj = np.zeros((N, N), np.float32)
    for i in range(N - 1):
        adj[i, i + 1] = adj[i + 1, i] = 1.0
    reach = sum(min(i, L) + min(N - 1 - i, L) for i in range(N))
    return adj, np.ones((L, N, N), np.float32), [2 * (N - 1), 2 * (N - 1) * L, reach, reach]


def hop_order_pair():
    """N = 3, L = 2, adj all ones.  First: hop 0 delivers only 1 <- 2, hop 1 only 0 <- 1: agent 0 hears 1, which already holds 2.
    Second: the hops swapped - agent 0 hears 1 before 1 has heard 2."""
    adj = np.ones((3, 3), np.float32)
    c = np.zeros((2, 3, 3), np.float32)
    c[0, 1, 2] = 1.0
    c[1, 0, 1] = 1.0
    return (adj, c, [6, 2, 3, 6]), (adj, np.ascontiguousarray(c[::-1]), [6, 2, 2, 6])


# ---- seeded graphs ------------------------------------------------------------------------------------------------------------
VALUES = np.array([1.0, 0.5, -2.0], np.float32)        # all "set"; 0.0 and -0.0 are not


def seeded(S, N, L, seed, densities=(0.0, 0.1, 0.5, 1.0)):
    """Asymmetric adj [S,N,N] and chan [S,L,N,N]: graph s has density densities[s % len] for adj and densities[(s // len) % len]
    for chan; set entries are 1, 0.5 or -2, unset ones 0 or -0.0; the diagonals hold garbage (set or not, at random)."""
    rng = np.random.default_rng(seed)
    D = len(densities)
    da = np.array([densities[s % D] for s in range(S)]).reshape(S, 1, 1)
    dc = np.array([densities[(s // D) % D] for s in range(S)]).reshape(S, 1, 1, 1)

    def fill(shape, dens):
        on = rng.random(shape) < dens
        val = VALUES[rng.integers(0, len(VALUES), shape)]
        zero = np.where(rng.random(shape) < 0.5, np.float32(0.0), np.float32(-0.0))
        return np.where(on, val, zero).astype(np.float32)

    adj, chan = fill((S, N, N), da), fill((S, L, N, N), dc)
    eye = np.eye(N, dtype=bool)
    adj[:, eye] = fill((S, N), 0.5)
    chan[:, :, eye] = fill((S, L, N), 0.5)
    return adj, chan
