"""Not a test: cm_listen_stats / cm_episode_listen / cm_listen_means / cm_listen_curves / cm_listen_curve_means (include/commarl.h)
restated in numpy float64 with plain loops over graphs, agents and actions: what the tests of csrc/cm_listen_stats.hip and of
evaluate.eval_summary(listen_stats=True) compare against.  Also the seeded inputs those tests share.

For one agent row, p the probabilities the policy acted on and q the counterfactual ones (f32, length A), in f64 on the f32 values:
    kl   = sum over a with p[a] > 0 of p[a] * (ln p[a] - ln max(q[a], FLT_MIN))        FLT_MIN = 2^-126; not clamped at 0
    tv   = 0.5 * sum_a |p[a] - q[a]|
    flip = argmax(p) != argmax(q), the first index on ties, compared on the f32 values
A graph row is [mute_kl, mute_tv, mute_flip, loss_kl, loss_tv, loss_flip], each the sum over the N agents in agent order; a
counterfactual that is None is identical to p: exact zeros.  Episode rows, means and curves are the attention statistics' with the
divisor n N (N * n_episodes for the curves) for all six columns.

Tolerance.  Both sides compute in f64 from the same f32 inputs.  A column is a sum of at most N A <= 2040 terms, each at most
|ln FLT_MIN| = 87.4 in magnitude: two orders of summation and two f64 logarithms (a few ulp each) differ by far less than
rtol = 1e-10 of the sum's magnitude, and where the terms cancel (kl of nearly equal rows) by a few ulp of the largest term per
agent: atol = 1e-12 N per graph.  Episode rows, means and curves (already divided by N): rtol = 1e-10, atol = 1e-12.  The flip
columns are sums of 0 / 1 and are compared exactly on graph rows."""
import numpy as np

from tests.episode_ref import episode_length

LISTEN_COLS, EPL_COLS = 6, 6
KEYS = ['listen_kl', 'listen_tv', 'listen_flip', 'loss_kl', 'loss_tv', 'loss_flip']
FLIP_COLS = [2, 5]
RTOL = 1e-10
FLT_MIN = 2.0 ** -126


def graph_atol(N):
    return 1e-12 * N


def row_terms(p, q):
    """One agent row: p, q f32 [A] -> (kl, tv, flip)."""
    p, q = np.asarray(p, np.float32), np.asarray(q, np.float32)
    assert p.shape == q.shape and p.ndim == 1
    kl = tv = 0.0
    for a in range(p.shape[0]):
        pa, qa = float(p[a]), float(q[a])
        if p[a] > 0:
            kl += pa * (np.log(pa) - np.log(max(qa, FLT_MIN)))
        tv += abs(pa - qa)
    return kl, 0.5 * tv, float(int(np.argmax(p)) != int(np.argmax(q)))       # (np.argmax: the first index on ties)


def graph_row(p, mute, lossless):
    """One graph: p [N,A] f32; mute / lossless [N,A] or None -> the six sums."""
    out = [0.0] * LISTEN_COLS
    for c0, q in ((0, mute), (3, lossless)):
        if q is None:
            continue
        for i in range(p.shape[0]):
            for c, v in enumerate(row_terms(p[i], q[i])):
                out[c0 + c] += v
    return out


def listen_stats(probs, mute, lossless):
    """cm_listen_stats on host arrays: probs [S,N,A]; mute / lossless [S,N,A] or None -> float64 [S, 6]."""
    S = probs.shape[0]
    out = np.zeros((S, LISTEN_COLS))
    for s in range(S):
        out[s] = graph_row(probs[s], None if mute is None else mute[s], None if lossless is None else lossless[s])
    return out


def episode_listen(path_len, stats, N, group_size, take, episodes_per_group, row0, episodes):
    """cm_episode_listen on host arrays (path_len [T,B], stats [T,B,6]): writes the named rows of `episodes`
    [B / group_size * episodes_per_group, 6] in place."""
    T, B = path_len.shape
    assert B % group_size == 0 and 0 <= take <= group_size and row0 >= 0 and row0 + take <= episodes_per_group
    for b in range(B):
        k, j = divmod(b, group_size)
        if j >= take:
            continue
        n = episode_length(path_len[:, b])
        total = np.zeros(LISTEN_COLS)
        for t in range(n):
            total += stats[t, b]
        episodes[k * episodes_per_group + row0 + j] = total / float(n * N)
    return episodes


def listen_means(episodes):
    """cm_listen_means: [K,E,6] -> [K,6]."""
    ep = np.asarray(episodes, np.float64)
    out = np.zeros((ep.shape[0], EPL_COLS))
    for k in range(ep.shape[0]):
        for e in range(ep.shape[1]):
            out[k] += ep[k, e]
        out[k] /= float(ep.shape[1])
    return out


def listen_curves(path_len, stats, group_size, take, accumulate, sums):
    """cm_listen_curves on host arrays (path_len [T,B], stats [T,B,6]): the groups' blocks of `sums` [B / group_size, T, 6]; an
    episode that has ended adds nothing."""
    T, B = path_len.shape
    assert accumulate in (0, 1) and B % group_size == 0 and 0 <= take <= group_size
    if take == 0:
        return sums
    new = np.zeros((B // group_size, T, LISTEN_COLS))
    for k in range(B // group_size):
        for j in range(take):
            b = k * group_size + j
            for t in range(episode_length(path_len[:, b])):
                new[k, t] += stats[t, b]
    sums[...] = sums + new if accumulate else new
    return sums


def listen_curve_means(sums, n_episodes, N):
    """cm_listen_curve_means: [cells,T,6] sums -> [cells,T,6] curves."""
    return np.asarray(sums, np.float64) / float(n_episodes * N)


# ---- seeded inputs ------------------------------------------------------------------------------------------------------------
def softmax_rows(logits):
    """f32 softmax over the last axis, as a forward would record it."""
    x = np.asarray(logits, np.float32)
    ex = np.exp(x - x.max(-1, keepdims=True), dtype=np.float32)
    return (ex / ex.sum(-1, keepdims=True, dtype=np.float32)).astype(np.float32)


def seeded(S, N, A, seed):
    """probs, mute, lossless [S,N,A]: f32 softmax rows of seeded logits scaled by 6 (probabilities from about 1e-16 to nearly 1; no
    exact 0 from the seed).  mute is drawn on its own; lossless is probs with a small perturbation of the logits (rows that nearly
    cancel in kl).  Planted, where S allows it, in agent row 0 - and in the last agent row too:
      graph 0  an exact 0 in mute under a positive p (the FLT_MIN term), the mass moved to the next action;
      graph 1  one-hot rows: p on action 0, mute on action A - 1, lossless = p;
      graph 2  an argmax tie in p (two equal largest values; the first index counts) and one in mute;
      graph 3  mute == p and lossless == p, for every agent (exact zeros)."""
    rng = np.random.default_rng(seed)
    logits = 6.0 * rng.standard_normal((S, N, A))
    probs = softmax_rows(logits)
    mute = softmax_rows(6.0 * rng.standard_normal((S, N, A)))
    lossless = softmax_rows(logits + 0.05 * rng.standard_normal((S, N, A)))
    rows = sorted({0, N - 1})
    for i in rows:
        a = int(np.argmax(probs[0, i]))
        mute[0, i, (a + 1) % A] += mute[0, i, a]
        mute[0, i, a] = 0.0
        if S > 1:
            probs[1, i] = 0.0
            probs[1, i, 0] = 1.0
            mute[1, i] = 0.0
            mute[1, i, A - 1] = 1.0
            lossless[1, i] = probs[1, i]
        if S > 2:
            top = np.float32(0.4)
            probs[2, i] = np.float32(0.2) / np.float32(max(A - 2, 1))
            probs[2, i, A - 2:] = top                              # the tie: argmax is A - 2
            if A == 2:
                probs[2, i] = np.float32(0.5)
            mute[2, i] = probs[2, i][::-1]                         # tie at indices 0, 1: argmax is 0
    if S > 3:
        mute[3] = probs[3]
        lossless[3] = probs[3]
    return probs, mute, lossless


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
