"""Not a test: cm_episode_curves / cm_curve_means / cm_comm_curves / cm_comm_curve_means (include/commarl.h) restated with plain
sequential loops, on the length rule of tests/episode_ref.py: what the tests of csrc/cm_episode_curves.hip and of
evaluate.eval_summary(curves=True) compare against.  Also the reference rule itself (`padded_mean`: zero-pad every episode's
per-step list to T and average over the episodes, exp_runners/testing.py:307-324) and the bounds the tests assert.

Bounds.  Every column but the reward is a sum of integers held exactly and divided once by an exact product: both sides round
once, the results are EQUAL.  The reward entry of step t is an f64 sum over the E episodes that run at t: two orders differ by
less than E 2^-53 sum|x| - each sum's error is at most half of that, and far less unless every rounding falls the same way - and
the means by that / E (`reward_bound`)."""
import numpy as np

from tests.episode_ref import CO, COLS, EPI_COLS, PP, U, episode_length, seq_sum, sum_bound   # noqa: F401

COMM_COLS, EPC_COLS = 4, 4
EPC = ['range_degree', 'heard_degree', 'reach', 'range_reach']
# sums column -> details column (columns 0, 1, 3, 6 are success, reward, the running count and the adjacency sum)
DETAIL_OF = {2: 0, 4: 1, 5: 2, 7: 4, 8: 3}


def _selected(B, group_size, take):
    assert B % group_size == 0 and 0 <= take <= group_size
    return [(k, k * group_size + j) for k in range(B // group_size) for j in range(take)]


def episode_curves(reward, details, success, path_len, dist_adj, N, group_size, take, accumulate, sums, abs_reward=None):
    """cm_episode_curves on host arrays ([T,B], [T,B,6], [T+1,B,N,N] or None): the blocks of `sums` [B / group_size, T, 9] of the
    groups in place (take = 0: nothing), envs in ascending order; abs_reward [B / group_size, T] gains the sum of |reward|."""
    T, B = reward.shape
    assert accumulate in (0, 1)
    if take == 0:
        return sums
    new = [[[0] * EPI_COLS for _ in range(T)] for _ in range(B // group_size)]
    rew = [[[] for _ in range(T)] for _ in range(B // group_size)]
    for k, b in _selected(B, group_size, take):
        n = episode_length(path_len[:, b])
        for t in range(n):
            row = new[k][t]
            row[0] += int(success[t, b])
            rew[k][t].append(float(reward[t, b]))
            for col, d in DETAIL_OF.items():
                row[col] += int(details[t, b, d])
            row[3] += 1
            s = t + 1 if t < n - 1 else n - 1                               # n = 1: slot 0
            row[6] += N * N if dist_adj is None else int(np.asarray(dist_adj[s, b], np.float64).sum())
    for k in range(B // group_size):
        for t in range(T):
            row = [float(v) for v in new[k][t]]
            row[1] = seq_sum(rew[k][t])
            sums[k, t] = (sums[k, t] + row) if accumulate else row
            if abs_reward is not None:
                abs_reward[k, t] = (abs_reward[k, t] if accumulate else 0.0) + seq_sum(abs(x) for x in rew[k][t])
    return sums


def curve_means(sums, n_episodes, scenario, N):
    """cm_curve_means: [cells,T,9] sums -> [cells,T,9] curves."""
    nE, nNE = float(n_episodes), float(N * n_episodes)
    pp = scenario == PP
    div = [nE, nE, nE if pp else nNE, nE, nNE, nE if pp else nNE, nNE, nNE, nNE]
    out = np.asarray(sums, np.float64) / np.array(div)
    if pp:
        out[..., 8] = 0.0
    return out


def comm_curves(path_len, stats, group_size, take, accumulate, sums):
    """cm_comm_curves on host arrays (path_len [T,B], stats [T+1,B,4]): the groups' blocks of `sums` [B / group_size, T, 4]."""
    T, B = path_len.shape
    assert accumulate in (0, 1)
    if take == 0:
        return sums
    new = [[[0] * COMM_COLS for _ in range(T)] for _ in range(B // group_size)]
    for k, b in _selected(B, group_size, take):
        for t in range(episode_length(path_len[:, b])):
            for c in range(COMM_COLS):
                new[k][t][c] += int(stats[t, b, c])
    for k in range(B // group_size):
        for t in range(T):
            row = np.array([float(v) for v in new[k][t]])
            sums[k, t] = (sums[k, t] + row) if accumulate else row
    return sums


def comm_curve_means(sums, n_episodes, N, L):
    """cm_comm_curve_means: [cells,T,4] sums -> [cells,T,4] curves."""
    nNE = float(N * n_episodes)
    return np.asarray(sums, np.float64) / np.array([nNE, float(N * L * n_episodes), nNE, nNE])


def delivery(curves):
    """[T,4] comm curves -> eval_summary's per-step delivery."""
    return np.array([h / r if r != 0 else 1.0 for r, h in zip(curves[:, 0], curves[:, 1])])


def reward_bound(n_episodes, abs_reward):
    """|difference| of two means over n_episodes of the zero-padded reward at a step whose sums took different orders:
    n_episodes 2^-53 sum|x| on the sums, divided by n_episodes."""
    return U * np.asarray(abs_reward, np.float64)


def padded_mean(lists, T):
    """The reference's rule: per-step lists of E episodes -> zero-padded to T (pad_sequence(..., padding_value=0)), mean over the
    episodes per step.  -> (mean [T], mean of |x| [T])."""
    pad = np.zeros((len(lists), T))
    for e, xs in enumerate(lists):
        pad[e, :len(xs)] = xs
    return pad.mean(0), np.abs(pad).mean(0)
