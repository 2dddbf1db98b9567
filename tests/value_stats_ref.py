"""Not a test: cm_value_stats / cm_episode_value / cm_value_means / cm_value_curves / cm_value_curve_means (include/commarl.h) and
the VALUE_KEYS of evaluate.eval_summary(value_stats=True) restated in numpy float64 with plain loops over envs and steps: what the
tests of csrc/cm_value_stats.hip and of the evaluation compare against.  Also the seeded inputs those tests share.

For env b, n = the length of its first episode (tests/episode_ref.episode_length) and, in f64,
    G[n-1] = r[n-1],   G[t] = r[t] + gamma * G[t+1]                       (no bootstrap at a cut episode)
row (t, b), t < n, is [v, G[t], (v - G[t])^2, G[t]^2, v - mute, lossless - v] with v = float64(values[t, b]); rows with t >= n are
zeros; a counterfactual that is None is identical to values: an exact 0 column.  Episode rows, means and curves are the listening
statistics' with the divisor n (n_episodes for the curves) for all six columns.

Tolerance.  Both sides compute in f64 from the same inputs.  The recurrence takes at most T steps of two roundings of 2^-53
relative each, on partial sums bounded by S = sum_t |r_t| (gamma <= 1): |error of G[t]| <= 2 T 2^-53 S, about 4.4e-14 S at T = 200 -
and the two sides may differ in whether the product and the sum are fused.  Where the rewards cancel, |G| is far below S, so the
bound is absolute per env: atol = 1e-12 max(1, S, max|v|) for value, ret, msg_value and loss_value (the last two are one exact
conversion and one subtraction: half an ulp of at most 2 max|v|).  sq_err = (v - G)^2 and ret_sq = G^2 inherit 2 |v - G| and 2 |G|
times the error of G, at most 2 (max|v| + S) of it: atol = 1e-12 max(1, S, max|v|)^2.  RTOL = 1e-10 covers the summation orders of
the reductions (at most T and n_episodes terms of one sign scale) with room to spare.  Reduced rows (already divided by n) take the
largest atol among the envs that enter them."""
import math

import numpy as np

from tests.episode_ref import episode_length
from tests.listen_stats_ref import path_lens

VALUE_COLS, EPV_COLS = 6, 6
KEYS = ['value_mean', 'value_return', 'value_bias', 'value_rmse', 'value_ev', 'msg_value', 'loss_value']
SQUARED = [2, 3]
RTOL = 1e-10


def env_atol(rewards, values):
    """-> [B, 6]: the absolute tolerance of every column of an env's rows (see the module docstring)."""
    scale = np.maximum(1.0, np.maximum(np.abs(np.asarray(rewards, np.float64)).sum(0), np.abs(np.asarray(values, np.float64)).max(0)))
    out = np.repeat((1e-12 * scale)[:, None], VALUE_COLS, 1)
    out[:, SQUARED] = (1e-12 * scale * scale)[:, None]
    return out


def returns(r, n, gamma):
    """The first n rewards of one env -> G[0 .. n-1]."""
    G = np.zeros(n)
    for t in range(n - 1, -1, -1):
        G[t] = float(r[t]) if t == n - 1 else float(r[t]) + gamma * G[t + 1]
    return G


def value_stats(rewards, path_len, values, mute, lossless, gamma):
    """cm_value_stats on host arrays: rewards [T,B] f64, path_len [T,B] i32, values [T,B] f32; mute / lossless [T,B] f32 or None
    -> float64 [T, B, 6]."""
    T, B = rewards.shape
    out = np.zeros((T, B, VALUE_COLS))
    for b in range(B):
        n = episode_length(path_len[:, b])
        G = returns(rewards[:, b], n, float(gamma))
        for t in range(n):
            v = float(values[t, b])
            out[t, b] = [v, G[t], (v - G[t]) ** 2, G[t] ** 2, 0.0 if mute is None else v - float(mute[t, b]),
                         0.0 if lossless is None else float(lossless[t, b]) - v]
    return out


def episode_value(path_len, stats, group_size, take, episodes_per_group, row0, episodes):
    """cm_episode_value on host arrays (path_len [T,B], stats [T,B,6]): writes the named rows of `episodes`
    [B / group_size * episodes_per_group, 6] in place."""
    T, B = path_len.shape
    assert B % group_size == 0 and 0 <= take <= group_size and row0 >= 0 and row0 + take <= episodes_per_group
    for b in range(B):
        k, j = divmod(b, group_size)
        if j >= take:
            continue
        n = episode_length(path_len[:, b])
        total = np.zeros(VALUE_COLS)
        for t in range(n):
            total += stats[t, b]
        episodes[k * episodes_per_group + row0 + j] = total / float(n)
    return episodes


def value_means(episodes):
    """cm_value_means: [K,E,6] -> [K,6]."""
    ep = np.asarray(episodes, np.float64)
    out = np.zeros((ep.shape[0], EPV_COLS))
    for k in range(ep.shape[0]):
        for e in range(ep.shape[1]):
            out[k] += ep[k, e]
        out[k] /= float(ep.shape[1])
    return out


def value_curves(path_len, stats, group_size, take, accumulate, sums):
    """cm_value_curves on host arrays: the groups' blocks of `sums` [B / group_size, T, 6]; an episode that has ended adds nothing."""
    T, B = path_len.shape
    assert accumulate in (0, 1) and B % group_size == 0 and 0 <= take <= group_size
    if take == 0:
        return sums
    new = np.zeros((B // group_size, T, VALUE_COLS))
    for k in range(B // group_size):
        for j in range(take):
            b = k * group_size + j
            for t in range(episode_length(path_len[:, b])):
                new[k, t] += stats[t, b]
    sums[...] = sums + new if accumulate else new
    return sums


def value_curve_means(sums, n_episodes):
    """cm_value_curve_means: [cells,T,6] sums -> [cells,T,6] curves."""
    return np.asarray(sums, np.float64) / float(n_episodes)


def explained(sq_err, bias, ret, ret_sq):
    """1 - Var[G - v] / Var[G] from the moments, with the degenerate rule: eps = 1e-12 max(1, E[G^2]); Var[G] <= eps -> 1 if the
    residual variance is <= eps too, else 0."""
    resid, var = sq_err - bias * bias, ret_sq - ret * ret
    eps = 1e-12 * max(1.0, ret_sq)
    if var <= eps:
        return 1.0 if resid <= eps else 0.0
    return 1.0 - resid / var


def keys(row):
    """A row of six means (value, ret, sq_err, ret_sq, msg_value, loss_value) -> the VALUE_KEYS dict."""
    mean, ret, sq_err, ret_sq, msg, loss = (float(x) for x in row)
    bias = mean - ret
    return dict(value_mean=mean, value_return=ret, value_bias=bias, value_rmse=math.sqrt(sq_err), value_ev=explained(sq_err, bias, ret, ret_sq),
                msg_value=msg, loss_value=loss)


def curve_keys(curves, step_cnt):
    """curves [T, 6] (zero-padded means over the episodes) and step_cnt [T] (the share of episodes still running at step t) -> the
    VALUE_KEYS curves, each [T]: rmse and ev from the columns divided by step_cnt[t]; 0 and 1 where no episode runs."""
    T = curves.shape[0]
    out = {k: np.zeros(T) for k in KEYS}
    for t in range(T):
        mean, ret, sq_err, ret_sq, msg, loss = (float(x) for x in curves[t])
        out["value_mean"][t], out["value_return"][t], out["value_bias"][t] = mean, ret, mean - ret
        out["msg_value"][t], out["loss_value"][t] = msg, loss
        if step_cnt[t] > 0:
            s = float(step_cnt[t])
            out["value_rmse"][t] = math.sqrt(sq_err / s)
            out["value_ev"][t] = explained(sq_err / s, mean / s - ret / s, ret / s, ret_sq / s)
        else:
            out["value_rmse"][t], out["value_ev"][t] = 0.0, 1.0
    return out


# ---- seeded inputs ------------------------------------------------------------------------------------------------------------
def seeded(T, B, kind, seed):
    """rewards [T,B] f64, path_len [T,B] i32, values, mute, lossless [T,B] f32.  kind "none": no episode ends; "all0": every
    episode ends at step 0; "mixed": listen_stats_ref.path_lens' mix (a third never end, some end a second time later).  The
    rewards are of mixed sign and scale (every fourth env 1000 times larger, every fifth env nearly cancelling pairs), the values
    the f32 roundings of the undiscounted suffix sums plus noise - correlated with the returns but not equal - and the
    counterfactuals the values with a perturbation; env 1 (where there is one) has lossless == values."""
    rng = np.random.default_rng(seed)
    path_len = path_lens(T, B, seed + 1, kind)
    rewards = rng.standard_normal((T, B))
    rewards[:, ::4] *= 1000.0
    rewards[1::2, ::5] = -rewards[:-1:2, ::5][:rewards[1::2, ::5].shape[0]] * (1.0 + 1e-9)
    suffix = np.cumsum(rewards[::-1], 0)[::-1]
    values = (suffix + rng.standard_normal((T, B))).astype(np.float32)
    mute = (values + rng.standard_normal((T, B)).astype(np.float32)).astype(np.float32)
    lossless = (values + np.float32(0.01) * rng.standard_normal((T, B)).astype(np.float32)).astype(np.float32)
    if B > 1:
        lossless[:, 1] = values[:, 1]
    return rewards, path_len, values, mute, lossless
