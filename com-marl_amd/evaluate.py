"""Greedy evaluation: ``eval_model`` with the reference's signature and return contract
(exp_runners/predatorprey/eval_pp.py:9-104; the coverage twin is the same loop), run as ONE batched
device rollout instead of a Python loop over episodes.

The reference plays ``n_eval_episodes`` episodes one after the other on one env; here the B envs of
the wrapper each play their *first* episode after a reset, all at once (policy forward with
``greedy=True`` + env step kernel, captured in the same RolloutEngine the sampler uses), and as many
such rounds are played as it takes to collect ``n_eval_episodes``.  Per episode the function returns
exactly what the reference returns: the per-step ``success`` list, the per-step ``VECTORS`` lists, the
per-episode sums (mean for ``nodeDeg``) and ``env.bound_return``.

Differences a maintainer should know (documented, not silent):
  * episodes are independent Philox streams (global env id, round) rather than one sequential
    generator re-seeded by ``fix_randomness(seed)``; ``seed`` re-keys nothing here - the wrapper's own
    ``seed=`` decides the streams;
  * ``render`` / ``inspect_steps`` are not supported (UI is out of scope) and raise;
  * with a range-limited adjacency, ``nodeDeg`` of an episode's terminal step is the degree *before*
    that step (the env auto-resets on done, vec_env_executor.py:36-43, so the post-step graph of a
    finished episode is never materialised).

``eval_summary`` plays the same rounds and returns only each policy's score (the CSV row of exp_runners/testing.py:329-335),
reduced on the device by cm_episode_stats / cm_episode_means: nothing but K x 12 doubles is copied to the host.
``eval_sweep`` does the same for K policies x C comm conditions in one rollout, on a wrapper built with ``conditions=``.
Both take five switches.  Each adds its keys to every dict, its doubles ride in the same single copy, and one that is off
launches, allocates and returns nothing:
  ``curves=True``        the same episodes reduced over the episodes with the STEP axis kept - per step the mean over the episodes
                         of the zero-padded lists eval_model returns, i.e. what exp_runners/testing.py:307-324 saves as rewMat3;
  ``comm_stats=True``    COMM_KEYS: how much of the offered communication was delivered and how much of the team an agent can hear
                         through the net's hops (cm_comm_stats on the engine's dist_adj / channels);
  ``attn_stats=True``    ATTN_KEYS: what the policy did with what was delivered - the self weight and the entropy of its attention
                         rows, the attention mass on links in range and on links that carried something, and the same two of the
                         weights the net really uses after masking and renormalising (cm_attn_stats on the engine's recorded attn);
  ``listen_stats=True``  LISTEN_KEYS: whether the messages changed what the agents did - the round replayed forward-only under a
                         mute and a lossless channel (RolloutEngine.replay_probs), compared with the recorded probabilities
                         (cm_listen_stats);
  ``value_stats=True, baselines=...``  VALUE_KEYS: how good the critic trained with each policy is - its values on the round's slots
                         (RolloutEngine.replay_values) against the discounted returns the episodes went on to collect, and what it
                         believes the messages and the channel loss are worth (cm_value_stats).
The four statistics families are one _Side each, told apart by a _Family description (FAMILIES); _layout describes the one buffer.
``ci=level`` adds bootstrap intervals and standard errors of every mean above, resampled over the episodes on the device tables
(cm_boot_means / cm_boot_quantiles; one index stream for every cell, column and table), and eval_sweep's ``contrast=`` the paired
difference of every cell against a reference condition or policy; off (the default) they launch, allocate and return nothing.
"""
import collections
import itertools
import math

import numpy as np
import torch

from . import _lib as L
from . import envs as _envs
from .nets import PolicySet
from .rollout import RolloutEngine

VECTORS = ['reward', 'capture_cnt', 'step_cnt', 'move_cnt', 'penalty_cnt', 'nodeDeg', 'variable', 'vars2']   # testing.py:209


def _play_round(eng, batch, T, greedy, chunk):
    """One round: reset + T steps, every env's first episode on the engine's trajectory buffers.  chunk: the T steps as chunk
    launches where the engine has them (one launch for every member of a PolicySet on the wave-owned kernel); bit-identical to
    stepping them one by one."""
    eng.reset()
    eng.play(0, T, greedy=greedy, chunk=chunk)
    eng.bump(T)
    batch.check_status()


def _first_episodes(eng, base, T, greedy, chunk=False):
    """_play_round; returns host arrays for every env's first episode."""
    _play_round(eng, base.batch, T, greedy, chunk)
    pl = eng.path_len[:T]                                                 # [T,B]
    ended = pl > 0
    # first t at which each env finished (T-1 when the loop limit cut it, eval_pp.py:73)
    first = torch.where(ended.any(0), ended.to(torch.int32).argmax(0), torch.full_like(pl[0], T - 1)).long()
    h = dict(first=first.cpu().numpy(), reward=eng.reward64[:T].cpu().numpy(), details=eng.details[:T].cpu().numpy(),
             success=eng.success[:T].cpu().numpy(), done=eng.done[:T].cpu().numpy())
    if eng.dist_adj is not None:
        h["deg"] = eng.dist_adj[:T + 1].sum(-1).mean(-1).cpu().numpy()   # [T+1,B] ave_deg (env_communication.py:232)
    return h


def eval_model(env, policy, itr, n_eval_episodes=100, max_env_steps=200, eval_greedy=True, render=False,
               inspect_steps=False, seed=1, flag=None):
    """eval_pp.py:9.  -> (episode_data, epi_success, epi_rewards, bound_return)."""
    if render or inspect_steps:
        raise NotImplementedError("rendering is outside the MI355X path")
    if flag is not None and flag[0]:
        return None, None, None, None
    base = getattr(env, "env", env)
    batch = base.batch
    B, N = batch.B, batch.N
    pp = batch.scenario == "pp"
    T = int(max_env_steps)
    if T > batch.cfg.max_path_length:
        raise ValueError(f"max_env_steps={T} exceeds the env's max_path_length={batch.cfg.max_path_length}")
    env.eval_n_epi = 0
    policy.sync_weights()
    policy.reset([True] * B)
    eng = RolloutEngine(batch, policy, T, store_attn=False, store_probs=False)
    episode_data, epi_success = [], []
    epi_rewards = {vec: [] for vec in VECTORS}
    eval_rewards = []
    while len(episode_data) < n_eval_episodes:
        h = _first_episodes(eng, base, T, bool(eval_greedy))               # (a single policy steps one by one)
        for b in range(min(B, n_eval_episodes - len(episode_data))):
            _append_episode(h, b, N, pp, episode_data, epi_success, epi_rewards, eval_rewards)
    env.eval_n_epi = len(episode_data)
    env.last_eval_average_reward = (sum(eval_rewards) / len(eval_rewards)) / base.bound_return    # eval_pp.py:95
    return episode_data, epi_success, epi_rewards, base.bound_return


def _episode(h, b, N, pp):
    """Env b's first episode of a round (host arrays of _first_episodes) -> what eval_model appends for it."""
    n = int(h["first"][b]) + 1
    det = h["details"][:n, b].astype(np.float64)
    rew = h["reward"][:n, b]
    deg = np.concatenate([h["deg"][1:n, b], h["deg"][n - 1:n, b]]) if "deg" in h else np.full(n, N)
    nA = float(N)
    if pp:                                                                  # predator_prey.py:440-448
        cols = dict(capture_cnt=det[:, 0], move_cnt=det[:, 1] / nA, penalty_cnt=det[:, 2],
                    variable=det[:, 4] / nA, vars2=np.zeros(n))
    else:                                                                   # coverage.py:308-315
        cols = dict(capture_cnt=det[:, 0] / nA, move_cnt=det[:, 1] / nA, penalty_cnt=det[:, 2] / nA,
                    variable=det[:, 4] / nA, vars2=det[:, 3] / nA)
    cols.update(reward=rew, step_cnt=np.ones(n), nodeDeg=deg)
    return n, cols, rew


def _append_episode(h, b, N, pp, episode_data, epi_success, epi_rewards, eval_rewards):
    """Env b's first episode of a round onto one policy's lists: what eval_model returns per episode (the per-step success and
    VECTORS lists, the final success, per vector the episode's sum - mean for nodeDeg) and the return behind
    last_eval_average_reward."""
    n, cols, rew = _episode(h, b, N, pp)
    episode_data.append((h["success"][:n, b].tolist(), {vec: cols[vec].tolist() for vec in VECTORS}))
    epi_success.append(int(h["success"][n - 1, b]))
    for vec in VECTORS:
        epi_rewards[vec].append(float(np.mean(cols[vec]) if vec == 'nodeDeg' else np.sum(cols[vec])))
    eval_rewards.append(float(rew.sum()))


def eval_models(env, policies, itr=None, n_eval_episodes=100, max_env_steps=200, eval_greedy=True, render=False,
                inspect_steps=False, seed=1, flag=None):
    """eval_model for K policies of one architecture at once (e.g. the checkpoints of a run): the B envs of `env` are split
    into K contiguous groups of B / K, policy k playing on group k, all K in the same rollout (one launch per round's chunk
    on the wave-owned kernel of teams of 4, nets.PolicySet).  -> list of K tuples (episode_data, epi_success, epi_rewards,
    bound_return); tuple k is exactly eval_model(W_k, policies[k], ...) for W_k a fresh wrapper of env's class, params and seed
    with n_envs = B / K and env_id_offset = env's + k B / K.  Comm-DP nets of other than the default layer sizes, also of
    different sizes, take one forward launch per step when passed as nets.PolicySet(policies, any_sizes=True) (the same holds
    for eval_summary and eval_sweep); as a list they step member by member.  Afterwards env.eval_n_epi is the episode count of one policy and
    env.last_eval_average_reward the list of the K policies' averages."""
    if render or inspect_steps:
        raise NotImplementedError("rendering is outside the MI355X path")
    if flag is not None and flag[0]:
        return [(None, None, None, None) for _ in policies]
    ps = policies if isinstance(policies, PolicySet) else PolicySet(policies)
    base = getattr(env, "env", env)
    batch = base.batch
    B, N, K = batch.B, batch.N, len(ps)
    if B % K:
        raise ValueError(f"eval_models: the {B} envs of the wrapper do not split evenly between {K} policies")
    Bk = B // K
    pp = batch.scenario == "pp"
    T = int(max_env_steps)
    if T > batch.cfg.max_path_length:
        raise ValueError(f"max_env_steps={T} exceeds the env's max_path_length={batch.cfg.max_path_length}")
    env.eval_n_epi = 0
    ps.sync_weights()
    ps.reset([True] * Bk)
    eng = RolloutEngine(batch, ps, T, store_attn=False, store_probs=False, groups=[Bk] * K)
    data = [[] for _ in range(K)]
    success = [[] for _ in range(K)]
    epi_rewards = [{vec: [] for vec in VECTORS} for _ in range(K)]
    eval_rewards = [[] for _ in range(K)]
    while len(data[0]) < n_eval_episodes:                 # every group has Bk envs: the same number of rounds for each
        h = _first_episodes(eng, base, T, bool(eval_greedy), chunk=True)
        take = min(Bk, n_eval_episodes - len(data[0]))
        for k, (lo, _) in enumerate(eng.groups):
            for b in range(lo, lo + take):
                _append_episode(h, b, N, pp, data[k], success[k], epi_rewards[k], eval_rewards[k])
    env.eval_n_epi = len(data[0])
    env.last_eval_average_reward = [(sum(r) / len(r)) / base.bound_return for r in eval_rewards]
    return [(data[k], success[k], epi_rewards[k], base.bound_return) for k in range(K)]


SUMMARY_STATS = ['return_std', 'return_min', 'return_max']     # cm_episode_means columns behind the CM_EPI_COLS means
COMM_STATS = ['range_degree', 'heard_degree', 'reach', 'range_reach']   # cm_episode_comm / cm_comm_means columns
COMM_KEYS = COMM_STATS + ['delivery']                          # what comm_stats=True adds to a summary dict
ATTN_STATS = ['self', 'entropy', 'range_mass', 'kept_mass', 'eff_self', 'eff_entropy']   # cm_episode_attn / cm_attn_means columns
ATTN_KEYS = ['attn_' + name for name in ATTN_STATS]            # what attn_stats=True adds to a summary dict
LISTEN_STATS = ['kl', 'tv', 'flip']                            # per counterfactual: cm_episode_listen / cm_listen_means columns
LISTEN_KEYS = ['listen_' + name for name in LISTEN_STATS] + ['loss_' + name for name in LISTEN_STATS]   # listen_stats=True: mute, lossless
VALUE_STATS = ['value', 'ret', 'sq_err', 'ret_sq', 'msg_value', 'loss_value']   # cm_episode_value / cm_value_means columns
VALUE_KEYS = ['value_mean', 'value_return', 'value_bias', 'value_rmse', 'value_ev', 'msg_value', 'loss_value']   # value_stats=True


def _round_channels(eng, batch):
    """-> (channels, stride in floats) of a round's graphs for cm_comm_stats / cm_attn_stats: the engine's recorded blocks, NULL
    (ones) for a constant FC channel, the batch's constant block (the identity) with stride 0 for a constant FL channel."""
    if eng.channels is not None:
        return eng.channels, batch.Lh * batch.N * batch.N
    if batch.channelType == "FC":
        return None, 0
    return batch.channels, 0


def _counterfactuals(eng, batch, graph=True):
    """-> (mute, lossless): which counterfactual replays a round needs - under the identity (every agent hears only itself) and under
    the all-ones channel (everything in range is delivered).  A constant FL channel IS the mute one and a constant FC channel the
    lossless one: that replay is skipped - no buffer, no forward, the counterfactual passed as NULL (its columns exact 0).  graph:
    the nets read the channel at all (a critic without a graph input needs neither)."""
    const = batch.channelType if eng.channels is None else None               # the channel every slot of every round has
    return graph and const != "FL", graph and const != "FC"


# ---- what produces a family's per-step rows: called once per call with the engine, the batch, T and the side's `stats` (it may
# allocate its own buffers then), -> the round's launches.  (Nothing here refers back to the _Side: no reference cycle keeps the
# device buffers waiting for the garbage collector.) ----
def _comm_rows(eng, batch, T, stats):
    """cm_comm_stats on the engine's dist_adj / channels, all T + 1 slots of all B envs.  A constant fully connected adjacency and a
    constant FC channel are passed as NULL (ones), a constant FL channel as the batch's constant block with stride 0."""
    B, N, Lh = batch.B, batch.N, batch.Lh

    def fill():
        chan, chan_stride = _round_channels(eng, batch)
        L.run("cm_comm_stats", (T + 1) * B, N, Lh, L.ptr(eng.dist_adj), N * N, L.ptr(chan), chan_stride, L.ptr(stats))
    return fill


def _attn_rows(eng, batch, T, stats):
    """cm_attn_stats over the round's T x B graphs, on an engine built with store_attn=True: attn[t] with dist_adj[t] / channels[t],
    the graph the forward of step t read; constant masks by _comm_rows' rules."""
    B, N, Lh = batch.B, batch.N, batch.Lh

    def fill():
        chan, chan_stride = _round_channels(eng, batch)
        L.run("cm_attn_stats", T * B, N, Lh, L.ptr(eng.attn), N * N, L.ptr(eng.dist_adj), N * N, L.ptr(chan), chan_stride, L.ptr(stats))
    return fill


def _listen_rows(eng, batch, T, stats):
    """The counterfactual replays of the round's T slots (RolloutEngine.replay_probs: "identity" = mute, "ones" = lossless; skipped
    by _counterfactuals' rule) into two buffers [T, B, N, A], then cm_listen_stats comparing the recorded probs - the engine is built
    with store_probs=True - with them over the round's T x B graphs."""
    B, N, A = batch.B, batch.N, eng.policy._action_dim
    mute, lossless = (torch.empty(T, B, N, A, dtype=torch.float32, device=batch.device) if wanted else None
                      for wanted in _counterfactuals(eng, batch))

    def fill():
        if mute is not None:
            eng.replay_probs(0, T, "identity", mute)
        if lossless is not None:
            eng.replay_probs(0, T, "ones", lossless)
        L.run("cm_listen_stats", T * B, N, A, L.ptr(eng.probs), N * A, L.ptr(mute), N * A, L.ptr(lossless), N * A, L.ptr(stats))
    return fill


def _value_rows(eng, batch, T, stats, critics, discount):
    """The critics' values of the round's T slots (RolloutEngine.replay_values "recorded", and for Comm-DP critics "identity" = mute
    and "ones" = lossless, skipped by _counterfactuals' rule) into buffers [T, B], then cm_value_stats over the round's T x B steps
    against the engine's reward64 / path_len.  `critics` is what replay_values takes: one critic, or a list with one per member."""
    graph = all(hasattr(c, "comm") for c in (critics if isinstance(critics, list) else [critics]))   # Comm-DP critics
    values, mute, lossless = (torch.empty(T, batch.B, dtype=torch.float32, device=batch.device) if wanted else None
                              for wanted in (True,) + _counterfactuals(eng, batch, graph))

    def fill():
        eng.replay_values(0, T, "recorded", critics, values)
        if mute is not None:
            eng.replay_values(0, T, "identity", critics, mute)
        if lossless is not None:
            eng.replay_values(0, T, "ones", critics, lossless)
        L.run("cm_value_stats", T, batch.B, L.ptr(eng.reward64), L.ptr(eng.path_len), L.ptr(values), L.ptr(mute), L.ptr(lossless),
              float(discount), L.ptr(stats))
    return fill


class _Side:
    """One statistics family (a _Family of FAMILIES) of an eval_summary / eval_sweep call: its device state - `stats`, the round's
    per-step rows; `table` [cells, n_epi, cols], the episode rows; with curves `sums` [cells, T, cols], the per-step sums - and its
    launches.  Behind every round the family's rows (_Family.rows: ONE stats launch, for listen and value behind their replays) and
    ONE cm_episode_<name> launch into the table, with curves ONE cm_<name>_curves launch more; after the last round ONE
    cm_<name>_means launch and with curves ONE cm_<name>_curve_means launch, into `out` ([cells, cols]) and `curve_out`
    ([cells, T, cols] or None), views of the buffer the caller copies to the host.
    The comm family (curves_last) predates the curves: its two curve launches come behind _Curves', not with its own round and
    means, and the launch order is part of the contract - so the caller runs round_curves / curve_means for it behind _Curves."""

    def __init__(self, fam, eng, batch, T, cells, n_epi, out, curve_out, **given):
        self.fam, self.eng, self.batch, self.T = fam, eng, batch, T
        self.cells, self.n_epi, self.out, self.curve_out = cells, n_epi, out, curve_out
        f64 = dict(dtype=torch.float64, device=batch.device)
        self.stats = torch.empty(T + fam.more_slots, batch.B, fam.cols, dtype=fam.dtype, device=batch.device)
        self.table = torch.zeros(cells, n_epi, fam.cols, **f64)
        self.sums = None if curve_out is None else torch.empty(cells, T, fam.cols, **f64)
        self.sizes = fam.sizes(batch)                           # the reductions' trailing size arguments
        self.fill = fam.rows(eng, batch, T, self.stats, **given)

    def round(self, group_size, take, row0):
        self.fill()
        L.run(f"cm_episode_{self.fam.name}", self.T, self.batch.B, *self.sizes, L.ptr(self.eng.path_len), L.ptr(self.stats),
              group_size, take, self.n_epi, row0, L.ptr(self.table))
        if not self.fam.curves_last:
            self.round_curves(group_size, take, row0)

    def round_curves(self, group_size, take, row0):
        if self.sums is not None:                               # the first round overwrites the sums, the later ones add
            L.run(f"cm_{self.fam.name}_curves", self.T, self.batch.B, *self.sizes, L.ptr(self.eng.path_len), L.ptr(self.stats),
                  group_size, take, int(row0 > 0), L.ptr(self.sums))

    def means(self):
        L.run(f"cm_{self.fam.name}_means", self.cells, self.n_epi, L.ptr(self.table), L.ptr(self.out))
        if not self.fam.curves_last:
            self.curve_means()

    def curve_means(self):
        if self.sums is not None:
            L.run(f"cm_{self.fam.name}_curve_means", self.cells, self.T, self.n_epi, *self.sizes, L.ptr(self.sums),
                  L.ptr(self.curve_out))


def _check_baselines(who, policies, value_stats, baselines):
    """The refusals of value_stats= / baselines= (ValueErrors naming value_stats, before anything is built; `policies` a list)
    -> the critics: one per policy, in order, or None with the switch off."""
    if not value_stats and baselines is None:
        return None
    if baselines is None:
        raise ValueError(f"{who}: value_stats=True needs baselines= (the critic trained with each policy)")
    if not value_stats:
        raise ValueError(f"{who}: baselines= is read by value_stats=True only")
    critics = list(baselines) if isinstance(baselines, (list, tuple)) else [baselines]
    if len(critics) != len(policies):
        raise ValueError(f"{who}: value_stats=True needs one critic per policy in baselines= ({len(critics)} for {len(policies)})")
    for k, (c, p) in enumerate(zip(critics, policies)):
        if not callable(getattr(c, "values_device", None)):
            raise ValueError(f"{who}: value_stats=True: baselines[{k}] has no values_device (a nets.CommBaseCritic or nets.GaussianMLPBaseline)")
        if type(c) is not type(critics[0]):
            raise ValueError(f"{who}: value_stats=True: the critics are of different classes ({type(critics[0]).__name__}, "
                             f"{type(c).__name__})")
        team = getattr(c, "_n_agents", None)                    # (a GaussianMLPBaseline knows the width of the joint observation only)
        width = c.input_dim if team is None else team * c._dec_obs_dim
        if (team is not None and team != p._n_agents) or width != p._n_agents * p._dec_obs_dim:
            raise ValueError(f"{who}: value_stats=True: baselines[{k}] was built for another team size or observation width than "
                             f"its policy ({p._n_agents} agents x {p._dec_obs_dim})")
    return critics


def _explained(sq_err, bias, ret, ret_sq):
    """1 - Var[G - v] / Var[G] from the moments (arrays or floats) -> array; where Var[G] <= eps = 1e-12 max(1, E[G^2]): 1 where the
    residual variance is <= eps too, else 0."""
    sq_err, bias, ret, ret_sq = (np.asarray(x, np.float64) for x in (sq_err, bias, ret, ret_sq))
    resid, var = sq_err - bias * bias, ret_sq - ret * ret
    eps = 1e-12 * np.maximum(1.0, ret_sq)
    flat = var <= eps
    return np.where(flat, np.where(resid <= eps, 1.0, 0.0), 1.0 - resid / np.where(flat, 1.0, var))


def _value_keys(cols):
    """The six cm_value_means columns (the means per step: floats, or arrays over the cells) -> the VALUE_KEYS dict."""
    mean, ret, sq_err, ret_sq, msg, loss = cols
    bias = mean - ret
    return dict(value_mean=mean, value_return=ret, value_bias=bias, value_rmse=np.sqrt(sq_err),
                value_ev=_explained(sq_err, bias, ret, ret_sq)[()], msg_value=msg, loss_value=loss)


def _value_curve_keys(cols, step_cnt):
    """The six columns of zero-padded means over the steps ([6, T] of a cell, or [6, cells, T]) and the step_cnt curves (the share
    of episodes still running at step t) -> the VALUE_KEYS curves: value_rmse and value_ev over the episodes still running (0 and 1
    where none does)."""
    mean, ret, sq_err, ret_sq, msg, loss = cols
    some = step_cnt > 0
    run = lambda x: np.where(some, x / np.where(some, step_cnt, 1.0), 0.0)           # noqa: E731
    r_mean, r_ret, r_sq, r_rsq = run(mean), run(ret), run(sq_err), run(ret_sq)
    return dict(value_mean=mean, value_return=ret, value_bias=mean - ret, value_rmse=np.sqrt(r_sq),
                value_ev=np.where(some, _explained(r_sq, r_mean - r_ret, r_ret, r_rsq), 1.0), msg_value=msg, loss_value=loss)


def _comm_keys(cols):
    """The four cm_comm_means columns (floats, or arrays over the cells, or over cells and steps) -> the COMM_KEYS dict: delivery =
    heard_degree / range_degree, 1.0 where nobody is in range."""
    d = dict(zip(COMM_STATS, cols))
    some = d["range_degree"] != 0
    d["delivery"] = np.where(some, d["heard_degree"] / np.where(some, d["range_degree"], 1.0), 1.0)
    return d


def _named(names):
    """-> keys(cols) of a family whose keys are its columns."""
    return lambda cols: dict(zip(names, cols))


# What tells the statistics families apart.  name: the stem of the four reductions cm_episode_<name>, cm_<name>_means,
# cm_<name>_curves, cm_<name>_curve_means and of the buffer's sections; cols / dtype / more_slots: a step row of `stats`
# [T + more_slots, B, cols] (an episode row has the same columns); sizes(batch): the reductions' trailing size arguments; rows(eng,
# ...): what produces a round's stats (above); keys(cols): the host side, elementwise on the columns of the family's means
# ([cols, cells]) -> what the dicts gain, and on those of its curves ([cols, cells, T]) -> what their `curves` gain - the latter
# through curve_keys(cols, step_cnt) where the curves need the share of running episodes; curves_last: the curve launches and
# sections come behind the episode curves', not with the family's own (_Side); kind: how cm_boot_quantiles forms the family's keys
# from a row of resampled means (envs.BOOT_KINDS) - the device twin of keys(cols), in the same order.
_Family = collections.namedtuple("_Family", "name cols dtype more_slots sizes rows keys curve_keys curves_last kind",
                                 defaults=(None, False, "columns"))
FAMILIES = dict(
    comm_stats=_Family("comm", L.COMM_COLS, torch.int32, 1, lambda batch: (batch.N, batch.Lh), _comm_rows, _comm_keys,
                       curves_last=True, kind="comm"),
    attn_stats=_Family("attn", L.ATTN_COLS, torch.float64, 0, lambda batch: (batch.N, batch.Lh), _attn_rows,
                       _named(ATTN_KEYS)),
    listen_stats=_Family("listen", L.LISTEN_COLS, torch.float64, 0, lambda batch: (batch.N,), _listen_rows,
                         _named(LISTEN_KEYS)),
    value_stats=_Family("value", L.VALUE_COLS, torch.float64, 0, lambda batch: (), _value_rows, _value_keys,
                        _value_curve_keys, kind="value"))


class _Curves:
    """The curves=True side of eval_summary / eval_sweep: behind every round ONE cm_episode_curves launch on the engine's
    trajectory buffers into the device table of per-step sums [cells, T, 9] - the first round overwrites it, the later ones add;
    after the last round ONE cm_curve_means launch into `out`, a view of the buffer the caller copies to the host."""

    def __init__(self, eng, batch, T, cells, n_epi, scen, out):
        self.eng, self.batch, self.T, self.cells, self.n_epi, self.scen, self.out = eng, batch, T, cells, n_epi, scen, out
        self.sums = torch.empty(cells, T, L.EPI_COLS, dtype=torch.float64, device=batch.device)

    def round(self, group_size, take, row0):
        eng, batch = self.eng, self.batch
        L.run("cm_episode_curves", self.T, batch.B, batch.N, self.scen, L.ptr(eng.reward64), L.ptr(eng.details), L.ptr(eng.success),
              L.ptr(eng.path_len), L.ptr(eng.dist_adj), group_size, take, int(row0 > 0), L.ptr(self.sums))

    def means(self):
        L.run("cm_curve_means", self.cells, self.T, self.n_epi, self.scen, self.batch.N, L.ptr(self.sums), L.ptr(self.out))

    @staticmethod
    def keys(rows):
        """The host table [cells, 9, T] -> per cell its `curves` dict."""
        return [dict(zip(['success'] + VECTORS, cell)) for cell in rows]


def _layout(cells, T, fams, curves, boot=()):
    """The one buffer that is copied to the host, as both sides read it: the ordered (name, shape) of its sections of doubles for
    the active families `fams` (in FAMILIES' order).  The summary [cells, 12]; a curves_last family's means [cells, cols]; with
    curves the episode curves [cells, T, 9] and that family's "<name>_curves" [cells, T, cols]; then per other family "<name>"
    and with curves "<name>_curves".  boot: behind all of these, per name of `boot` ("boot" with ci=, then "contrast" with
    contrast=) the cm_boot_quantiles blocks "summary_<name>" [cells, 9, 4] and per family "<family>_<name>" [cells, keys, 4]."""
    first, rest = [f for f in fams if f.curves_last], [f for f in fams if not f.curves_last]
    sections = [("summary", (cells, L.SUM_COLS))] + [(f.name, (cells, f.cols)) for f in first]
    if curves:
        sections += [("curves", (cells, T, L.EPI_COLS))] + [(f.name + "_curves", (cells, T, f.cols)) for f in first]
    for f in rest:
        sections += [(f.name, (cells, f.cols))] + ([(f.name + "_curves", (cells, T, f.cols))] if curves else [])
    for b in boot:
        sections += [(f"summary_{b}", (cells, L.EPI_COLS, L.BOOT_OUT))]
        sections += [(f"{f.name}_{b}", (cells, _envs.boot_keys(f.kind, f.cols), L.BOOT_OUT)) for f in fams]
    return sections


def _cut(flat, layout):
    """-> {name: its section of `flat`, shaped}: views of the device buffer (a torch tensor) or of its host copy (a numpy array)."""
    ends = itertools.accumulate(math.prod(shape) for _, shape in layout)
    return {name: flat[end - math.prod(shape):end].reshape(shape) for (name, shape), end in zip(layout, ends)}


def _host_tables(host_all, layout):
    """_cut of the host copy, with one transposition per curve table: [cells, cols, T], a cell's curve is then a contiguous row."""
    return {name: np.ascontiguousarray(part.transpose(0, 2, 1)) if name.endswith("curves") else part
            for name, part in _cut(host_all, layout).items()}


def _check_boot(who, ci, n_boot, boot_seed, contrast, sweep, paired):
    """The refusals of ci= / n_boot= / boot_seed= / contrast= that need no cell count (ValueErrors naming the keyword, before
    anything is built) -> None with ci off, else the interval's (lo_rank, hi_rank) (envs.boot_ranks).  Off, the other three must
    be at their defaults: a resample count or seed nobody reads is refused, not ignored."""
    if contrast is not None and not sweep:
        raise ValueError(f"{who}: contrast= is eval_sweep's (the policies of eval_summary play unpaired envs: no paired difference)")
    if ci is None:
        for name, given, default in (("n_boot", n_boot, 2000), ("boot_seed", boot_seed, 0), ("contrast", contrast, None)):
            if given != default:
                raise ValueError(f"{who}: {name}= is read with ci= only (ci=None: no intervals)")
        return None
    ranks = _envs.boot_ranks(ci, n_boot, who, "ci")
    _envs.boot_seed_words(boot_seed, who, "boot_seed")
    if contrast is not None:
        if not paired:
            raise ValueError(f"{who}: contrast= needs paired=True (row e of two cells must be the same scenario)")
        if not isinstance(contrast, dict) or len(contrast) != 1 or next(iter(contrast)) not in ("condition", "policy"):
            raise ValueError(f"{who}: contrast= takes dict(condition=c0) or dict(policy=k0), not {contrast!r}")
    return ranks


def _contrast_cells(who, contrast, K, C_):
    """contrast= of eval_sweep over K policies x C_ conditions -> per cell g = k*C_ + c the cell it is compared with: (k, c0) for
    dict(condition=c0), (k0, c) for dict(policy=k0); None without.  ValueError naming contrast for an index out of range."""
    if contrast is None:
        return None
    (axis, at), = contrast.items()
    size = C_ if axis == "condition" else K
    if isinstance(at, bool) or not isinstance(at, (int, np.integer)) or not 0 <= at < size:
        raise ValueError(f"{who}: contrast=dict({axis}={at!r}): the index must lie in 0..{size - 1}")
    at = int(at)
    return [(g // C_) * C_ + at if axis == "condition" else at * C_ + g % C_ for g in range(K * C_)]


def _score(who, env, policies, n_eval_episodes, max_env_steps, eval_greedy, flag, episodes, comm_stats, conds=None, paired=True,
           curves=False, attn_stats=False, ci=None, n_boot=2000, boot_seed=0, contrast=None, listen_stats=False,
           value_stats=False, baselines=None, discount=0.99):
    """eval_summary (conds None: one cell per policy) and eval_sweep (one cell per policy and condition) - `who` for the
    refusals' texts.  The B envs are K policies x C conditions x E envs, cell g = k*C + c owning the contiguous envs
    [g*E, (g+1)*E), policy k the C*E envs of its cells: the engine's groups.  The refusals; the engine (it keeps its attention
    output for attn_stats and its probabilities for listen_stats; `baselines` checked by _check_baselines and synced); the active
    _Sides in FAMILIES' order, their views cut from the one buffer by _layout.  Per round _play_round, the episode rows of groups of
    E envs into the device table [K*C, n_eval_episodes, 9], every side's round, _Curves.round and the curves_last sides' curve sums;
    then the means in the same order, the one copy to the host, and the dicts from the sides' keys.  With ci= behind the means, per
    table (the summary's, then every side's) ONE cm_boot_means launch into a scratch [cells, n_boot, cols] and ONE cm_boot_quantiles
    launch - with contrast= one more, against the cells of _contrast_cells - into sections of the same buffer."""
    ranks = _check_boot(who, ci, n_boot, boot_seed, contrast, conds is not None, paired)
    single = not isinstance(policies, (PolicySet, list, tuple))
    comm_dp = all(hasattr(p, "comm") for p in ([policies] if single else policies))
    if attn_stats and not comm_dp:
        raise ValueError(f"{who}: attn_stats=True needs Comm-DP policies (an Obs-DP / CENT policy has no attention output)")
    if listen_stats and not comm_dp:
        raise ValueError(f"{who}: listen_stats=True needs Comm-DP policies (an Obs-DP / CENT policy hears no messages)")
    critics = _check_baselines(who, [policies] if single else list(policies), value_stats, baselines)
    if critics is not None and not (np.isfinite(discount) and 0 <= discount <= 1):
        raise ValueError(f"{who}: value_stats=True needs 0 <= discount <= 1, not {discount!r}")
    C_ = 1 if conds is None else len(conds)
    ref_of = _contrast_cells(who, contrast, 1 if single else len(policies), C_)

    def shaped(cells):
        """K*C values in cell order -> the caller's [K] (eval_summary) or [K][C] (eval_sweep); a single policy: its entry."""
        per = cells if conds is None else [cells[i:i + C_] for i in range(0, len(cells), C_)]
        return per[0] if single else per

    if flag is not None and flag[0]:
        return shaped([None] * ((1 if single else len(policies)) * C_))
    base = getattr(env, "env", env)
    batch = base.batch
    B, N = batch.B, batch.N
    T = int(max_env_steps)
    if single:
        ps, K = policies, 1
    else:
        ps = policies if isinstance(policies, PolicySet) else PolicySet(policies)
        K = len(ps)
    cells = K * C_
    if B % cells:
        raise ValueError(f"{who}: the {B} envs of the wrapper do not split evenly between {K} policies"
                         + ("" if conds is None else f" x {C_} conditions"))
    E = B // cells
    if T > batch.cfg.max_path_length:
        raise ValueError(f"max_env_steps={T} exceeds the env's max_path_length={batch.cfg.max_path_length}")
    n_epi = int(n_eval_episodes)
    if n_epi < 1:
        raise ValueError(f"{who}: n_eval_episodes must be at least 1")
    if conds is not None:
        batch.set_conditions(conds, *sweep_layout(B, K, C_, batch.cfg.env_id_offset, paired))
    env.eval_n_epi = 0
    ps.sync_weights()
    for c in critics or ():
        c.sync_weights()
    ps.reset([True] * (C_ * E))
    eng = RolloutEngine(batch, ps, T, store_attn=bool(attn_stats), store_probs=bool(listen_stats),
                        **({} if single else dict(groups=[C_ * E] * K)))
    # eval_summary of a single policy plays eval_model's rounds, which step one by one; every other call asks for the chunk
    # launch, as eval_models does.  A conditions batch declines the fused forms (two launches per step) unless the wrapper was
    # built with fused_conditions=True (GridEnvBatch.fuse_conditions): then teams of 4 play the round as one launch, a single
    # policy included
    chunk = conds is not None or not single
    scen = L.CM_PP if batch.scenario == "pp" else L.CM_CO
    table = torch.zeros(cells, n_epi, L.EPI_COLS, dtype=torch.float64, device=batch.device)
    on = dict(comm_stats=comm_stats, attn_stats=attn_stats, listen_stats=listen_stats, value_stats=critics is not None)
    given = dict(value_stats=dict(critics=critics and (critics[0] if single else critics), discount=discount))
    boot = () if ranks is None else ("boot",) if ref_of is None else ("boot", "contrast")
    layout = _layout(cells, T, [fam for switch, fam in FAMILIES.items() if on[switch]], bool(curves), boot)
    flat = torch.empty(sum(math.prod(shape) for _, shape in layout), dtype=torch.float64, device=batch.device)
    views = _cut(flat, layout)
    sides = [_Side(fam, eng, batch, T, cells, n_epi, views[fam.name], views.get(fam.name + "_curves"), **given.get(switch, {}))
             for switch, fam in FAMILIES.items() if on[switch]]
    last = [side for side in sides if side.fam.curves_last]
    curve = _Curves(eng, batch, T, cells, n_epi, scen, views["curves"]) if curves else None
    done = 0
    while done < n_epi:
        _play_round(eng, batch, T, bool(eval_greedy), chunk)
        take = min(E, n_epi - done)
        L.run("cm_episode_stats", T, B, N, scen, L.ptr(eng.reward64), L.ptr(eng.details), L.ptr(eng.success), L.ptr(eng.path_len),
              L.ptr(eng.dist_adj), E, take, n_epi, done, L.ptr(table))
        for side in sides:
            side.round(E, take, done)
        if curve:
            curve.round(E, take, done)
        for side in last:
            side.round_curves(E, take, done)
        done += take
    L.run("cm_episode_means", cells, n_epi, L.ptr(table), L.ptr(views["summary"]))
    for side in sides:
        side.means()
    if curve:
        curve.means()
    for side in last:
        side.curve_means()
    if boot:                                                    # every table resampled by the same index stream (boot_seed)
        ref_dev = None if ref_of is None else torch.tensor(ref_of, dtype=torch.int32, device=batch.device)
        for name, rows, kind in [("summary", table, "columns")] + [(side.fam.name, side.table, side.fam.kind) for side in sides]:
            resampled = _envs.boot_means(rows, n_boot, boot_seed)               # [cells, n_boot, cols]: freed with the call
            _envs.boot_quantiles(resampled, *ranks, kind, out=views[name + "_boot"])
            if ref_dev is not None:
                _envs.boot_quantiles(resampled, *ranks, kind, ref_dev, out=views[name + "_contrast"])
    host = _host_tables(flat.cpu().numpy(), layout)
    bound = base.bound_return
    by_cols = lambda name: np.moveaxis(host[name], 1, 0)                   # noqa: E731  [cols, cells] or [cols, cells, T]
    side_keys = [side.fam.keys(by_cols(side.fam.name)) for side in sides]    # per side: name -> [cells]
    cell_curves = curve.keys(host["curves"]) if curve else None
    for fam in (side.fam for side in sides if curve):
        cols = by_cols(fam.name + "_curves")
        step_cnt = by_cols("curves")[1 + VECTORS.index("step_cnt")]                                  # [cells, T]
        more = fam.keys(cols) if fam.curve_keys is None else fam.curve_keys(cols, step_cnt)
        for g, d in enumerate(cell_curves):
            d.update({name: v[g] for name, v in more.items()})
    res = []
    for g, row in enumerate(host["summary"]):
        d = dict(n_episodes=n_epi, success=float(row[0]))
        d.update({vec: float(row[1 + i]) for i, vec in enumerate(VECTORS)})
        d.update({name: float(row[L.EPI_COLS + i]) for i, name in enumerate(SUMMARY_STATS)})
        d["bound_return"] = bound
        if conds is not None:
            d["condition"] = conds[g % C_]
        if episodes:
            d["episodes"] = table[g]
        for side, keys in zip(sides, side_keys):
            d.update({name: float(v[g]) for name, v in keys.items()})
            if episodes:
                d[side.fam.name + "_episodes"] = side.table[g]
        if curve:
            d["curves"] = cell_curves[g]
        res.append(d)
    # the bootstrap blocks, [cells, keys, 4] each: the summary's keys are its nine means, a side's its keys in their order
    named = [(["success"] + VECTORS, "summary")] + [(list(keys), side.fam.name) for side, keys in zip(sides, side_keys)]
    blocks = {b: [host[f"{tab}_{b}"].tolist() for _, tab in named] for b in boot}      # (floats at once, not one numpy scalar a time)
    for g, d in enumerate(res if boot else ()):
        rows = [(name, block[g][i]) for (names, _), block in zip(named, blocks["boot"]) for i, name in enumerate(names)]
        d["ci"] = {name: (lo, hi) for name, (lo, hi, _, _) in rows}
        d["se"] = {name: se for name, (_, _, se, _) in rows}
        if ref_of is not None:                                  # diff: of the point estimates already here
            to = res[ref_of[g]]
            d["contrast"] = {name: dict(diff=d[name] - to[name], lo=row[0], hi=row[1], se=row[2], p_gt=row[3])
                             for (names, _), block in zip(named, blocks["contrast"]) for i, name in enumerate(names)
                             for row in (block[g][i],)}
            d["contrast_ref"] = (ref_of[g] // C_, ref_of[g] % C_)
    env.eval_n_epi = n_epi
    env.last_eval_average_reward = shaped([d["reward"] / bound for d in res])
    return shaped(res)


def eval_summary(env, policies, itr=None, n_eval_episodes=100, max_env_steps=200, eval_greedy=True, seed=1, flag=None,
                 episodes=False, comm_stats=False, curves=False, attn_stats=False, ci=None, n_boot=2000, boot_seed=0,
                 contrast=None, listen_stats=False, value_stats=False, baselines=None, discount=0.99):
    """The score of one policy, a list of policies or a nets.PolicySet: the episodes eval_models plays (one policy: the ones
    eval_model plays), reduced on the device instead of copied to the host.  Behind every round ONE cm_episode_stats launch on
    the engine's trajectory buffers writes the round's episode rows into a device table [K, n_eval_episodes, 9] (success, then
    VECTORS: the per-episode values eval_model returns as epi_success / epi_rewards); ONE cm_episode_means launch then reduces
    the table, and its [K, 12] doubles are the only device-to-host copy of the call.
    -> a list of K dicts (one dict for a single policy): n_episodes; success and every name of VECTORS, each the mean over the
    episodes (the columns of exp_runners/testing.py:329, see summary_row); return_std (population), return_min, return_max of
    the episode returns; bound_return; with episodes=True also `episodes`, the policy's [n_eval_episodes, 9] slice of the table
    as a device tensor (column 1 is what testing.py keeps as rewMat2).  Sums are f64 in a fixed order: two calls on the same
    episodes give the same bits; against the host loop the values agree to f64 rounding (nodeDeg to f32 rounding, the host
    path rounds each step's degree to f32).
    bound_return is the scalar env.bound_return for both scenarios: the Coverage twin of eval_model differs only in returning
    it once per episode, so there is no _co entry here.  render / inspect_steps are not parameters (UI is out of scope).
    flag[0] set returns None per policy, as eval_models returns its empty tuples.  Afterwards env.eval_n_epi and
    env.last_eval_average_reward (a list of K for several policies) are what eval_models / eval_model leave.
    The five switches below have this in common.  A statistics family <f> (comm, attn, listen, value) takes, behind every round,
    ONE cm_<f>_stats launch over the round's recorded slots (for listen and value behind their forward-only replays) and ONE
    cm_episode_<f> launch into a device table [K, n_eval_episodes, cols] (with curves ONE cm_<f>_curves more, into per-step
    sums [K, T, cols]); after the last round ONE cm_<f>_means launch (with curves ONE cm_<f>_curve_means more).  Their doubles
    ride in the same single device-to-host copy as the summary.  Sums are integers or f64 in one fixed order and every value is
    divided once: the same episodes give the same bits.  With episodes=True a family also returns `<f>_episodes`, its
    [n_eval_episodes, cols] slice of the table as a device tensor, and with curves=True its keys also in `curves`.  Off (the
    default), a switch launches, allocates and returns nothing, and everything else is bit for bit the same.
    comm_stats=True adds the communication statistics of the graphs the policy acted through (slots 0 .. n-1 of each episode;
    include/commarl.h, cm_comm_stats, on the engine's dist_adj / channels).  Every dict gains range_degree (mean number of agents
    in range), heard_degree (mean number heard per hop), reach (mean number of team mates whose information can arrive within the
    net's hops), range_reach (the same without channel loss) and delivery = heard_degree / range_degree (1.0 when nobody is in
    range); `comm_episodes` holds the first four.
    curves=True adds `curves` to every dict: numpy float64 arrays of length max_env_steps keyed success and every name of
    VECTORS - entry t is the mean over ALL n_eval_episodes episodes of the per-step value eval_model lists for step t, an episode
    that has ended counting as zero (the reference pads its per-step lists with zeros to max_env_steps before it saves them as
    rewMat3, testing.py:307-324).  curves['step_cnt'][t] is therefore the share of episodes still running at step t, and another
    curve divided by it the mean over the running episodes; a summed vector's curve adds up to the vector's summary value.  With
    comm_stats=True also every name of COMM_KEYS, from the graphs the policies acted through at step t (delivery[t] =
    heard_degree[t] / range_degree[t], 1.0 where nobody is in range - or no episode runs).  Behind every round ONE
    cm_episode_curves launch adds the round's per-step sums to a device table [K, T, 9], after the last round ONE cm_curve_means
    launch divides them (the comm family's two curve launches come behind these).  Integer-valued sums are exact, the reward
    sums have one fixed order.
    attn_stats=True (Comm-DP policies; anything else raises ValueError before anything is built) adds what the policy did with
    what was delivered.  The engine then keeps the attention matrix M every forward writes - row i is agent i's softmax over the
    team, BEFORE any mask (the reference's attention_weights); for hop l the net uses M * dist_adj * channels[l] renormalised
    per row.  Every dict gains ATTN_KEYS, means per agent over the graphs the policy acted through (the last three also per hop):
    attn_self (weight on the agent itself), attn_entropy (nats, of a row of M), attn_range_mass (attention on agents in range),
    attn_kept_mass (attention on links that carried something), attn_eff_self and attn_eff_entropy (self weight and entropy of
    the renormalised weights the hop really uses; a row with nothing kept counts as 0); `attn_episodes` holds the same six.
    Keeping M costs 4 T B N^2 bytes of device memory for the call; off, the engine keeps no attention.
    listen_stats=True (Comm-DP policies; anything else raises ValueError before anything is built) adds whether the messages
    changed what the agents did.  The engine then keeps the probabilities p it acted on, and behind every round replays the
    round's slots forward-only (RolloutEngine.replay_probs: the recorded observations and dist_adj; nothing is drawn, no recorded
    buffer and no counter moves) under two counterfactual channels: mute - the identity, every agent hears only itself - and
    lossless - all ones, everything in range is delivered.  Every dict gains LISTEN_KEYS, means per agent over the graphs the
    policy acted through of, with q the counterfactual probabilities: listen_kl = KL(p || q_mute) in nats (q floored at FLT_MIN;
    not clamped at 0), listen_tv = the total variation, listen_flip = the share of agents whose greedy action changes; loss_kl,
    loss_tv, loss_flip the same against q_lossless - what the channel loss changed in the decisions; `listen_episodes` holds the same
    six.  A replay is one forward launch per member, under the identity one per block of rollout.REPLAY_MASK_BYTES of mask.  A
    wrapper with a constant FC channel skips the lossless replay and one with a constant FL channel the mute replay: exact zeros.
    The probabilities cost 4 T B N A bytes of device memory each (recorded, mute, lossless); off, the engine keeps none.
    value_stats=True with baselines= (one critic for one policy, a list of K for K policies, critic k judging policy k's envs:
    nets.CommBaseCritic of any aggregator and layer sizes, or nets.GaussianMLPBaseline for Obs-DP / CENT policies; all of one
    class, built for their policy's team size and observation width - anything else, and either keyword without the other,
    raises ValueError before anything is built) adds how good the critic trained with the policy is.  The critics are
    sync_weights()-ed, and behind every round their values v of the round's slots are computed forward-only
    (RolloutEngine.replay_values on the recorded observations, dist_adj and channels) and compared with G, the return-to-go of
    the rewards discounted by `discount` within the episode (no bootstrap where max_env_steps cuts it).  Every dict gains
    VALUE_KEYS, from means over the steps the policy acted in: value_mean = E[v], value_return = E[G], value_bias = their
    difference, value_rmse = sqrt(E[(v - G)^2]), value_ev = 1 - Var[G - v] / Var[G] - the explained variance, 1 for a perfect
    baseline, 0 for a constant one, negative for one worse than that (where Var[G] <= 1e-12 max(1, E[G^2]): 1 if Var[G - v] is
    that small too, else 0) - and for Comm-DP critics msg_value = E[v - v_mute], what the critic believes the messages are worth
    (the outcome-side twin of listen_kl), and loss_value = E[v_lossless - v], what it believes the channel loss costs, v_mute /
    v_lossless being its values under the identity / the all-ones channel (replay_values "identity" / "ones"; a GaussianMLPBaseline
    has no graph input: exact zeros, no forward).  E is episode-balanced like every key here: a step of episode e weighs
    1 / (n_e E), n_e its length and E the number of episodes.  garage's ExplainedVariance pools the steps instead (each weighs
    1 / sum_e n_e), so long episodes count for more there; with episodes=True `value_episodes`, the [n_eval_episodes, 6] device
    table behind the keys (per episode the means over its steps of v, G, (v - G)^2, G^2, v - v_mute, v_lossless - v), times the
    `step_cnt` column of `episodes` gives the per-episode sums to pool.  With curves=True the same seven names are in `curves`:
    value_mean, value_return, value_bias, msg_value and loss_value zero-padded means like every curve, value_rmse and value_ev
    over the episodes still running at step t (0 and 1 where none does).  A replay is one forward launch per critic, under
    the identity one per block of rollout.REPLAY_MASK_BYTES of mask; the constant-channel rule of listen_stats skips the same
    replays here: exact zeros.
    ci=level (0 < level < 1; None, the default, launches, allocates and returns nothing) says how far to trust every mean above:
    a percentile bootstrap over the episodes, on the device tables.  Resample r draws n_eval_episodes episode rows with
    replacement - the same rows in every table and every cell (the Philox stream of boot_seed, include/commarl.h cm_boot_means) -
    and every key is formed from the resampled column means exactly as the point estimate is formed from the means, so delivery,
    value_bias, value_rmse and value_ev are resampled jointly, not column by column.  Every dict gains `ci`: name -> (lo, hi), the
    order statistics lo_rank = min(floor((1 - level) / 2 * n_boot), (n_boot - 1) // 2) and n_boot - 1 - lo_rank of the n_boot
    values (not interpolated), and `se`: name -> the bootstrap standard error (their standard deviation, ddof 1) - for success,
    every name of VECTORS and every key of every active family; not for return_std / return_min / return_max, bound_return or
    curves.  After the last round, per table (the summary's and each active family's) ONE cm_boot_means launch into a device
    scratch of n_boot * cols doubles per cell, freed with the call, and ONE cm_boot_quantiles launch; the [K, keys, 4] blocks ride
    in the same single copy to the host.  n_boot in 2..4096, boot_seed in 0..2^64-1; either given without ci, and ci outside
    (0, 1), raises ValueError before anything is built.  contrast= is eval_sweep's and raises ValueError here: the policies of
    this call play different envs, there is no paired difference between them."""
    return _score("eval_summary", env, policies, n_eval_episodes, max_env_steps, eval_greedy, flag, episodes, comm_stats,
                  curves=curves, attn_stats=attn_stats, listen_stats=listen_stats, value_stats=value_stats, baselines=baselines,
                  discount=discount, ci=ci, n_boot=n_boot, boot_seed=boot_seed, contrast=contrast)


def sweep_layout(B, K, C, env_id_offset=0, paired=True):
    """The env layout of eval_sweep: B envs = K policies x C conditions x E envs, env b = (k*C + c)*E + e playing policy k under
    condition c.  -> (condition_of [B], rng_ids [B]), int64 numpy.  paired: rng_id = env_id_offset + e - every (policy,
    condition) cell sees the same spawns, prey moves and channel uniforms; else env_id_offset + b (every env its own stream)."""
    B, K, C = int(B), int(K), int(C)
    if K < 1 or C < 1 or B < 1 or B % (K * C):
        raise ValueError(f"sweep_layout: {B} envs do not split evenly between {K} policies x {C} conditions")
    E = B // (K * C)
    b = np.arange(B, dtype=np.int64)
    return (b // E) % C, int(env_id_offset) + (b % E if paired else b)


def eval_sweep(env, policies, itr=None, n_eval_episodes=100, max_env_steps=200, eval_greedy=True, paired=True, flag=None,
               episodes=False, comm_stats=False, curves=False, attn_stats=False, ci=None, n_boot=2000, boot_seed=0,
               contrast=None, listen_stats=False, value_stats=False, baselines=None, discount=0.99):
    """eval_summary over a grid of checkpoints x comm conditions in ONE rollout: `env` is a wrapper built with a list of C
    conditions (envs.GridEnvBatch(conditions=...): the points of a --teRcom / --tepl / --Pgb / --Pbg curve), `policies` one
    policy, a list or a nets.PolicySet (K policies).  The call lays the B = K*C*E envs out itself (sweep_layout; B % (K*C) != 0
    is refused) and leaves that layout on the wrapper.  Policy k's envs are one contiguous range, so the engine is eval_summary's
    (groups of C*E envs); behind every round ONE cm_episode_stats launch with groups of E envs fills a device table
    [K*C, n_eval_episodes, 9], ONE cm_episode_means launch reduces it, and [K*C, 12] doubles are the only copy to the host.
    -> a [K][C] list (a [C] list for a single policy) of eval_summary's dicts, each with `condition` (the dict given) added.
    Cell (k, c) holds exactly what eval_summary(W_c, policies[k]) returns for W_c a fresh wrapper of env's class, seed and
    channel kind whose params carry condition c, with E envs - at env's env_id_offset when paired (under greedy evaluation the
    points of a curve then differ only through the condition), at the cell's first env otherwise.
    flag, episodes, comm_stats, the refusals and env.eval_n_epi are eval_summary's; env.last_eval_average_reward is a [K][C] list
    ([C] for a single policy).  The five switches are eval_summary's, with its launches per round and at the end (the reductions
    with groups of E envs) and K*C cells in place of K policies in every table; their doubles ride in the same copy.
    comm_stats=True: every cell carries eval_summary's communication keys - a robustness curve can then be plotted against what
    was delivered (delivery, reach), not only against the knob that was turned.
    curves=True: every cell carries eval_summary's `curves` - when a lossy channel starts to hurt, and whether delivery collapses
    as the team spreads out, step by step.
    attn_stats=True: every cell carries eval_summary's ATTN_KEYS - how much attention mass a condition strands on dead links and
    how far the weights the hops really use concentrate: what explains the curve that delivery and reach only describe.
    listen_stats=True: every cell carries eval_summary's LISTEN_KEYS - whether a condition changed any decision; a cell that
    loses nothing has loss_* exactly 0.
    value_stats=True, baselines= (one critic per policy): every cell carries eval_summary's VALUE_KEYS - whether the baseline
    stays good at the lossy end of the curve and what it believes the loss costs; a cell that loses nothing has loss_value
    exactly 0.
    ci=level, n_boot=, boot_seed=: every cell carries eval_summary's `ci` and `se` - the error bars of the curve.  All cells are
    resampled by the same index stream.
    contrast=dict(condition=c0) or dict(policy=k0) (needs ci and paired=True): cell (k, c) is compared with cell (k, c0), or with
    (k0, c).  Paired, row e of every cell is the same scenario - the same Philox env id, every round reset at the same rng_step -
    so the difference of two cells is resampled over the SAME episodes in both, which removes the scenario-to-scenario variance
    from it: "is checkpoint 7 better than checkpoint 5 at pl = 0.3" and "does delivery differ between these two ranges" are what
    it answers.  Every dict gains `contrast`: name -> dict(diff=, lo=, hi=, se=, p_gt=) over the names of `ci` - diff the
    difference of the two point estimates, (lo, hi) and se the interval and standard error of the resampled difference, p_gt the
    share of resamples in which this cell's value is above the other's (ties half; near 0 or 1: the sign of diff is settled) - and
    `contrast_ref` = (k, c) of the cell compared with.  A cell compared with itself holds exact zeros and p_gt = 0.5.  It costs
    ONE more cm_boot_quantiles launch per table.  contrast without ci, with paired=False, with both or neither key or an index
    out of range raises ValueError before anything is built."""
    conds = getattr(env, "env", env).batch.conditions
    if conds is None:
        raise ValueError("eval_sweep: the wrapper was built without conditions= (eval_summary scores a uniform wrapper)")
    return _score("eval_sweep", env, policies, n_eval_episodes, max_env_steps, eval_greedy, flag, episodes, comm_stats,
                  conds=conds, paired=paired, curves=curves, attn_stats=attn_stats, listen_stats=listen_stats,
                  value_stats=value_stats, baselines=baselines, discount=discount, ci=ci, n_boot=n_boot, boot_seed=boot_seed,
                  contrast=contrast)


def summary_row(summary):
    """One eval_summary dict -> [success] + the VECTORS means: the list exp_runners/testing.py:329 writes between the epoch
    columns and the time stamp of a checkpoint's CSV row."""
    return [summary["success"]] + [summary[vec] for vec in VECTORS]


def eval_models_co(env, policies, itr=None, **kwargs):
    """eval_models with eval_model_co's contract: the fourth value of each tuple is the per-episode list of
    ``env.bound_return``."""
    return [out if out[0] is None else (out[0], out[1], out[2], [out[3]] * len(out[0]))
            for out in eval_models(env, policies, itr, **kwargs)]


def eval_model_co(env, policy, itr, **kwargs):
    """exp_runners/coverage/eval_co.py:9-101: same loop; the fourth return value is the per-episode
    list of ``env.bound_return`` (``epi_optRew``) instead of the scalar."""
    out = eval_model(env, policy, itr, **kwargs)
    if out[0] is None:
        return out
    return out[0], out[1], out[2], [out[3]] * len(out[0])


def eval_simple(args, env, algo, _eval=eval_model):
    """exp_runners/predatorprey/eval_pp.py:107-157 (`--mode eval`): ``args.n_eval_episodes`` episodes of at most
    ``args.max_env_steps`` steps with the algo's policy, printing the average length of the episodes that ended
    before the step limit.  The reference's loop exists to drive ``env.my_render`` (UI, out of scope): with
    ``args.render`` set this raises, otherwise the episodes are played as one batched device rollout (eval_model)."""
    import time
    start = time.time()
    data, _succ, _rew, _bound = _eval(env, algo.policy, 0, n_eval_episodes=args.n_eval_episodes,
                                      max_env_steps=args.max_env_steps, eval_greedy=bool(args.eval_greedy),
                                      render=bool(getattr(args, "render", False)),
                                      inspect_steps=bool(getattr(args, "inspect_steps", False)))
    traj_len = [len(step_success) for step_success, _ in data if len(step_success) < args.max_env_steps]
    print('Average trajectory length = {}'.format(np.mean(traj_len) if traj_len else float('nan')))
    print(f'test_time: {time.time() - start}')
    return traj_len


def eval_simple_co(args, env, algo):
    """exp_runners/coverage/eval_co.py:104-150: the same loop on the coverage env."""
    return eval_simple(args, env, algo, _eval=eval_model_co)
