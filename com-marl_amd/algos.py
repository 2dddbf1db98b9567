"""CentralizedMAPPO - the PPO update of com_marl/torch/algos/centralized_ma_ppo.py:39-659 with
the trajectory resident in HBM.

Same ctor kwargs and the same numbers:
returns f64 recurrence -> f32, GAE over the padded length with V of padded steps as the critic
outputs them, per-path advantage normalisation (biased variance, eps 1e-8), clip range fixed at
0.1, entropy bonus, mean over valid steps, Gaussian-NLL critic loss over padded steps, grad-clip
on the policy only, two Adam optimisers (lr 3e-4, eps 1e-5), minibatches over shuffled paths.

What changed is where it runs: the padded [P,T,...] batch is gathered on the device from the
sampler's time-major buffers; returns / GAE / normalisation are HIP scan kernels
(cm_discount_returns, cm_gae); critic baselines, old-policy log-likelihoods and the KL/entropy
diagnostics are fused no-grad launches; the training forward shares ONE trunk evaluation for the
entropy and the new log-likelihood (the reference runs it twice); multi-GPU adds one RCCL
all-reduce of the flat (policy ‖ critic ‖ counts) gradient bucket per optimiser step.
"""
import collections
import contextlib
import copy
import functools
import os
import time

import numpy as np
import torch
import torch.nn.functional as F
from torch.distributions import Categorical

from . import _lib as L
from . import deterministic
from .optim import Adam as FusedAdam
from .sampler import CentralizedMAOnPolicyVectorizedSampler, PathBatch, SegmentBatch, tabular


class _SurrogateFn(torch.autograd.Function):
    """-(sum over valid steps of the clipped surrogate + entropy bonus) from the policy logits in one launch
    (cm_ppo_surrogate: the ~30 elementwise / reduction launches of :390-438 + :540-589 and as many again in their
    autograd); the gradient wrt the logits is produced by the same launch.  Returns (total f32, count int64).
    add_entropy: the CM_ENT_* bits of include/commarl.h (0 / 1 = no term / the plain term)."""

    @staticmethod
    def forward(ctx, logits, actions, old_ll, adv, valids, clip, ent_coeff, add_entropy):
        P, T, N, A = logits.shape
        dev = logits.device
        lg = logits.contiguous()
        need = logits.requires_grad
        dl = torch.empty_like(lg) if need else None
        total = torch.empty((), dtype=torch.float64, device=dev)
        count = torch.empty((), dtype=torch.int64, device=dev)
        # (deterministic mode: block sums summed in a fixed order, no f64 atomics)
        L.launch("cm_ppo_surrogate", (P, T, N, A, L.ptr(lg), L.cptr(actions), L.cptr(old_ll), L.cptr(adv), L.ptr(valids), float(clip),
                                      float(ent_coeff), int(add_entropy), L.ptr(total), L.ptr(count), L.ptr(dl)), (P, T), device=dev)
        ctx.dl = dl
        ctx.mark_non_differentiable(count)
        return total.to(torch.float32), count

    @staticmethod
    def backward(ctx, g_total, _g_count):
        dl, ctx.dl = ctx.dl, None
        return (dl.mul_(g_total),) + (None,) * 7


def _fused_loss_ok(policy, obs, avail_actions, actions, valids):
    return (obs.is_cuda and avail_actions is None and hasattr(policy, "_logits") and policy._action_dim <= 8
            and actions.dtype == torch.int32 and valids.dtype == torch.int32 and os.environ.get("COMMARL_FUSED_LOSS", "1") != "0")


def _is_fused_adam(opt):
    """com_marl_amd.optim.Adam, or an optimiser of any class that offers the same: the clip folded into step(max_norm=...) and
    the device-step mode the update graphs and the KL stop are built on.  torch.optim.Adam is not one."""
    return hasattr(opt, "begin_device_steps")


@contextlib.contextmanager
def _torch_deterministic():
    """Deterministic update mode: the framework / library operations of the update (the input-gradient GEMMs of nets._LinearFn and
    _MatmulWFn, the wide first layers, the layer-by-layer path) with torch's deterministic setting on - the library GEMMs then
    take no atomic split-K kernels - and no NaN fill of every torch.empty (nothing here reads one unwritten); the caller's three
    settings come back afterwards."""
    import torch.utils.deterministic as tud
    was = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(), tud.fill_uninitialized_memory
    torch.use_deterministic_algorithms(True, warn_only=True)
    tud.fill_uninitialized_memory = False
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(was[0], warn_only=was[1])
        tud.fill_uninitialized_memory = was[2]


# One minibatch: its paths' rows of process_samples' tensors (None where the batch has none), of the epoch's advantages and old
# log-likelihoods, and n_crit, the critic's count of padded steps (device scalar): to _UpdateGraphs the tuple of a step's inputs.
_Minibatch = collections.namedtuple("_Minibatch", "obs actions rewards valids baselines dist_adjs channels advantages old_ll returns n_crit")


class _UpdateGraphs:
    """hipGraphs of the optimiser steps of train_once: the reference walks the SAME minibatches in each of its mini-epochs
    (centralized_ma_ppo.py:209-268: one permutation per epoch), so a minibatch's step is the same ~70 launches on the same
    buffers every time - only the weights, the Adam moments and the step number differ, and those live in device memory
    (optim.Adam.begin_device_steps).  The first mini-epoch of a process goes eagerly (first-use set-up inside the library,
    Adam's moments); after that a minibatch's step is captured the first time it comes up and every later step is one graph
    launch.  The graphs outlive the epoch: a later epoch whose minibatch i has the same shapes (the usual case at a fixed
    number of envs and path length) copies its tensors into the captured step's input buffers and replays - no capture at
    all (a capture costs as much host time as ~5 replayed steps).  For small batches the step is launch-bound (~3 ms of
    host work per eager step at the reference's 30 000 agent-steps per epoch); large batches keep the eager path
    (COMMARL_UPDATE_GRAPH=1 forces the graphs, =0 disables them; the default threshold is in agent rows per minibatch).
    Bookkeeping: at its first replayed or captured step it puts into the device-step mode those of the two optimisers that are
    not in it yet (under target_kl _run_steps has armed the policy's, behind the gate), and close() books the replayed steps
    into exactly those; _run_steps closes it, whatever happened."""
    MAX_ROWS = 1 << 18
    MAX_CACHED = 12

    @classmethod
    def maybe(cls, algo, minibatches, T, distributed):
        mode = os.environ.get("COMMARL_UPDATE_GRAPH", "auto")
        E = algo._optimization_mini_epochs
        obs = minibatches[0].obs
        if (mode == "0" or distributed or not obs.is_cuda or E < 3
                or not all(_is_fused_adam(o) for o in (algo._optimizer, algo._baseline_optimizer))
                or E * len(minibatches) > algo._optimizer.DEV_STEP_CAPACITY
                or not _fused_loss_ok(algo.policy, obs, None, minibatches[0].actions, minibatches[0].valids)   # (the framework's Categorical
                or not all(getattr(n, "_graph_capturable_update", False) for n in (algo.policy, algo.baseline))):   # validates on the host)
            return None                                      # only the nets whose whole step is this library's launches (CommBaseNet)
        rows = max(mb.obs.shape[0] for mb in minibatches) * T * getattr(algo.policy, "_n_agents", 1)
        if mode != "1" and rows > cls.MAX_ROWS:
            return None
        self = getattr(algo, "_update_graphs", None)
        owner = (id(algo.policy), id(algo.baseline), id(algo._optimizer), id(algo._baseline_optimizer),
                 next(algo.policy.parameters()).data_ptr(), next(algo.baseline.parameters()).data_ptr(), obs.device)
        if self is None or self.owner != owner:
            self = algo._update_graphs = cls(algo, owner)
        # the first optimiser steps of a process go eagerly (first-use set-up inside the library, Adam's moment buffers and norm
        # workspace); from then on a step is replayed (or captured) from mini-epoch 0
        first = 0 if getattr(algo, "_eager_stepped", False) else 1
        self._begin(len(minibatches), (E - first) * len(minibatches), first)
        # what a captured step has baked in besides its tensors: part of the cache key
        grp = lambda o: tuple((g["lr"], tuple(g["betas"]), g["eps"]) for g in o.param_groups)   # noqa: E731
        self.hyper = (T, grp(algo._optimizer), grp(algo._baseline_optimizer), algo._lr_clip_range, algo._policy_ent_coeff,
                      algo._entropy_method, algo._use_softplus_entropy, algo._stop_entropy_gradient, algo._positive_adv,
                      algo._clip_grad_norm, os.environ.get("COMMARL_CRITIC_STREAM", "1"), deterministic(),
                      algo._update_stats, algo._target_kl)   # (the stop threshold is an argument of the captured statistics launch)
        return self

    def __init__(self, algo, owner):
        self.algo, self.owner = algo, owner
        self.cache = collections.OrderedDict()               # (minibatch index, shapes) -> [graph, output, input tensors]
        self.pool, self.stream = None, None
        self.cur, self.done, self.n_steps, self.first_epoch = [], 0, 0, 1
        self.armed, self.broken, self.hyper = None, False, None   # armed: the optimisers this epoch's steps put into device-step mode
        self.captured = self.reused = 0                       # (counters: captures taken / earlier epochs' graphs taken over)

    def _begin(self, n_mb, n_steps, first_epoch):
        self.cur, self.done, self.n_steps, self.first_epoch = [None] * n_mb, 0, n_steps, first_epoch
        self.armed, self.broken = None, False

    def _key(self, i, inputs):
        return (i, self.hyper) + tuple(None if t is None else (tuple(t.shape), t.dtype) for t in inputs)

    def step(self, i, inputs, fn):
        """Step of minibatch i on `inputs` (the tuple of its tensors: fn(inputs) issues the step): replayed from its graph -> the step's
        gradient-norm output.  First time this epoch: the graph of an earlier epoch with the same shapes gets the tensors copied
        into its input buffers, else the step is captured with these tensors as its input buffers.  A capture that fails
        switches the rest of the epoch back to eager steps."""
        if self.broken:
            return fn(inputs)
        if self.armed is None:                               # the moments exist, the step counts are known
            self.armed = [o for o in (self.algo._optimizer, self.algo._baseline_optimizer) if o._dev_steps is None]
            for o in self.armed:
                o.begin_device_steps(self.n_steps)
        if self.cur[i] is None:
            key = self._key(i, inputs)
            ent = self.cache.get(key)
            if ent is not None:
                with torch.no_grad():
                    for dst, src in zip(ent[2], inputs):
                        if dst is not None and dst.data_ptr() != src.data_ptr():
                            dst.copy_(src)
                self.cache.move_to_end(key)
                self.reused += 1
            else:
                try:
                    g, out = self._capture(lambda: fn(inputs))
                except Exception as e:                       # noqa: BLE001 - whatever the capture tripped over, the step itself is fine
                    import warnings
                    warnings.warn(f"PPO update: hipGraph capture of the optimiser step failed ({type(e).__name__}: {e}); eager steps from here")
                    torch.cuda.synchronize()
                    self.close()
                    self.broken = True
                    return fn(inputs)
                ent = self.cache[key] = [g, out, list(inputs)]
                self.captured += 1
                while len(self.cache) > self.MAX_CACHED:
                    self.cache.popitem(last=False)
            self.cur[i] = ent
        g, out = self.cur[i][0], self.cur[i][1]
        g.replay()
        self.done += 1
        return out

    def _capture(self, fn):
        # capture_begin / capture_end directly: torch.cuda.graph() would synchronise the device and empty the allocator's cache
        # in front of every capture
        g = torch.cuda.CUDAGraph()
        cur = torch.cuda.current_stream()
        if self.stream is None:
            self.stream = torch.cuda.Stream(device=cur.device)
        self.stream.wait_stream(cur)
        # a capture freezes the host's decisions: the weight-pack cache must not answer "fresh" (it would, right after the
        # epoch's no-grad forward) - the replays run after optimiser steps the host-side version counters never saw
        for net in (self.algo.policy, self.algo.baseline):
            if hasattr(net, "_pack_sig"):
                net._pack_sig = None
        with L.capture_guard(), torch.cuda.stream(self.stream):
            kw = {} if self.pool is None else dict(pool=self.pool)
            g.capture_begin(capture_error_mode="thread_local", **kw)
            try:
                out = fn()
            finally:
                g.capture_end()
        cur.wait_stream(self.stream)
        if self.pool is None:
            self.pool = g.pool()
        return g, out

    def close(self):
        """Book the epoch's replayed steps into the host state of the optimisers armed here (idempotent); the graphs stay for
        later epochs."""
        for o in self.armed or ():
            o.end_device_steps(self.done)
        self.armed, self.done = None, 0
        self.cur = [None] * len(self.cur)


class _UpdateStats:
    """The per-step update statistics and the KL early stop (update_stats / target_kl; csrc/cm_ppo_stats.hip), all of it that
    is not PPO: the switches, the refusals, the launch, the row collection and the summary stats.  An instance is the device
    side - row table, row cursor, gate and workspace, allocated once per device (a step captured in one epoch replays in later
    ones on the same addresses) - and lives as algo._upd_state: made by the first arm(), so there is none while both switches
    are off, and left out of the algo's pickle."""

    @staticmethod
    def resolve(update_stats, target_kl):
        """-> (update_stats: bool, target_kl: float or None) from the ctor's arguments and their environment fall-backs."""
        if update_stats is None:
            update_stats = os.environ.get("COMMARL_UPDATE_STATS", "") == "1"
        if target_kl is None and os.environ.get("COMMARL_TARGET_KL", "") != "":
            target_kl = os.environ["COMMARL_TARGET_KL"]
        if target_kl is not None:
            try:
                target_kl = float(target_kl)
            except (TypeError, ValueError):
                raise ValueError(f"target_kl must be a finite float > 0, got {target_kl!r}") from None
            if not (np.isfinite(target_kl) and target_kl > 0):
                raise ValueError(f"target_kl must be a finite float > 0, got {target_kl!r}")
        return bool(update_stats) or target_kl is not None, target_kl

    @classmethod
    def arm(cls, algo, minibatches, distributed):
        """What the statistics and the stop need, each refusal with its reason; then the device side for this epoch's
        `n_steps` scheduled optimiser steps, its row cursor at 0 and its gate open (outside any graph)."""
        what = "target_kl" if algo._target_kl is not None else "update_stats"
        mb = minibatches[0]
        if algo._target_kl is not None and distributed:
            raise NotImplementedError("target_kl in a distributed update: the ranks would have to agree on the gate "
                                      "(update_stats alone is allowed, with rank-local rows)")
        if not _fused_loss_ok(algo.policy, mb.obs, None, mb.actions, mb.valids):
            raise L.CommarlError(f"{what} needs the fused PPO loss (a CUDA batch, a policy with _logits and at most 8 actions, "
                                 "COMMARL_FUSED_LOSS not 0): the statistics are taken from the logits that loss runs on")
        if not _is_fused_adam(algo._optimizer):
            raise L.CommarlError(f"{what} needs com_marl_amd.optim.Adam as the policy's optimiser (its device-side step), "
                                 f"not {type(algo._optimizer).__name__}")
        n = algo._optimization_mini_epochs * len(minibatches)
        if n > FusedAdam.DEV_STEP_CAPACITY:
            raise L.CommarlError(f"{what}: {algo._optimization_mini_epochs} mini-epochs x {len(minibatches)} minibatches = {n} optimiser "
                                 f"steps per epoch, the row table holds optim.Adam.DEV_STEP_CAPACITY = {FusedAdam.DEV_STEP_CAPACITY}")
        self = getattr(algo, "_upd_state", None)
        if self is None or self.rows.device != mb.obs.device:
            self = algo._upd_state = cls(mb.obs.device)
        self.n_steps, self.n_minibatches = n, len(minibatches)
        self.cursor.zero_()
        self.gate.zero_()
        return self

    def __init__(self, dev):
        self.ws_bytes = int(L.lib().cm_ppo_update_stats_ws_bytes(1 << 16, 1))       # the largest grid's
        self.rows = torch.zeros(FusedAdam.DEV_STEP_CAPACITY, L.UPD_COLS, dtype=torch.float64, device=dev)
        self.cursor = torch.zeros(1, dtype=torch.int32, device=dev)
        self.gate = torch.zeros(1, dtype=torch.int32, device=dev)
        self.ws = torch.empty(self.ws_bytes // 8, dtype=torch.float64, device=dev)

    def launch(self, algo, logits, mb):
        """cm_ppo_update_stats on the step's logits: the row of the step about to be taken and, under target_kl, the gate the
        policy's Adam obeys.  Two small launches on the current (the policy's) stream, part of a captured step."""
        P, T, N, A = logits.shape
        gated = algo._target_kl is not None
        L.run("cm_ppo_update_stats", P, T, N, A, L.cptr(logits), L.cptr(mb.actions), L.cptr(mb.old_ll), L.ptr(mb.valids),
              float(algo._lr_clip_range), 1.5 * algo._target_kl if gated else 0.0, L.ptr(self.rows), self.rows.shape[0],
              L.ptr(self.cursor), L.ptr(self.gate) if gated else None, L.ptr(self.ws), self.ws_bytes, device=logits.device)

    def collect(self):
        """After the epoch's synchronise: the row table to the host (one copy) -> (update_rows, the number of applied policy
        steps, the PolicySteps / ApproxKL / ClipFraction stats)."""
        rows = self.rows[:self.n_steps].cpu().numpy()
        n_rows = min(int(self.cursor.item()), self.n_steps)              # (fewer than scheduled only if the steps were cut short)
        rows = rows[:n_rows]
        out = {name: rows[:, c].copy() for c, name in enumerate(L.UPD_COLUMNS)}
        k = np.arange(n_rows)
        out["mini_epoch"], out["minibatch"] = k // self.n_minibatches, k % self.n_minibatches
        went = out["stopped"] == 0
        applied = int(went.sum())
        return out, applied, dict(PolicySteps=applied, ApproxKL=float(out["approx_kl"].max()) if n_rows else 0.0,
                                  ClipFraction=float(out["clip_frac"][went].mean()) if applied else 0.0)


def _resolve_segment_steps(segment_steps):
    """-> segment_steps: None (off) or an int >= 1, from the ctor's argument and its environment fall-back."""
    if segment_steps is None:
        segment_steps = os.environ.get("COMMARL_SEGMENT_STEPS", "") or None
        if segment_steps is None:
            return None
    bad = ValueError(f"segment_steps must be an integer >= 1, got {segment_steps!r}")
    if isinstance(segment_steps, bool) or not isinstance(segment_steps, (int, np.integer, str)):
        raise bad                                            # (a float is refused even when it is whole: 8.0 is a typo for 8)
    try:
        n = int(segment_steps)
    except ValueError:
        raise bad from None
    if n < 1:
        raise bad
    return n


class CentralizedMAPPO:
    _update_stats, _target_kl, update_rows = False, None, None      # (an algo pickled before these switches existed: off)
    _segment_steps = None

    def __init__(self, env_spec, policy, baseline, optimizer=None, baseline_optimizer=None,
                 optimization_n_minibatches=1, optimization_mini_epochs=1, policy_lr=3e-4, lr_clip_range=2e-1,
                 max_path_length=500, num_train_per_epoch=1, discount=0.99, gae_lambda=1, center_adv=True,
                 positive_adv=False, policy_ent_coeff=0.0, use_softplus_entropy=False, stop_entropy_gradient=False,
                 entropy_method='no_entropy', clip_grad_norm=None, device='cpu', update_stats=None, target_kl=None,
                 segment_steps=None):
        """update_stats / target_kl (both opt-in, not in the reference): per-step statistics of the policy update (`update_rows`,
        and the PolicySteps / ApproxKL / ClipFraction stats) and the KL early stop on top of them.  With target_kl set, the
        first optimiser step of an epoch in front of which the approximate KL (k3, mean of (r - 1) - log r over the minibatch's
        valid steps) exceeds kl_stop = 1.5 * target_kl - the factor Spinning Up and Stable-Baselines3 use - is not applied to the
        policy, and none after it; the critic keeps taking every scheduled step.  The decision is taken and obeyed on the
        device (cm_ppo_update_stats, cm_multi_adam_step_gated).  target_kl implies update_stats.  None falls back to
        COMMARL_UPDATE_STATS (1 = on) / COMMARL_TARGET_KL (a float), so the reference's unmodified runners can switch it on.

        segment_steps (opt-in, not in the reference; None falls back to COMMARL_SEGMENT_STEPS): an integer n >= 1 trains on
        fixed-length rollout segments instead of whole episodes.  The sampler's obtain_samples then answers with
        obtain_segments(itr, n): every env runs n more steps per epoch, without a reset in between, and train_once takes the
        SegmentBatch with P = n_envs, T = n, valids = n.  Episode ends inside a segment cut the return and GAE scans, the
        cut at the segment's end is bootstrapped from the critic's value of the state behind it (cm_segment_targets); the time
        limit is a terminal state like any other end, as in the reference.  center_adv then means ONE normalisation over the
        whole batch per epoch (cm_adv_normalize; biased variance, eps 1e-8) - the reference's per-path normalisation has no
        meaning for fragments of episodes.  The progress columns come from the episodes that ended in the segment (NaN means and
        NumTrajs 0 when none did).  positive_adv, update_stats, target_kl, the deterministic mode and the entropy methods
        'no_entropy' and 'regularized' work as on whole paths; entropy_method='max' (its per-minibatch cm_entropy_gae has no
        done-aware form) and a distributed update (the batch-wide moments would have to be reduced over the ranks) are refused
        with NotImplementedError."""
        self._update_stats, self._target_kl = _UpdateStats.resolve(update_stats, target_kl)
        self._segment_steps = _resolve_segment_steps(segment_steps)
        if self._segment_steps is not None and entropy_method == 'max':
            raise NotImplementedError(self._SEGMENTS_MAXENT)
        self.update_rows = None
        self.device = device
        self.env_spec, self.policy, self.baseline = env_spec, policy, baseline
        self.discount, self.max_path_length, self.n_samples = discount, max_path_length, num_train_per_epoch
        self._gae_lambda, self._center_adv, self._positive_adv = gae_lambda, center_adv, positive_adv
        self._policy_ent_coeff = policy_ent_coeff
        self._use_softplus_entropy, self._stop_entropy_gradient = use_softplus_entropy, stop_entropy_gradient
        self._entropy_method = entropy_method
        self._lr_clip_range = 0.1                       # hard-coded in the reference (:115); ctor arg ignored
        self._eps = 1e-8
        self._maximum_entropy = entropy_method == 'max'
        self._entropy_regularzied = entropy_method == 'regularized'
        self._check_entropy_configuration(entropy_method, center_adv, stop_entropy_gradient, policy_ent_coeff)
        # default: the multi-tensor Adam of optim.py (two launches per step, clip folded in); it and torch.optim.Adam are
        # the same update as the vendored torch-1.9 Adam (my_optimizer/_functional.py:72-98): pinned by tests against the
        # reference's optimiser.
        on_gpu = next(policy.parameters()).is_cuda
        opt = optimizer or (FusedAdam if on_gpu else torch.optim.Adam)
        bopt = baseline_optimizer or (FusedAdam if on_gpu else torch.optim.Adam)
        self._optimizer = opt(policy.parameters(), lr=policy_lr, eps=1e-5)
        self._baseline_optimizer = bopt(baseline.parameters(), lr=policy_lr, eps=1e-5)
        self._optimization_n_minibatches = optimization_n_minibatches
        self._optimization_mini_epochs = optimization_mini_epochs
        self._clip_grad_norm = clip_grad_norm
        self._old_policy = copy.deepcopy(self.policy)
        self._old_policy._pack_sig, self._old_policy._pack = None, None
        self.sampler_cls = CentralizedMAOnPolicyVectorizedSampler
        self.episode_reward_mean = collections.deque(maxlen=100)
        self.stats = {}

    _SEGMENTS_MAXENT = ("rollout segments with entropy_method='max': its per-minibatch cm_entropy_gae recomputes the advantages "
                        "from the padded rows and has no done-aware form")

    def __getstate__(self):
        """Snapshots pickle the algo (snapshotter.py:102-104); a HIP stream is not picklable and is re-made on first use."""
        st = dict(self.__dict__)
        st.pop("_side_stream", None)
        st.pop("_bucket", None)
        st.pop("_eager_stepped", None)                   # per process: the first optimiser steps of a process run eagerly
        st.pop("_update_graphs", None)                   # hipGraphs of optimiser steps (rebuilt on demand)
        st.pop("_upd_state", None)                       # device tables of the update statistics (re-made on first use)
        st.pop("_norm_ws", None)                         # cm_adv_normalize's workspace
        return st

    @staticmethod
    def _check_entropy_configuration(entropy_method, center_adv, stop_entropy_gradient, policy_ent_coeff):
        if entropy_method not in ('max', 'regularized', 'no_entropy'):
            raise ValueError('Invalid entropy_method')
        if entropy_method == 'max':
            if center_adv:
                raise ValueError('center_adv should be False when entropy_method is max')
            if not stop_entropy_gradient:
                raise ValueError('stop_gradient should be True when entropy_method is max')
        if entropy_method == 'no_entropy' and policy_ent_coeff != 0.0:
            raise ValueError('policy_ent_coeff should be zero when there is no entropy method')

    # ------------------------------------------------------------------------------------------
    # process_samples (:612-659)
    # ------------------------------------------------------------------------------------------
    def _dev(self):
        return next(self.policy.parameters()).device

    def process_samples(self, itr, paths):
        """-> (obs [P,T,N*d], avail (None = ones), actions [P,T,N], rewards [P,T] f32, valids [P] int32,
        baselines [P,T], returns [P,T], dist_adjs [P,T,N,N]|None, channels [P,T,L,N,N]|None), all on device.
        Zero padding for obs/actions/rewards/returns, ONE padding for the masks (App. A-5)."""
        dev = self._dev()
        if isinstance(paths, SegmentBatch):
            return self._process_segments(paths)
        if isinstance(paths, PathBatch):
            e = paths.engine
            P, T = paths.gather_index()[:2]
            obs = paths.padded("obs", 0).reshape(P, T, -1)
            actions = paths.padded("actions", 0)
            rew64 = paths.padded("reward64", 0)
            dist_adjs = None if e.dist_adj is None else paths.padded("dist_adj", 1)
            channels = None if e.channels is None else paths.padded("channels", 1)
            valids = paths.length.to(torch.int32)
        else:                                                                       # reference list-of-dicts
            P = len(paths)
            T = max(len(p['rewards']) for p in paths)
            N = self.policy._n_agents
            Lh = np.asarray(paths[0]['channels']).shape[-2] // N                    # [T, L*N, N] (sampler.py:191)

            def pad(key, val, dtype, tail):
                out = torch.full((P, T) + tail, val, dtype=dtype)
                for i, p in enumerate(paths):
                    a = torch.as_tensor(np.asarray(p[key])).to(dtype).reshape((-1,) + tail)
                    out[i, :a.shape[0]] = a
                return out.to(dev)
            obs = pad('observations', 0, torch.float32, (paths[0]['observations'].shape[-1],))
            actions = pad('actions', 0, torch.int32, (N,))
            rew64 = pad('rewards', 0, torch.float64, ())
            dist_adjs = pad('dist_adjs', 1, torch.float32, (N, N))
            channels = pad('channels', 1, torch.float32, (Lh, N, N))
            valids = torch.tensor([len(p['actions']) for p in paths], dtype=torch.int32, device=dev)
        self.temp_max_path_length = T
        rewards = rew64.to(torch.float32).contiguous()                              # torch.Tensor(path['rewards']) (:645)
        returns = torch.empty(P, T, dtype=torch.float32, device=dev)
        L.run("cm_discount_returns", P, T, L.cptr(rew64), L.ptr(valids), float(self.discount), L.ptr(returns), device=dev)
        with torch.no_grad():                                                       # :653-657
            baselines = self._baseline_forward(obs, dist_adjs, channels)
        return obs, None, actions, rewards, valids, baselines, returns, dist_adjs, channels

    def _process_segments(self, seg):
        """process_samples of a SegmentBatch: P = n_envs rows of T = n_steps steps, all valid.  The [P,T,...] tensors are
        transposed copies of the engine's time-major slots (the minibatches gather rows of them); rewards and dones are not
        copied for the targets: cm_segment_targets reads them where they are.  The raw advantages stay on the batch
        (seg.advantages) for _segment_advantages."""
        seg._check_fresh()
        e, n, P = seg.engine, seg.n_steps, seg.B
        rows = lambda b: None if b is None else b[:n].transpose(0, 1).contiguous()      # noqa: E731  ([n,B,...] -> [B,n,...])
        obs, actions = rows(e.obs).reshape(P, n, -1), rows(e.actions)
        dist_adjs, channels = rows(e.dist_adj), rows(e.channels)
        rewards = e.reward64[:n].to(torch.float32).t().contiguous()
        valids = torch.full((P,), n, dtype=torch.int32, device=obs.device)
        self.temp_max_path_length = n
        with torch.no_grad():
            baselines = self._baseline_forward(obs, dist_adjs, channels).contiguous()
            b_obs, b_adj, b_ch = seg.bootstrap()
            step = lambda x: None if x is None else x.unsqueeze(1)                       # noqa: E731  (a batch of one-step rows)
            v_last = self._baseline_forward(step(b_obs), step(b_adj), step(b_ch)).reshape(P).contiguous()
        adv, returns = torch.empty_like(baselines), torch.empty_like(baselines)
        L.run("cm_segment_targets", P, n, L.ptr(e.reward64), L.ptr(e.done), 1, P, L.ptr(baselines), L.ptr(v_last),
              float(self.discount), float(self._gae_lambda), L.ptr(adv), L.ptr(returns), device=obs.device)
        seg.advantages, seg.v_last = adv, v_last
        return obs, None, actions, rewards, valids, baselines, returns, dist_adjs, channels

    def _segment_advantages(self, seg):
        """The epoch's advantages of a SegmentBatch: cm_segment_targets' (left on the batch by process_samples), under center_adv
        normalised ONCE over the whole batch (cm_adv_normalize), then positive_adv."""
        adv = seg.advantages.clone()
        if self._center_adv:
            nb = int(L.lib().cm_adv_normalize_ws_bytes())
            ws = getattr(self, "_norm_ws", None)
            if ws is None or ws.device != adv.device:
                ws = self._norm_ws = torch.empty(nb // 8, dtype=torch.float64, device=adv.device)
            L.run("cm_adv_normalize", adv.numel(), L.ptr(adv), self._eps, L.ptr(ws), nb, device=adv.device)
        return self._positive(adv)

    # baseline dispatch (:230-233, :654-657): the GNN critic takes the graph, plain baselines only obs
    def _baseline_forward(self, obs, dist_adjs, channels):
        if self.baseline.name in ['base_critic']:
            return self.baseline.forward(obs, None, dist_adjs, channels)
        return self.baseline.forward(obs)

    def _baseline_loss(self, obs, returns, dist_adjs, channels):
        if self.baseline.name in ['base_critic']:
            return self.baseline.compute_loss(obs, returns, dist_adjs, channels)
        return self.baseline.compute_loss(obs, returns)

    # ------------------------------------------------------------------------------------------
    # loss pieces
    # ------------------------------------------------------------------------------------------
    def _advantages(self, rewards, baselines, valids):
        """compute_advantages + per-path normalisation (:418-426) in one scan kernel."""
        P, T = rewards.shape
        adv = torch.empty_like(rewards)
        L.run("cm_gae", P, T, L.cptr(rewards), L.cptr(baselines), L.ptr(valids), float(self.discount), float(self._gae_lambda),
              int(self._center_adv), self._eps, L.ptr(adv), device=rewards.device)
        return self._positive(adv)

    def _positive(self, adv):                                  # positive_adv (:428-429): minus the min of this call's advantages
        return adv - adv.min() if self._positive_adv else adv

    def _max_entropy_advantages(self, logits, rewards, baselines, in_place):
        """entropy_method 'max' (:415-418): r' = r + c * H of the current policy, then compute_advantages, in one
        cm_entropy_gae launch on the detached logits [P,T,N,A] (the entropy carries no gradient in this mode: the ctor
        demands stop_entropy_gradient).  in_place writes r' back into `rewards`, as the reference's `rewards +=` does to the
        epoch's full-batch tensor (the two quirks of the in-place add); a minibatch step leaves its rewards
        buffer alone (the reference adds to a copy, and a replayed update graph would add c * H again every mini-epoch)."""
        P, T = rewards.shape
        N, A = logits.shape[-2:]
        lg = logits.detach().contiguous()
        adv = torch.empty_like(rewards)
        L.run("cm_entropy_gae", P, T, N, A, L.ptr(lg), L.ptr(rewards), L.cptr(baselines), float(self.discount),
              float(self._gae_lambda), float(self._policy_ent_coeff), int(self._use_softplus_entropy),
              L.ptr(rewards) if in_place else None, None, L.ptr(adv), device=rewards.device)
        return self._positive(adv)

    def _entropy_flags(self):
        """cm_ppo_surrogate's add_entropy bits: the 'regularized' term and its two switches (:434-435, :509-536)."""
        if not self._entropy_regularzied:
            return 0
        return (L.ENT_ADD | (L.ENT_SOFTPLUS if self._use_softplus_entropy else 0)
                | (L.ENT_STOP_GRAD if self._stop_entropy_gradient else 0))

    @torch.no_grad()
    def _act_probs(self, policy, obs, dist_adjs, channels):
        """Action probabilities [P,T,N,A] of `policy` over the padded batch from its act_device: one fused no-grad launch."""
        flat = lambda x: None if x is None else x.reshape(-1, *x.shape[2:])         # noqa: E731  ([P,T,...] -> [P*T,...])
        _, probs, _ = policy.act_device(flat(obs), None, flat(dist_adjs), flat(channels), want_actions=False, want_attn=False, policy_step=0)
        return probs.reshape(*obs.shape[:2], self.policy._n_agents, -1)

    def _evaluate(self, policy, obs, dist_adjs, channels):
        """One no-grad forward over the full batch -> (logits or None, probs [P,T,N,A]): the policy's evaluate_nograd, or, of a
        policy object without one, act_device's probabilities and no logits."""
        if hasattr(policy, "evaluate_nograd"):
            return policy.evaluate_nograd(obs, dist_adjs, channels)
        return None, self._act_probs(policy, obs, dist_adjs, channels)

    def _old_log_likelihood(self, obs, actions, dist_adjs, channels):
        """old_policy.log_likelihood (:561-566)."""
        return self._ll_from_probs(self._act_probs(self._old_policy, obs, dist_adjs, channels), actions)

    @staticmethod
    def _ll_from_probs(probs, actions):
        """log-likelihood of the taken joint action from action probabilities [P,T,N,A] -> [P,T] (:561-566)."""
        return torch.log(probs.gather(-1, actions.long().unsqueeze(-1))).squeeze(-1).sum(-1)

    def _kl_entropy(self, p_old, p_new):
        """KL(old || new) mean and the logged Entropy of `p_new` (:366), both over ALL padded steps (:440-538), from two
        probability tensors.  Entropy: the per-step entropy (mean over agents), softplus per step first when
        use_softplus_entropy is set (it goes through _compute_policy_entropy, :499-538)."""
        kl = (p_old * (torch.log(p_old) - torch.log(p_new))).sum(-1).mean()
        h = -(p_new * torch.log(p_new)).sum(-1).mean(-1)
        if self._use_softplus_entropy:
            h = F.softplus(h)
        return float(kl), float(h.mean())

    def _compute_loss(self, itr, obs, avail_actions, actions, rewards, valids, baselines, dist_adjs, channels,
                      advantages=None, old_ll=None, reduce=True, logits=None, rewards_in_place=False, logits_out=None):
        """:390-438.  Returns -(mean over valid steps of clipped surrogate + c * entropy); with
        reduce=False returns (sum, count) for the count-weighted multi-GPU reduction.
        entropy_method 'max' ignores `advantages`: they come from this call's entropy (_max_entropy_advantages), and
        rewards_in_place says whether r + c * H is written back into `rewards` (the full-batch calls of train_once).
        logits_out: a list that receives the detached logits the fused loss ran on (the update statistics judge the same ones)."""
        maxent = self._maximum_entropy
        if advantages is None and not maxent:
            advantages = self._advantages(rewards, baselines, valids)
        if old_ll is None:
            old_ll = self._old_log_likelihood(obs, actions, dist_adjs, channels)
        if _fused_loss_ok(self.policy, obs, avail_actions, actions, valids):
            if logits is None:
                logits = self.policy._logits(obs, dist_adjs, channels)               # [P,T,N,A]
            if logits_out is not None:
                logits_out.append(logits.detach())
            if maxent:
                advantages = self._max_entropy_advantages(logits, rewards, baselines, rewards_in_place)
            total, count = _SurrogateFn.apply(logits, actions, old_ll, advantages, valids, self._lr_clip_range,
                                              self._policy_ent_coeff, self._entropy_flags())
            return (total, count) if not reduce else total / count
        probs, _ = self.policy._probs(obs, avail_actions, dist_adjs, channels)      # one trunk pass for both terms
        dist_n = Categorical(probs=probs)
        entropies = dist_n.entropy().mean(-1)                                        # policy.entropy (:121-126)
        if self._stop_entropy_gradient:
            entropies = entropies.detach()                                           # (:509-514: under no_grad)
        if self._use_softplus_entropy:
            entropies = F.softplus(entropies)                                        # (:535-536)
        if maxent:                                                                   # :415-418
            c = self._policy_ent_coeff
            advantages = self._advantages(rewards.add_(c * entropies) if rewards_in_place else rewards + c * entropies,
                                          baselines, valids)
        new_ll = dist_n.log_prob(actions).sum(-1)                                    # policy.log_likelihood (:128-137)
        ratio = (new_ll - old_ll).exp()
        surrogate = ratio * advantages
        clipped = torch.clamp(ratio, min=1 - self._lr_clip_range, max=1 + self._lr_clip_range) * advantages
        objective = torch.min(surrogate, clipped)                                    # :540-589
        if self._entropy_regularzied:
            objective = objective + self._policy_ent_coeff * entropies               # :434-435
        mask = torch.arange(obs.shape[1], device=valids.device)[None, :] < valids[:, None]
        total, count = -(objective * mask).sum(), mask.sum()
        return (total, count) if not reduce else total / count

    def _log_performance(self, itr, paths, returns, valids):
        """The progress.csv columns of centralized_ma_ppo.py:286-366 (per-path sums -> means over paths).
        With a PathBatch everything is reduced on the device and one small vector comes to the host."""
        N = self.policy._n_agents
        if isinstance(paths, SegmentBatch):
            return self._log_segments(itr, paths)
        if isinstance(paths, PathBatch):
            e, dev, lens = paths.engine, self._dev(), paths.length
            P, T, valid, t_idx, b_idx = paths.gather_index()
            undisc = paths.padded("reward64", 0).sum(1)                              # np.sum(path_rewards), f64
            det = (e.details[t_idx, b_idx].to(torch.float64) * valid[..., None]).sum(1)   # [P,6]
            succ = e.success[paths.start + lens - 1, paths.env_idx].to(torch.float64)
            if e.dist_adj is not None:
                deg = (e.dist_adj[t_idx, b_idx].sum(-1).mean(-1).to(torch.float64) * valid).sum(1) / lens
                if e.diameter is not None:                                           # calc_diameter: the path's mean (:314-317)
                    diam = (e.diameter[t_idx, b_idx].to(torch.float64) * valid).sum(1) / lens
                else:
                    diam = torch.zeros(P, dtype=torch.float64, device=dev)           # get_graph: diameter 0 (:234)
            else:
                deg = torch.full((P,), float(N), dtype=torch.float64, device=dev)
                diam = deg.clone()
            pp = e.env.scenario == "pp"
            nA = float(N)
            cap = det[:, 0] if pp else det[:, 0] / nA
            pen = det[:, 2] if pp else det[:, 2] / nA
            var2 = torch.zeros_like(cap) if pp else det[:, 3] / nA
            cols = torch.stack([undisc, returns[:, 0].to(torch.float64), succ, cap, lens.to(torch.float64),
                                det[:, 1] / nA, pen, det[:, 4] / nA, var2, deg, diam])
            means = cols.mean(1).tolist()
            std, mx, mn = float(undisc.std(unbiased=False)), float(undisc.max()), float(undisc.min())
            trput = float(e.env.n_empty_cells if not pp else 0)
            undisc_list = undisc.tolist()
        else:
            def col(f):
                return [f(p) for p in paths]
            dsum = lambda k: col(lambda p: float(np.sum([d[k] for d in p['rewards_details']])))   # noqa: E731
            undisc_list = col(lambda p: float(np.sum(np.asarray(p['rewards']))))
            means = [np.mean(undisc_list), float(returns[:, 0].to(torch.float64).mean()),
                     np.mean(col(lambda p: np.mean(p['success']))), np.mean(dsum('capture_cnt')),
                     np.mean(dsum('step_cnt')), np.mean(dsum('move_cnt')), np.mean(dsum('penalty_cnt')),
                     np.mean(dsum('variable')), np.mean(dsum('vars2')),
                     np.mean(col(lambda p: np.mean(p['ave_degs']))), np.mean(col(lambda p: np.mean(p['diameters'])))]
            std, mx, mn = float(np.std(undisc_list)), float(np.max(undisc_list)), float(np.min(undisc_list))
            trput = float(np.mean(col(lambda p: np.mean(p['ave_trputs']))))
            P = len(paths)
        self.episode_reward_mean.extend(undisc_list)
        keys = ("AverageReturn", "AverageDiscountedReturn", "SuccessRate", "AverageCaptureCount", "AverageStepCount",
                "AverageMovingCount", "AveragePenaltyCount", "AverageVariable", "AverageVar2", "AveDegree", "Diameter")
        out = dict(Iteration=itr, NumTrajs=P * N)                                    # :346-347
        out.update({k: float(v) for k, v in zip(keys, means)})
        out.update(StdReturn=std, MaxReturn=mx, MinReturn=mn, AveTroughput=trput)
        return out

    def _log_segments(self, itr, seg):
        """_log_performance's columns for a SegmentBatch, from its episode table (cm_segment_episodes: the episodes that ENDED
        in the segment; one small host copy): means over those episodes, NaN where there is none (NumTrajs 0).  AveDegree and
        Diameter are means over the segment's steps."""
        e, N, n = seg.engine, self.policy._n_agents, seg.n_steps
        ep = seg.episodes
        cnt, nA, pp = ep["count"], float(N), e.env.scenario == "pp"
        nan = float("nan")
        mean = (lambda x: x / cnt) if cnt > 0 else (lambda x: nan)                        # noqa: E731
        avg = mean(ep["ret_sum"])
        if e.dist_adj is not None:
            deg = float(e.dist_adj[:n].sum(-1).mean(dtype=torch.float64))
            diam = float(e.diameter[:n].mean(dtype=torch.float64)) if e.diameter is not None else 0.0
        else:
            deg = diam = float(N)
        if cnt > 0:
            self.episode_reward_mean.append(avg)
        return dict(Iteration=itr, NumTrajs=int(cnt) * N, AverageReturn=avg, AverageDiscountedReturn=mean(ep["disc_sum"]),
                    SuccessRate=mean(ep["success"]), AverageCaptureCount=mean(ep["details_0"] if pp else ep["details_0"] / nA),
                    AverageStepCount=mean(ep["len_sum"]), AverageMovingCount=mean(ep["details_1"] / nA),
                    AveragePenaltyCount=mean(ep["details_2"] if pp else ep["details_2"] / nA),
                    AverageVariable=mean(ep["details_4"] / nA), AverageVar2=mean(0.0 if pp else ep["details_3"] / nA),
                    AveDegree=deg, Diameter=diam,
                    StdReturn=float(np.sqrt(max(ep["ret_sumsq"] / cnt - avg * avg, 0.0))) if cnt > 0 else nan,
                    MaxReturn=ep["ret_max"] if cnt > 0 else nan, MinReturn=ep["ret_min"] if cnt > 0 else nan,
                    AveTroughput=float(e.env.n_empty_cells if not pp else 0))

    # ------------------------------------------------------------------------------------------
    # gradient exchange
    # ------------------------------------------------------------------------------------------
    def _allreduce_grads(self, n_valid, n_crit):
        """One RCCL all-reduce of [policy grads ‖ critic grads ‖ n_valid ‖ n_crit] through the persistent bucket
        (dist.GradBucket): nothing is allocated and nothing waits for the host per optimiser step."""
        from .dist import GradBucket
        pol, cri = list(self.policy.parameters()), list(self.baseline.parameters())
        b = getattr(self, "_bucket", None)
        if b is None or not b.matches(pol, cri) or b.flat.device != pol[0].device:
            b = self._bucket = GradBucket(pol, cri)
        b.allreduce(n_valid, n_crit)

    def _max_norm(self):
        return float("inf") if self._clip_grad_norm is None else float(self._clip_grad_norm)

    def _mean_grad_norm(self, grad_norm, dev):
        """Mean over the epoch's optimiser steps of the norm the reference records AFTER the clip (:256):
        |g| * min(1, max / (|g| + 1e-6)); optim.Adam hands over |g|^2 per step on the device, the rest is done once here."""
        if not grad_norm:
            return 0.0
        if not torch.is_tensor(grad_norm[0]):
            return float(np.mean(grad_norm))
        pre = torch.stack(grad_norm).to(torch.float32).sqrt()
        return float((pre * torch.clamp(self._max_norm() / (pre + 1e-6), max=1.0)).mean())

    # ------------------------------------------------------------------------------------------
    # train_once (:175-388)
    # ------------------------------------------------------------------------------------------
    def train_once(self, runner=None, itr=None, paths=None):
        with _torch_deterministic() if deterministic() else contextlib.nullcontext():
            return self._train_once(runner, itr, paths)

    def _minibatches(self, batch, advantages, old_ll, distributed):
        """The epoch's minibatches (:209-215).  The permutation is drawn once, so the minibatches are the same path subsets in
        every mini-epoch: gather them once instead of 10 times (each gather copies ~1/3 of the padded batch)."""
        obs, _, actions, rewards, valids, baselines, returns, dist_adjs, channels = batch
        P, T = rewards.shape
        step_size = int(np.ceil(P / self._optimization_n_minibatches))
        if distributed and P < 2 * self._optimization_n_minibatches:
            raise RuntimeError("distributed update needs >= 2 paths per minibatch on every rank (equal optimiser-step counts)")
        shuffled_ids = np.random.permutation(P)                                      # :209
        cols = (obs, actions, rewards, valids, baselines, dist_adjs, channels, advantages, old_ll, returns)
        minibatches = []
        for start in range(0, P, step_size):
            ids = torch.as_tensor(shuffled_ids[start:start + step_size], device=obs.device)
            minibatches.append(_Minibatch(*(None if x is None else x[ids] for x in cols),
                                          n_crit=torch.tensor(float(len(ids) * T), device=obs.device)))
        return minibatches

    def _critic_step(self, mb, side, distributed):
        """The critic's half of a step, on stream `side`: Gaussian NLL, mean over padded steps (comm_base_critic.py:88-89)."""
        with torch.cuda.stream(side):
            bl_loss = self._baseline_loss(mb.obs, mb.returns, mb.dist_adjs, mb.channels)
            (bl_loss * mb.n_crit if distributed else bl_loss).backward()
            if not distributed:
                self._baseline_optimizer.step()

    def _optimiser_step(self, mb, distributed=False, two_streams=False):
        """One optimiser step of both nets on one minibatch (:211-268) -> the squared pre-clip gradient norm (device scalar,
        optim.Adam) or the post-clip norm (host float, any other optimiser)."""
        main = torch.cuda.current_stream(mb.obs.device)
        side = self._side_stream if two_streams else main
        self._baseline_optimizer.zero_grad()
        self._optimizer.zero_grad()
        side.wait_stream(main)                                               # fork: both nets see the minibatch, nothing else
        # Issue order: the policy's chain is the longer one, and a captured graph submits its nodes in capture order - with the
        # critic first the policy's first kernel of a replayed step started ~110 us late (kernel trace of the reference-batch
        # step).  The distributed step keeps the critic first: its gradients must be there when the bucket is reduced.
        if distributed:
            self._critic_step(mb, side, distributed)
        lg = [] if self._update_stats else None
        loss_sum, n_valid = self._compute_loss(None, mb.obs, None, mb.actions, mb.rewards, mb.valids, mb.baselines, mb.dist_adjs,
                                               mb.channels, mb.advantages, mb.old_ll, reduce=False, logits_out=lg)
        if self._update_stats:                                               # this step's row (and the gate), on the policy's stream
            self._upd_state.launch(self, lg[0], mb)
        if distributed:
            loss_sum.backward()
            main.wait_stream(side)
            self._allreduce_grads(n_valid, mb.n_crit)
        else:
            (loss_sum / n_valid).backward()
        if _is_fused_adam(self._optimizer):                                  # optim.Adam: clip + update in two launches
            self._optimizer.step(max_norm=self._max_norm(), return_norm=False)   # policy only (:253-255)
            gn = self._optimizer.norm_sq                                     # a view of the optimiser's workspace
        else:
            if self._clip_grad_norm is not None:
                torch.nn.utils.clip_grad_norm_(self.policy.parameters(), self._clip_grad_norm)
            gn = self.policy.grad_norm()
            self._optimizer.step()                                           # _optimize (:606-610)
        if distributed:
            self._baseline_optimizer.step()
        else:
            self._critic_step(mb, side, distributed)
        main.wait_stream(side)
        return gn

    def _run_steps(self, minibatches, T, distributed):
        """optimization_mini_epochs passes over the minibatches (:209-268), up to and including the epoch's synchronise -> (the
        gradient norm of every applied policy step, in order; the update statistics' stats, {} when they are off).
        The one owner of the optimisers' device-step mode: whoever arms one - this function the policy's, behind the gate, under
        target_kl; _UpdateGraphs at its first replayed step those not armed yet - does so inside the try, and the finally takes
        both out of it with the applied steps booked."""
        dev = minibatches[0].obs.device
        gated = self._target_kl is not None
        stats = _UpdateStats.arm(self, minibatches, distributed) if self._update_stats else None   # (refuses before any step)
        # The critic has its own trunk (a-17): its forward / backward (/ optimiser step) share nothing with the policy's
        # but the minibatch, so they run on a second HIP stream and fill the gaps of the policy's launch chain.
        two_streams = dev.type == "cuda" and os.environ.get("COMMARL_CRITIC_STREAM", "1") != "0"
        if two_streams and (getattr(self, "_side_stream", None) is None or self._side_stream.device != dev):
            self._side_stream = torch.cuda.Stream(device=dev)
        step = functools.partial(self._optimiser_step, distributed=distributed, two_streams=two_streams)
        # mini-epochs 1.. repeat mini-epoch 0's launches on the same buffers with other weights: small (launch-bound) batches
        # capture each minibatch's step into a hipGraph in mini-epoch 1 and replay it from then on (_UpdateGraphs)
        graphs, grad_norm, upd_stats = None, [], {}
        try:
            if gated:                                        # for the whole train_once: the host learns how many steps were
                self._optimizer.begin_device_steps(stats.n_steps, gate=stats.gate)   # applied only after the synchronise
            graphs = _UpdateGraphs.maybe(self, minibatches, T, distributed)
            for mini_epoch in range(self._optimization_mini_epochs):
                for i, mb in enumerate(minibatches):
                    if graphs is not None and mini_epoch >= graphs.first_epoch:
                        gn = graphs.step(i, mb, step)
                    else:
                        gn = step(mb)
                        self._eager_stepped = True
                    grad_norm.append(gn.clone() if torch.is_tensor(gn) else gn)
        finally:
            if graphs is not None:                           # the count of replayed steps, into the optimisers the graphs armed
                graphs.close()
            torch.cuda.synchronize(dev)
            if stats is not None:                            # the rows, and from them the steps the gate let through
                self.update_rows, applied, upd_stats = stats.collect()
                if gated:
                    self._optimizer.end_device_steps(applied)
        # GradNorm: over the applied steps (the stop is sticky: the first ones)
        return (grad_norm[:applied] if gated else grad_norm), upd_stats

    def _train_once(self, runner=None, itr=None, paths=None):
        if runner is not None:
            itr, paths = runner.step_itr, runner.step_path
        t_start = time.time()
        from .dist import is_distributed
        distributed = is_distributed()
        segments = isinstance(paths, SegmentBatch)
        if segments:                                         # refused before anything is launched
            if self._maximum_entropy:
                raise NotImplementedError(self._SEGMENTS_MAXENT)
            if distributed:
                raise NotImplementedError("rollout segments in a distributed update: the batch-wide advantage moments would have "
                                          "to be reduced over the ranks")
        batch = obs, avail, actions, rewards, valids, baselines, returns, dist_adjs, channels = self.process_samples(itr, paths)
        T = rewards.shape[1]
        # entropy_method 'max': no epoch-wide advantages - every loss evaluation derives its own from the current policy's
        # entropy (_max_entropy_advantages), and the full-batch evaluations before / after the update add c * H into `rewards`
        # in place as the reference does (its minibatches are sliced from the tensor loss_before left behind)
        maxent = self._maximum_entropy
        if segments:
            advantages = self._segment_advantages(paths)
        else:
            advantages = None if maxent else self._advantages(rewards, baselines, valids)
        # The reference evaluates the two policies over the full batch eight times per epoch (old log-likelihood twice, loss
        # before / after, KL + entropy before / after with both nets each).  Only three distinct (weights, batch) pairs are
        # involved - last epoch's pre-update weights, this epoch's (which the old policy becomes at :204) and the post-update
        # ones - so three forwards are run and shared, for every policy kind (no logits from a row-MLP forward: the loss runs its own)
        full_loss = functools.partial(self._compute_loss, itr, obs, avail, actions, rewards, valids, baselines, dist_adjs, channels,
                                      advantages, rewards_in_place=maxent)
        with torch.no_grad():
            _, p_old0 = self._evaluate(self._old_policy, obs, dist_adjs, channels)
            lg_new, p_new = self._evaluate(self.policy, obs, dist_adjs, channels)
            loss_before = float(full_loss(self._ll_from_probs(p_old0, actions), logits=lg_new))
            kl_before, _ = self._kl_entropy(p_old0, p_new)
            del p_old0, lg_new
        self._old_policy.load_state_dict(self.policy.state_dict())                  # :204
        old_ll = self._ll_from_probs(p_new, actions)                                 # the old policy now IS the policy

        t_opt = time.time()
        minibatches = self._minibatches(batch, advantages, old_ll, distributed)
        grad_norm, upd_stats = self._run_steps(minibatches, T, distributed)   # (ends with the epoch's synchronise)
        epoch_time = time.time() - t_opt
        self.policy.sync_weights()

        with torch.no_grad():
            lg_after, p_after = self._evaluate(self.policy, obs, dist_adjs, channels)
            loss_after = float(full_loss(old_ll, logits=lg_after))
            kl, entropy = self._kl_entropy(p_new, p_after)
            del lg_after, p_after, p_new
        perf = self._log_performance(itr, paths, returns, valids)
        self.stats = dict(perf, LossBefore=loss_before, LossAfter=loss_after,
                          dLoss=loss_before - loss_after, KLBefore=kl_before, KL=kl, Entropy=entropy,
                          GradNorm=self._mean_grad_norm(grad_norm, obs.device), EpochTime=epoch_time,
                          TrainOnceTime=time.time() - t_start, MaxPathLength=T,
                          EnvSteps=int(valids.sum().item()),
                          GPUMemoryMax=torch.cuda.max_memory_allocated(self._dev()) / 1024 ** 3,     # :372-383 (GiB)
                          **upd_stats)
        for k, v in self.stats.items():
            tabular.record(k, v)
        return perf["AverageReturn"]

    def train(self, runner):
        """MABatchPolopt.train (com_marl/np/algos/ma_batch_polopt.py:72-120): sample -> train_once per epoch."""
        last_return = None
        for _epoch in runner.step_epochs():
            if getattr(runner, "flag", [0])[0]:
                break
            for _ in range(self.n_samples):
                runner.step_path = runner.obtain_samples(runner.step_itr)
                last_return = self.train_once(runner)
                runner.step_itr += 1
        return last_return
