"""Device-resident rollout engine: the inner loop of
CentralizedMAOnPolicyVectorizedSampler.obtain_samples (com_marl/sampler/
centralized_ma_on_policy_vectorized_sampler.py:119-232) for B envs at once.

One step = one fused launch (cm_rollout_step) where the library has a fused kernel for the shape, else two kernel
launches; either way no host synchronisation and no copies:
    policy forward + sample  (cm_policy_forward)  reads  obs[t], dist_adj[t], channels[t]
                                                   writes actions[t], probs[t], attn[t]
    env step + auto-reset    (cm_env_step)        reads  actions[t]
                                                   writes obs[t+1], reward[t], done[t], ... , dist_adj[t+1], channels[t+1]
The trajectory buffers are time-major [H(+1), B, ...] in HBM, so every step reads and writes
contiguous [B, ...] slabs and the kernels write straight into them (zero-copy).  A chunk of
steps can be captured into a hipGraph and replayed (the launch-bound regime at 4096 x N=4).
"""
import contextlib
import ctypes as C
import os

import torch

from . import _lib as L
from .envs import graph_diameter
from .nets import PolicySet

WG_ENVS = 16                 # envs per workgroup of the wave-owned kernels: a multi-policy launch gives each workgroup one policy

# replay_probs under the identity channel: bytes of the one constant mask block an engine keeps for it (cm_policy_forward reads a
# channel block per env state, so the identity is written out for the rows of ONE launch and reused by the next) - at the
# headline shape (N = 4, 2 hops: 128 bytes per env state) 64 slots of 4096 envs per launch; never below one env state (at most
# 2 MB: 8 hops x 255^2).  REPLAY_ROW_ALIGN: launches start on whole workgroups of the forward kernels
REPLAY_MASK_BYTES = 32 << 20
REPLAY_ROW_ALIGN = 64

_null = contextlib.nullcontext


class _Parts:
    """Facade over several GridEnvBatch shards that together form one batch (global env ids are
    contiguous: shard k starts at the end of shard k-1)."""

    def __init__(self, parts):
        self.parts = parts
        e0 = parts[0]
        self.device, self.N, self.M, self.d, self.Lh = e0.device, e0.N, e0.M, e0.d, e0.Lh
        self.adj_const, self.ch_const, self.scenario = e0.adj_const, e0.ch_const, e0.scenario
        self.n_empty_cells, self.channels = e0.n_empty_cells, e0.channels
        self.calc_diameter = getattr(e0, "calc_diameter", False)
        self.B = sum(p.B for p in parts)
        self.bounds, lo = [], 0
        for p in parts:
            if getattr(p, "conditions", None) is not None:
                raise ValueError("per-env comm conditions run on one GridEnvBatch, not on shards")
            assert (p.N, p.d, p.Lh, p.scenario) == (e0.N, e0.d, e0.Lh, e0.scenario) and p.device == e0.device
            assert p.cfg.env_id_offset == e0.cfg.env_id_offset + lo, "shards must cover contiguous global env ids"
            self.bounds.append((lo, lo + p.B))
            lo += p.B

    def check_status(self):
        for p in self.parts:
            p.check_status()


class RolloutEngine:
    def __init__(self, env, policy, horizon, store_attn=True, store_probs=True, fused="auto", persistent="auto",
                 graph_fused=True, groups=None):
        """env: envs.GridEnvBatch, or a list of shards of one batch (then every shard runs its own
        policy -> env chain on its own HIP stream: the chains are independent, so kernels of different
        shards overlap and their phases drift apart instead of contending in lockstep).
        policy: nets.CommCategoricalMLPPolicy (or the Obs-DP / CENT policy) on the same device, or a nets.PolicySet of K
        policies on one GridEnvBatch: `groups` lists the env count of each member (default: B / K each), member k owning the
        contiguous envs [lo_k, hi_k).  Each env plays exactly what it would play in a single-policy engine whose env batch
        starts at the same global env id.  Teams of 4 whose groups start on multiples of 16 envs run a chunk as ONE
        cm_rollout_chunk_multi launch (multi_form "wave"); every other set takes one forward + one env step over the batch per
        step (multi_form "loop"), the forward being ONE launch for all members where the library has a set kernel for the
        shape (multi_forward "set": cm_policy_forward_multi for Comm-DP teams other than 4, up to 80 agents,
        cm_mlp_policy_forward_multi for Obs-DP / CENT members of any team size, and cm_policy_forward_any_multi for a
        PolicySet(any_sizes=True) of Comm-DP nets with non-default - also mixed - layer sizes; one sampler seed, production RNG) and one
        forward launch per member on its envs otherwise (multi_forward "member")."""
        if isinstance(env, (list, tuple)):
            env = _Parts(list(env)) if len(env) > 1 else env[0]
        self.env, self.policy, self.H = env, policy, int(horizon)
        self.parts = env.parts if isinstance(env, _Parts) else [env]
        self.bounds = env.bounds if isinstance(env, _Parts) else [(0, env.B)]
        self.streams = [torch.cuda.Stream(device=env.device) for _ in self.parts] if len(self.parts) > 1 else [None]
        self.id0 = self.parts[0].cfg.env_id_offset
        dev, B, N, M, d, Lh = env.device, env.B, env.N, max(env.M, 1), env.d, env.Lh
        A = policy._action_dim
        store_attn = store_attn and hasattr(policy, "comm")     # Obs-DP / CENT policies have no attention output
        H = self.H
        f32, i32, u8 = torch.float32, torch.int32, torch.uint8
        z = lambda *shape, dtype=f32: torch.zeros(*shape, dtype=dtype, device=dev)   # noqa: E731
        self.obs = z(H + 1, B, N, d)
        self.actions = z(H, B, N, dtype=i32)
        self.probs = z(H, B, N, A) if store_probs else None
        self.attn = z(H, B, N, N) if store_attn else None
        self.reward = z(H, B)
        self.reward64 = z(H, B, dtype=torch.float64)
        self.done = z(H, B, dtype=u8)
        self.details = z(H, B, 6, dtype=i32)
        self.prey_alive = z(H, B, M, dtype=u8) if env.M else None
        self.success = z(H, B, dtype=i32)
        self.path_len = z(H, B, dtype=i32)
        # constant masks are never stored per step (4N^2 [adj != const] rule of SURVEY.md §8d)
        self.dist_adj = None if env.adj_const else z(H + 1, B, N, N)
        self.channels = None if env.ch_const else z(H + 1, B, Lh, N, N)
        # params['calc_diameter'] on a range graph: the hop diameter of dist_adj[t][b], filled by ONE cm_graph_diameter launch
        # per finished span of slots (fill_diameters) - derived data, no kernel of the step loop knows it.  None = switch off.
        self.diameter = z(H + 1, B, dtype=i32) if self.dist_adj is not None and getattr(env, "calc_diameter", False) else None
        # device-side Philox counter base of the action sampler (uint32 bits), ONE PER SHARD: every shard bumps its own
        # copy on its own stream (all copies always hold the same value), so that the shards' chains share nothing
        self.step_bases = [torch.zeros(1, dtype=i32, device=dev) for _ in self.parts]
        self._graphs = {}
        self._eye_rows = None                    # replay_probs' constant identity block, built on first use
        # fused: step() uses cm_rollout_step (policy forward + sample + env step in one launch) where the library has a fused
        # kernel for the shape.  fused="auto": teams of 4 only - for larger teams the fused kernel runs the env step of ONE env on
        # a 256-thread workgroup that is mostly idle (measured per step: N = 24 127 vs 95 us, N = 72 424 vs 176 us), so they take
        # the two-kernel form.  True forces it (parity tests), False disables it.
        # persistent: a chunk / span of steps as ONE cm_rollout_chunk launch per shard.  "auto": teams of 4 on the wave-owned
        # kernel (csrc/cm_rollout_w.hip: a wave keeps its four envs and the weights stay in LDS / registers for the whole
        # chunk - 17.0 us per step at the headline config against 24.7 for one launch per step, which re-stages 145 KB of
        # weights per workgroup every step); the older workgroup-tiled kernels (COMMARL_POLICY_KERNEL=h / f32) step faster
        # with one launch per step under a hipGraph and keep that form.  Both forms are bit-identical
        # (tests/test_hip_fused_parity.py).
        if fused == "auto":
            fused = getattr(policy, "_n_agents", 0) == 4
        if persistent == "auto":
            pk = os.environ.get("COMMARL_POLICY_KERNEL", "w")[:1]
            persistent = bool(fused) and getattr(policy, "_n_agents", 0) == 4 and pk not in ("h", "f", "v") \
                and os.environ.get("COMMARL_PERSISTENT", "1") != "0"
        self._fused = None if fused else False              # None = try the fused step, False = two launches per step
        self._persistent = bool(persistent and fused)
        self._capturing = False
        # captured chunks: one fused launch per step (cm_rollout_step) or the two-kernel form - measured per config in
        # bench.py
        self._fused_in_graph = bool(fused) and bool(graph_fused)
        self.t = 0
        self.generation = 0                      # bumped by reset(): a PathBatch of an earlier rollout refuses to read the buffers
        self.multi_form = None                   # PolicySet: "wave" (one launch per chunk for all members) or "loop"
        self.multi_forward = None                # loop form: "set" (one forward launch for all members) or "member"
        if isinstance(policy, PolicySet):
            self._init_multi(groups)
        elif groups is not None:
            raise ValueError("groups= splits the envs between the members of a nets.PolicySet")

    def _init_multi(self, groups):
        ps, B = self.policy, self.env.B
        if len(self.parts) != 1:
            raise ValueError("a PolicySet runs on one GridEnvBatch, not on shards")
        K = len(ps)
        if groups is None:
            if B % K:
                raise ValueError(f"{B} envs do not split evenly between {K} policies: pass groups=")
            groups = [B // K] * K
        groups = [int(g) for g in groups]
        if len(groups) != K or min(groups) < 1 or sum(groups) != B:
            raise ValueError(f"groups must give each of the {K} policies at least one env and sum to B={B}: {groups}")
        self.groups, lo = [], 0
        for g in groups:
            self.groups.append((lo, lo + g))
            lo += g
        # one launch for the whole set: teams of 4 on the default (wave-owned) kernel, every member's envs in whole workgroups of
        # 16, one sampler seed; the library may still answer "not for this shape" (1), and the engine then loops from there on
        pk = os.environ.get("COMMARL_POLICY_KERNEL", "w")[:1]
        # (ps.forward_kind "default": Comm-DP policies that pass the whole architecture check and have the default layer sizes)
        wave = (ps.forward_kind == "default" and ps._n_agents == 4
                and pk not in ("h", "f", "v") and ps.seed is not None
                and all(lo % WG_ENVS == 0 for lo, _ in self.groups) and getattr(self.env.cfg, "rng_mode", 0) == L.RNG_PHILOX)
        self.multi_form = "wave" if wave else "loop"
        self._persistent, self._fused = wave, None
        # loop form: one forward launch for the whole set (cm_policy_forward_multi for Comm-DP members, cm_mlp_policy_forward_multi
        # for Obs-DP / CENT members) - one sampler seed, production RNG; the library answers "not for this shape" (1) for the
        # teams it has no set kernel for, and the engine remembers it.  PolicySet(any_sizes=True) of non-default Comm-DP nets:
        # cm_policy_forward_any_multi, whatever the members' layer sizes
        set_fwd = (ps.forward_kind is not None and ps.seed is not None
                   and getattr(self.env.cfg, "rng_mode", 0) == L.RNG_PHILOX)
        self.multi_forward = None if wave else ("set" if set_fwd else "member")
        if wave:
            n_wg = (B + WG_ENVS - 1) // WG_ENVS
            wg = [k for k, (lo, hi) in enumerate(self.groups) for _ in range(lo // WG_ENVS, (hi + WG_ENVS - 1) // WG_ENVS)]
            assert len(wg) == n_wg and all(0 <= k < K for k in wg)       # checked here: the kernel trusts the table
            self._wg_policy = torch.tensor(wg, dtype=torch.int32).to(self.env.device)

    def _multi_chunk(self, t0, n, greedy):
        """Slots t0 .. t0+n-1 of every member in ONE cm_rollout_chunk_multi launch.  False - nothing launched - when the
        library has no multi-policy kernel for this shape (the engine loops member by member from then on).  The members'
        packs are used as they are: sync_weights() (run_chunk, prepare_graph, eval_models) refreshes them."""
        if self.multi_form != "wave":
            return False
        ps, env, B = self.policy, self.env, self.env.B
        w = ps[0]._weights_struct()                                         # the shape every member shares
        st = L.PolicySetT(len(ps), self._wg_policy.numel(), L.ptr(ps.pack_table()), L.ptr(self._wg_policy))
        obs, adj, ch, actions, probs, attn = self._slot(t0, 0, B)
        if not L.run("cm_rollout_chunk_multi", env._h, C.byref(w), C.byref(st), int(n), C.byref(self._strides()), L.ptr(obs),
                     L.ptr(adj), L.ptr(ch), ps.seed, self.id0, t0 & 0xFFFFFFFF, L.ptr(self.step_bases[0]), int(greedy), L.ptr(actions),
                     L.ptr(probs), L.ptr(attn), C.byref(env._out(self._out(t0, 0, B))), device=env.device, maybe=True):
            self.multi_form, self._persistent, self.multi_forward = "loop", False, "member"     # (teams of 4: no set forward)
            return False
        return True

    def _set_forward(self, t, greedy):
        """Slot t's forward + sample of every member in ONE launch over the batch: cm_policy_forward_multi,
        cm_mlp_policy_forward_multi for Obs-DP / CENT members, or cm_policy_forward_any_multi for a PolicySet(any_sizes=True) of
        non-default Comm-DP nets.  The set names the entry point and the arguments it begins with (PolicySet.forward_call); the
        rest is the same for every kind.  False - nothing launched - when the library has no set kernel
        for this shape (the engine launches member by member from then on).  The members' packs are used as they are, as in
        _multi_chunk."""
        ps, B = self.policy, self.env.B
        call = ps.forward_call([hi - lo for lo, hi in self.groups], B)
        done = False                                                        # no table: as the library's "not for this shape"
        if call is not None:
            what, lead = call
            obs, adj, ch, actions, probs, attn = self._slot(t, 0, B)
            # the Obs-DP / CENT entry point has no adjacency, channel or attention argument
            graph, attn = ((), ()) if ps.forward_kind == "mlp" else ((L.ptr(adj), L.ptr(ch)), (L.ptr(attn),))
            done = L.run(what, *lead, L.ptr(obs), None, *graph, ps.seed, self.id0, t & 0xFFFFFFFF, L.ptr(self.step_bases[0]),
                         int(greedy), L.ptr(actions), L.ptr(probs), *attn, device=self.env.device, maybe=True)
        if not done:
            self.multi_forward = "member"
        return done

    def _multi_step(self, t, greedy):
        """Slot t -> t+1 for every member: one launch (a chunk of one step) where the set has the multi-policy kernel, else the
        members' forward + sample - one launch for the set, or each member on its envs (env ids id0 + lo_k, the shared Philox
        base) - and one env step over the batch."""
        if self._multi_chunk(t, 1, greedy):
            return
        if self.multi_forward != "set" or not self._set_forward(t, greedy):
            for pol, (lo, hi) in zip(self.policy, self.groups):
                obs, adj, ch, actions, probs, attn = self._slot(t, lo, hi)
                pol.act_device(
                    obs, None, adj, ch, greedy=greedy, out_actions=actions, out_probs=probs, out_attn=attn,
                    want_probs=self.probs is not None, want_attn=self.attn is not None,
                    policy_step=t, step_base=self.step_bases[0], env_id_offset=self.id0 + lo)
        self.env.step_device(self.actions[t], out=self._out(t, 0, self.env.B))

    @property
    def step_base(self):
        return self.step_bases[0]

    def bump(self, n):
        """Advance the sampler's Philox counter base by n policy steps (what a chunk does at its end)."""
        for k, st in enumerate(self.streams):
            with torch.cuda.stream(st) if st is not None else _null():
                self.step_bases[k].add_(n)

    # ------------------------------------------------------------------------------------------
    def _slot(self, t, lo, hi):
        """The policy-side views of slot t for envs lo .. hi-1: obs as [nb, N*d], dist_adj, channels, actions, probs, attn
        (None where the engine keeps no such buffer)."""
        cut = lambda b: None if b is None else b[t][lo:hi]                           # noqa: E731
        return self.obs[t][lo:hi].view(hi - lo, -1), cut(self.dist_adj), cut(self.channels), self.actions[t][lo:hi], \
            cut(self.probs), cut(self.attn)

    def _out(self, t, lo, hi):
        o = dict(obs=self.obs[t + 1][lo:hi], reward=self.reward[t][lo:hi], reward_f64=self.reward64[t][lo:hi],
                 done=self.done[t][lo:hi], details=self.details[t][lo:hi], success=self.success[t][lo:hi],
                 path_len=self.path_len[t][lo:hi])
        if self.prey_alive is not None:
            o["prey_alive"] = self.prey_alive[t][lo:hi]
        if self.dist_adj is not None:
            o["dist_adj"] = self.dist_adj[t + 1][lo:hi]
        if self.channels is not None:
            o["channels"] = self.channels[t + 1][lo:hi]
        return o

    # ---- forward-only replay ---------------------------------------------------------------------
    def _identity_rows(self, rows):
        """-> [r, Lh, N, N] identity channels (every agent hears only itself, on every hop) for r = min(rows, what
        REPLAY_MASK_BYTES holds, at least one) env states: ONE constant block per engine, reused by every launch of every
        replay - a [T, B, Lh, N, N] tensor is never built."""
        env = self.env
        cap = max(1, REPLAY_MASK_BYTES // (4 * env.Lh * env.N * env.N))
        if cap >= REPLAY_ROW_ALIGN:
            cap -= cap % REPLAY_ROW_ALIGN                   # whole workgroups of the forward kernels in every launch but the last
        r = min(int(rows), cap)
        if self._eye_rows is None or self._eye_rows.shape[0] < r:
            self._eye_rows = torch.eye(env.N, dtype=torch.float32, device=env.device).expand(r, env.Lh, env.N, env.N).contiguous()
        return self._eye_rows[:r]

    def _replay(self, who, t0, n, channels, actors, several, launch, out, tail, check=None):
        """The route of replay_probs / replay_values (`who`, for the refusals' texts): `actors` - one policy / critic, or with
        `several` one per group - on the recorded slots t0 .. t0+n-1 under `channels`, into out [n, B, *tail].  launch(actor, obs
        [R, N*d], adj [R, N, N] | None, ch [R, Lh, N, N] | None, out [R, *tail]) is the forward-only launch on R env states.  One
        actor takes the n * B rows as they lie (slots are contiguous in the buffers); of several each takes its n * (hi - lo) rows,
        gathered from the slots by device copies and scattered back (a member's envs are contiguous within a slot only; the
        gathered rows of one member at a time are the replay's only temporaries).  Either way ONE launch per actor, or one per
        _identity_rows block of rows under the identity.  check(): the caller's own refusals, behind the common ones."""
        env = self.env
        B, N, d, Lh = env.B, env.N, env.d, env.Lh
        t0, n = int(t0), int(n)
        if channels not in ("recorded", "identity", "ones"):
            raise ValueError(f"{who}: channels must be 'recorded', 'identity' or 'ones', not {channels!r}")
        if not (n >= 1 and t0 >= 0 and t0 + n <= self.H):
            raise ValueError(f"{who}: slots {t0} .. {t0 + n - 1} are not within the horizon {self.H}")
        if not (out.dtype == torch.float32 and tuple(out.shape) == (n, B) + tail and out.is_contiguous() and out.device == self.obs.device):
            raise ValueError(f"{who}: out must be a contiguous f32 tensor [{', '.join(map(str, (n, B) + tail))}] on the engine's device")
        if check is not None:
            check()
        adj, chan = self.dist_adj, self.channels if channels == "recorded" else None     # (NULL where the engine keeps none)

        def rows(actor, obs, adj, chan, out):
            R = obs.shape[0]
            eye = self._identity_rows(R) if channels == "identity" else None
            step = R if eye is None else eye.shape[0]
            for r0 in range(0, R, step):
                r1 = min(R, r0 + step)
                ch = eye[:r1 - r0] if eye is not None else (None if chan is None else chan[r0:r1])
                launch(actor, obs[r0:r1], None if adj is None else adj[r0:r1], ch, out[r0:r1])

        if not several:
            flat = lambda b, *shape: None if b is None else b[t0:t0 + n].view(n * B, *shape)    # noqa: E731
            rows(actors, flat(self.obs, N * d), flat(adj, N, N), flat(chan, Lh, N, N), out.view(n * B, *tail))
            return out
        for actor, (lo, hi) in zip(actors, self.groups):
            # 3 copies + 1 launch instead of n launches
            R = n * (hi - lo)
            take = lambda b, *shape: None if b is None else b[t0:t0 + n, lo:hi].reshape(R, *shape)   # noqa: E731
            mine = torch.empty(R, *tail, dtype=torch.float32, device=out.device)
            rows(actor, take(self.obs, N * d), take(adj, N, N), take(chan, Lh, N, N), mine)
            out[:, lo:hi] = mine.view(n, hi - lo, *tail)
        return out

    @torch.no_grad()
    def replay_probs(self, t0, n, channels, out):
        """Forward only: the action probabilities of the recorded slots t0 .. t0+n-1 - their obs[t] and dist_adj[t] as they
        stand - under `channels` into out [n, B, N, A] (f32, contiguous, the caller's):
            "recorded"   channels[t] as recorded (what the round's forward read: NULL where the engine keeps none),
            "identity"   every agent hears only itself on every hop (the FL channel),
            "ones"       everything in range is delivered (the FC channel; passed as NULL).
        For every env they are what its policy's act_device(..., want_actions=False) returns on these inputs.  A single policy
        takes ONE launch over the n * B rows (slots are contiguous in the buffers), a PolicySet ONE launch per member over
        its n * (hi - lo) rows, gathered from the slots by device copies and scattered back (a member's envs are contiguous
        within a slot only; the gathered rows of one member at a time are the replay's only temporaries).  Under the identity
        a launch covers at most the rows of the engine's constant mask block, which REPLAY_MASK_BYTES bounds whatever n is.
        Nothing else changes: no recorded buffer is written, nothing is drawn, and neither the sampler's Philox base nor a
        policy's step counter moves.  The weight packs are used as they are (the round that recorded the slots synced them).
        On the current stream, behind the round (play() has joined the shards)."""
        def launch(pol, obs, adj, ch, probs):                   # act_device without actions, attention or a draw
            pol.act_device(obs, None, adj, ch, greedy=True, want_actions=False, want_attn=False, out_probs=probs, policy_step=0)

        return self._replay("replay_probs", t0, n, channels, self.policy, self.multi_form is not None, launch, out,
                            (self.env.N, self.policy._action_dim))

    @torch.no_grad()
    def replay_values(self, t0, n, channels, critics, out):
        """Forward only: what `critics` - one critic (nets.CommBaseCritic of any aggregator and layer sizes, or
        nets.GaussianMLPBaseline), or a list with one per group of a PolicySet engine, critic k judging member k's envs - make of
        the recorded slots t0 .. t0+n-1, their obs[t] and dist_adj[t] as they stand, under `channels` ("recorded", "identity" or
        "ones": replay_probs' three), into out [n, B] (f32, contiguous, the caller's).  For every env they are what its critic's
        values_device returns on these inputs.  A single critic takes ONE launch over the n * B rows (under the identity one per
        block of the engine's constant mask, which REPLAY_MASK_BYTES bounds), a list ONE launch per member over its
        n * (hi - lo) rows, gathered from the slots by device copies and scattered back.  A GaussianMLPBaseline has no graph input:
        channels other than "recorded" are refused for it.  Nothing else changes: no recorded buffer is written and neither the
        sampler's Philox base nor a step counter moves.  The weight packs are used as they are (the caller has run the critics'
        sync_weights()).  On the current stream, behind the round (play() has joined the shards)."""
        several = isinstance(critics, (list, tuple))

        def check():
            if several and (self.multi_form is None or len(critics) != len(self.groups)):
                raise ValueError("replay_values: a list of critics needs a PolicySet engine and one critic per group")
            if channels != "recorded" and not all(hasattr(c, "comm") for c in (critics if several else [critics])):
                raise ValueError(f"replay_values: channels={channels!r} needs critics with a graph input (a GaussianMLPBaseline has none)")

        def launch(critic, obs, adj, ch, values):
            if hasattr(critic, "comm"):
                critic.values_device(obs, adj, ch, out=values)
            else:                                               # (a GaussianMLPBaseline reads the observations alone)
                critic.values_device(obs, out=values)

        return self._replay("replay_values", t0, n, channels, critics, several, launch, out, (), check)

    def fill_diameters(self, t0, n):
        """diameter[t] of the n slots t0 .. t0+n-1 from dist_adj[t], in one launch on the current stream (the caller has
        joined the shards' streams: the slots are final).  Nothing without the switch."""
        if self.diameter is not None and n > 0:
            graph_diameter(self.dist_adj[t0:t0 + n], out=self.diameter[t0:t0 + n])

    def span_diameters(self, t0, n):
        """Behind a span over slots t0 .. t0+n-1: the slots it wrote, t0+1 .. t0+n, and with them slot 0 (the reset's, or the
        one a chunk's tail carried) when the span starts there."""
        if t0 == 0:
            self.fill_diameters(0, n + 1)
        else:
            self.fill_diameters(t0 + 1, n)

    def reset(self):
        """VecEnvExecutor.reset: every env restarts; slot 0 receives the first observation."""
        for part, (lo, hi) in zip(self.parts, self.bounds):
            o = dict(obs=self.obs[0][lo:hi])
            if self.dist_adj is not None:
                o["dist_adj"] = self.dist_adj[0][lo:hi]
            if self.channels is not None:
                o["channels"] = self.channels[0][lo:hi]
            part.reset_all(out=o)
        self.t = 0
        self.generation += 1

    def _step_part(self, k, t, greedy):
        if self.multi_form is not None:
            self._multi_step(t, greedy)
            return
        part, (lo, hi) = self.parts[k], self.bounds[k]
        obs, adj, ch, actions, probs, attn = self._slot(t, lo, hi)
        if self._fused is not False and (not self._capturing or self._fused_in_graph) and hasattr(self.policy, "step_fused"):
            # policy forward + sample + env step of this shard in one launch (cm_rollout_step); shapes without a fused
            # kernel report "not available" once and the two-launch path below is used from then on
            ok = self.policy.step_fused(
                part, obs, adj, ch, part._out(self._out(t, lo, hi)), greedy=greedy, out_actions=actions, out_probs=probs, out_attn=attn,
                policy_step=t, step_base=self.step_bases[k], env_id_offset=self.id0 + lo)
            self._fused = ok
            if ok:
                return
        self.policy.act_device(
            obs, None, adj, ch, greedy=greedy, out_actions=actions, out_probs=probs, out_attn=attn,
            want_probs=self.probs is not None, want_attn=self.attn is not None,
            policy_step=t, step_base=self.step_bases[k], env_id_offset=self.id0 + lo)
        part.step_device(actions, out=self._out(t, lo, hi))

    def step(self, t, greedy=False):
        """Slot t -> t+1 (asynchronous).  With several shards each chain goes to its own stream; call
        join() (or run_chunk) before the host or another stream consumes the slot."""
        if len(self.parts) == 1:
            self._step_part(0, t, greedy)
            return
        for k, st in enumerate(self.streams):
            with torch.cuda.stream(st):
                self._step_part(k, t, greedy)

    def fork(self):
        cur = torch.cuda.current_stream(self.env.device)
        for st in self.streams:
            if st is not None:
                st.wait_stream(cur)

    def join(self):
        cur = torch.cuda.current_stream(self.env.device)
        for st in self.streams:
            if st is not None:
                cur.wait_stream(st)

    def play(self, t0, n, greedy=False, chunk=True):
        """Slots t0 .. t0+n-1, joined (a round of an evaluation): with `chunk` as steps_fused's launch where the library has
        one, else - and where it has none - step by step between fork() and join().  Bit-identical either way; neither resets
        nor bumps the sampler's Philox base."""
        if chunk and self.steps_fused(t0, n, greedy=greedy):
            return
        self.fork()
        for t in range(t0, t0 + n):
            self.step(t, greedy=greedy)
        self.join()

    def _wrap_part(self, k, n):
        """Carry the last slot written by an n-step chunk into slot 0 for shard k (what `obses = next_obses` does)."""
        lo, hi = self.bounds[k]
        self.obs[0][lo:hi].copy_(self.obs[n][lo:hi])
        if self.dist_adj is not None:
            self.dist_adj[0][lo:hi].copy_(self.dist_adj[n][lo:hi])
        if self.channels is not None:
            self.channels[0][lo:hi].copy_(self.channels[n][lo:hi])

    def _chunk_tail(self, k, n):
        """Shard k: counter bump + slot n -> slot 0 in one launch (cm_chunk_tail) on the current stream."""
        lo, hi = self.bounds[k]
        pairs = [(b[n][lo:hi], b[0][lo:hi]) for b in (self.obs, self.dist_adj, self.channels) if b is not None]
        args = []
        for src, dst in pairs + [(None, None)] * (3 - len(pairs)):
            args += [L.ptr(src), L.ptr(dst), 0 if src is None else src.numel() * src.element_size()]
        L.run("cm_chunk_tail", L.ptr(self.step_bases[k]), n, *args, device=self.env.device)

    def carry(self, n):
        """Slot n into slot 0 and the sampler's Philox base += n, every shard on its own stream, joined: a chunk's tail
        (cm_chunk_tail) as a call of its own.  obtain_segments puts it at the head of every call but the first - behind the
        chunk it would overwrite the slot 0 of the segment just returned."""
        self.fork()
        for k, st in enumerate(self.streams):
            with torch.cuda.stream(st) if st is not None else _null():
                self._chunk_tail(k, n)
        self.join()

    def _strides(self):
        e = self.env
        B, N, M, d, Lh, A = e.B, e.N, max(e.M, 1), e.d, e.Lh, self.policy._action_dim
        return L.ChunkStrides(obs=B * N * d, actions=B * N, probs=B * N * A, attn=B * N * N, reward=B, reward_f64=B,
                              done=B, details=B * 6, dist_adj=B * N * N, channels=B * Lh * N * N, prey_alive=B * M,
                              success=B, path_len=B)

    def steps_fused(self, t0, n, greedy=False, tail=False):
        """Slots t0 .. t0+n-1 in one persistent launch per shard (cm_rollout_chunk); tail: followed by the chunk's tail - slot
        t0+n into slot 0, Philox base += n (cm_rollout_chunk_tail: the same launch where the library can).  False when the
        library has no fused kernel for this shape (nothing was launched)."""
        if self.multi_form is not None:                     # PolicySet: every member in one launch, or False (loop form)
            if not self._multi_chunk(t0, n, greedy):
                return False
            if tail:
                self._chunk_tail(0, t0 + n)
            return True
        if self._fused is False or not hasattr(self.policy, "chunk_fused") or getattr(self.parts[0].cfg, "rng_mode", 0) != L.RNG_PHILOX:
            return False
        st = self._strides()
        self.fork()
        for k, stream in enumerate(self.streams):
            part, (lo, hi) = self.parts[k], self.bounds[k]
            obs, adj, ch, actions, probs, attn = self._slot(t0, lo, hi)
            with torch.cuda.stream(stream) if stream is not None else _null():
                ok = self.policy.chunk_fused(
                    part, n, st, obs, adj, ch, part._out(self._out(t0, lo, hi)), greedy=greedy, out_actions=actions,
                    out_probs=probs, out_attn=attn, policy_step=t0, step_base=self.step_bases[k], env_id_offset=self.id0 + lo,
                    tail_next=self._slot(0, lo, hi)[:3] if tail else None)
            if not ok:
                assert k == 0, "fused chunk availability must not differ between shards"
                self._fused = False
                self.join()
                return False
        self.join()
        self._fused = True
        return True

    def _chunk(self, n, t0=0, tail=True):
        """All shards: fork, every shard's n-step chain over slots t0 .. t0+n-1 (+ its tail) on its own stream, join.  The
        launches are issued step by step across the shards (t outer, shard inner): a captured graph submits its nodes in
        capture order, so issuing one shard's whole chain first would start the other shard's chain only after it
        (measured: ~100 us stagger per replay, profiles/r02_trace_short.txt).  tail=False (the sampler's spans): no carry
        of slot t0+n into slot 0 and no bump of the sampler's Philox base - the caller bumps once per rollout."""
        if self._persistent and self.steps_fused(t0, n, tail=tail):    # one launch per shard for the whole span, its tail included
            return
        self.fork()
        for t in range(t0, t0 + n):
            for k, st in enumerate(self.streams):
                with torch.cuda.stream(st) if st is not None else _null():
                    self._step_part(k, t, False)
        if tail:
            for k, st in enumerate(self.streams):
                with torch.cuda.stream(st) if st is not None else _null():
                    self._chunk_tail(k, t0 + n)
        self.join()

    def prepare_graph(self, n=None, t0=0, tail=True):
        """Capture + instantiate the hipGraph of an n-step chunk over slots t0 .. t0+n-1 (t0 + n <= H, default the whole
        horizon) WITHOUT advancing the rollout.
        One graph holds every shard's chain as a parallel branch (fork ... join).  Measured alternatives
        (profiles/r02_steps_sweep.txt, config 2): one single-stream graph per shard replayed on the shards' own
        streams runs 37.7 us/step against 36.4 for the joint graph - independent streams start in phase, so policy
        kernels meet policy kernels, whereas the joint graph's second branch starts ~100 us (three steps) after the
        first and the shards stay out of phase; that same stagger is why a SHORT run (bench.py --steps 20) is better
        off with a single shard.
        One-time host-side setup that must not happen inside a capture (the weight pack, the kernels'
        hipFuncSetAttribute calls) is triggered by one scratch step whose effects are undone: the env state is
        snapshotted before and restored after it, and every trajectory slot it wrote is rewritten by the chunk itself.
        Call it before a timed region; run_chunk() / run_span() call it on first use otherwise."""
        n = self.H if n is None else int(n)
        t0 = int(t0)
        assert n >= 1 and t0 >= 0 and t0 + n <= self.H
        key = (t0, n, bool(tail))
        g = self._graphs.get(key)
        if g is not None:
            return g
        self.policy.sync_weights()
        if not self._graphs:                                # first capture of this engine: the scratch step
            saved = [part.get_state() for part in self.parts]
            saved_slot = [b[t0:t0 + 2].clone() for b in (self.obs, self.dist_adj, self.channels) if b is not None]
            self._capturing = True                          # the launch form the capture will issue
            try:
                self.fork()
                self.step(t0)
                self.join()
            finally:
                self._capturing = False
            torch.cuda.synchronize(self.env.device)
            for part, st in zip(self.parts, saved):
                part.set_state(**st)
            # slot t0 is the chunk's INPUT when the sampler captures mid-rollout (the scratch step only wrote slot t0 + 1
            # and the per-step outputs, all rewritten by the chunk; restoring both slots keeps the argument simple)
            for b, keep in zip([b for b in (self.obs, self.dist_adj, self.channels) if b is not None], saved_slot):
                b[t0:t0 + 2].copy_(keep)
        torch.cuda.synchronize(self.env.device)
        g = torch.cuda.CUDAGraph()
        self._capturing = True
        try:
            # "thread_local": the capturing thread may not make a call a capture rejects, other threads (RCCL's watchdog)
            # are not this capture's business.  The one such call this package could make - cm_env_destroy -> hipFree of a
            # garbage-collected env handle, the cause of round 2's invalidated captures - is kept out by L.capture_guard():
            # garbage is collected before the capture opens and handle destruction is deferred until it has closed.
            with L.capture_guard():
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    self._chunk(n, t0, tail)
        finally:
            self._capturing = False
        self._graphs[key] = g
        return g

    def run_chunk(self, use_graph=True, n=None, weights_synced=False):
        """n steps (default: the whole horizon H) from slot 0, filling slots 0..n-1 (+ slot n of obs / masks), then
        carrying slot n into slot 0 and advancing the sampler's Philox base by n (cm_chunk_tail, per shard): one
        persistent launch per shard where the library has a fused kernel for the shape and the engine was built with
        persistent=True; otherwise n x (policy, env) launches per shard - replayed from one hipGraph per chunk length
        with use_graph.  The graph path and the eager path produce the same trajectory slot by slot
        (tests/test_hip_ppo_parity.py)."""
        n = self.H if n is None else int(n)
        assert 1 <= n <= self.H
        if not use_graph:
            if not weights_synced:
                self.policy.sync_weights()
            self._chunk(n)
            self.span_diameters(0, n)
            return
        g = self._graphs.get((0, n, True)) or self.prepare_graph(n)
        if not weights_synced:              # in-place refresh of the weight pack the graph points at; a caller that steps
            self.policy.sync_weights()      # many chunks between optimiser steps syncs once itself (~15 us of host time)
        g.replay()
        self.span_diameters(0, n)          # a plain launch behind the replay, not a node of the graph

    def run_span(self, t0, n, use_graph=True, weights_synced=True):
        """Slots t0 .. t0+n-1 -> t0+1 .. t0+n, nothing else (no carry into slot 0, no Philox bump): what obtain_samples
        strings together.  One hipGraph per (t0, n), captured on first use and reused by every later rollout of this
        engine (the trajectory slots, the weight pack and the Philox base are fixed device addresses)."""
        if not use_graph:
            if not weights_synced:
                self.policy.sync_weights()
            self._chunk(n, t0, tail=False)
            self.span_diameters(t0, n)
            return
        g = self._graphs.get((t0, n, False)) or self.prepare_graph(n, t0, tail=False)
        if not weights_synced:
            self.policy.sync_weights()
        g.replay()
        self.span_diameters(t0, n)

    def invalidate_graphs(self):
        """Call after the policy weights were re-packed at a new address (never needed when
        parameters are updated in place: the pack buffer is rewritten, see nets.pack._WeightPack._packed)."""
        self._graphs.clear()
