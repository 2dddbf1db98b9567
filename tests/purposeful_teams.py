"""Scripted teams that play with a purpose, for judging the env step where a trained policy takes it: the late game of
Predator-Prey (one or two preys left, several captures in a step, a team crowded into few cells, episodes ended by success in
the middle of a horizon) and the end of Coverage (full coverage, its final reward, the reset that follows).

No test and no GPU code in here: numpy and the CPU oracle only.  Actions are 0 row+1, 1 col-1, 2 row-1, 3 col+1, 4 stay, as in
oracle/gen_golden.py::chase_actions, whose two scripts chase() and sweep() restate, vectorised over [B, N].

  chase / sweep     the scripts, on a state dict (state_of)
  free_cells        the Coverage obstacle layout (cm_env.hip:99), restated
  tally             per-step counts of the event classes the tests put floors under (a final-reward step is the one the env flags in
                    details[5]: final_reward less the step's own penalties can fall below final_reward)
  CASES             one entry per env form (env_form restates the rules of cm_env.hip:227 and :296)
  play              one case through the oracle - alone, or in lockstep with a second env that assert_same compares each step
  dense_start       late-game states for the rollout kernels, which no script can drive (DENSE: the cases)
"""
import functools

import numpy as np

from oracle import oracle as O

DR = np.array([1, 0, -1, 0, 0])
DC = np.array([0, -1, 0, 1, 0])
SEED = 1234
FAR = 1 << 20


# --------------------------------------------------------------------------------------------------------------------------
# the scripts
# --------------------------------------------------------------------------------------------------------------------------
def state_of(env):
    """What the scripts and tally() read, copied out of an OracleEnv-shaped object."""
    s = dict(agent_pos=np.array(env.agent_pos, np.int64))
    if env.M:
        s["prey_pos"] = np.array(env.prey_pos, np.int64)[:, :env.M]
        s["prey_alive"] = np.array(env.prey_alive, bool)[:, :env.M]
    else:
        s["visited"] = env.visited_dense().astype(bool)
        s["total_capture"] = np.array(env.total_capture)
    return s


def chase(state, rng, p_random):
    """PP: every agent steps toward its nearest live prey (Manhattan distance, lowest index on ties) along the larger axis
    (rows on ties) and stays at distance <= 1; with probability p_random, or with no live prey, a uniform action."""
    ap, pp, alive = state["agent_pos"], state["prey_pos"], state["prey_alive"]
    B, N = ap.shape[:2]
    acts = rng.randint(0, 5, size=(B, N))
    scripted = rng.random_sample((B, N)) >= p_random
    dr = pp[:, None, :, 0] - ap[:, :, None, 0]                          # [B, N, M]
    dc = pp[:, None, :, 1] - ap[:, :, None, 1]
    dist = np.where(alive[:, None, :], np.abs(dr) + np.abs(dc), FAR)
    j = dist.argmin(axis=2)[..., None]
    d, dr, dc = (np.take_along_axis(a, j, 2)[..., 0] for a in (dist, dr, dc))
    rows = np.abs(dr) >= np.abs(dc)
    move = np.where(rows, np.where(dr > 0, 0, 2), np.where(dc > 0, 3, 1))
    want = np.where(d <= 1, 4, move)
    return np.where(scripted & (d < FAR), want, acts).astype(np.int32)


def free_cells(grid, hard):
    """CO: [S, S] bool, True where an agent can stand - the wall ring and the fixed rectangles scaled by r = m / 10 taken out
    (cm_env.hip:99 co_walls, coverage.py:44,69-80,165-168,482-500), S = m + 2."""
    S, r = grid + 2, grid // 10
    f = np.ones((S, S), bool)
    f[0, :] = f[S - 1, :] = f[:, 0] = f[:, S - 1] = False
    rects = [(2 * r + 1, 2 * r + 1, 6 * r, r), (3 * r + 1, 8 * r + 1, 4 * r, 2 * r)]
    if hard:
        rects += [(1, 2 * r + 1, r, 3 * r), (1, 7 * r + 1, 2 * r, r), (4 * r + 1, 4 * r + 1, 2 * r, 3 * r),
                  (8 * r + 1, 5 * r + 1, 2 * r, 2 * r), (8 * r + 1, 8 * r + 1, r, r)]
    for r0, c0, h, w in rects:
        f[r0:r0 + h, c0:c0 + w] = False
    return f


def _shortest_to_unvisited(passable, target):
    """[B, S, S] steps from every passable cell to the nearest target cell over passable cells (FAR: none).  The wall ring is
    never passable, so a shifted copy never carries a distance round the edge."""
    dist = np.where(target, 0, FAR)
    while True:
        near = np.minimum(np.minimum(np.roll(dist, 1, 1), np.roll(dist, -1, 1)), np.minimum(np.roll(dist, 1, 2), np.roll(dist, -1, 2)))
        new = np.where(passable, np.minimum(dist, near + 1), FAR)
        if np.array_equal(new, dist):
            return dist
        dist = new


def sweep(state, rng, p_random, free):
    """CO: every agent takes the first step (lowest action on ties) of a shortest path over free cells no agent stands on to
    the nearest unvisited cell; with probability p_random, or with no such path, a uniform action."""
    ap, visited = state["agent_pos"], state["visited"]
    B, N = ap.shape[:2]
    acts = rng.randint(0, 5, size=(B, N))
    scripted = rng.random_sample((B, N)) >= p_random
    bi = np.arange(B)[:, None]
    passable = np.broadcast_to(free, visited.shape).copy()
    passable[bi, ap[..., 0], ap[..., 1]] = False
    dist = _shortest_to_unvisited(passable, passable & ~visited)
    step = np.stack([dist[bi, ap[..., 0] + DR[a], ap[..., 1] + DC[a]] for a in range(4)], axis=2)       # [B, N, 4]
    want = step.argmin(axis=2)
    return np.where(scripted & (step.min(axis=2) < FAR), want, acts).astype(np.int32)


def uniform(state, rng):
    return rng.randint(0, 5, size=state["agent_pos"].shape[:2]).astype(np.int32)


# --------------------------------------------------------------------------------------------------------------------------
# the event classes
# --------------------------------------------------------------------------------------------------------------------------
TALLY_KEYS = ("env_steps", "captures", "multi_capture_steps", "one_prey_steps", "blocked_moves", "success_episodes",
              "final_reward_steps", "revisits", "lazy")


def tally(before, after, details, done, success, reward, cfg):
    """Counts over one env step of a batch.  before / after: state_of() around the step; details, done, success, reward: what
    the step wrote.  A blocked move is a non-stay action that left the agent in place: Coverage counts it itself (details[2]); in
    Predator-Prey it is details[1] (non-stay actions) less the agents that moved, taken over the envs that did not reset."""
    pp = cfg.scenario == O.PP
    done = np.asarray(done, bool)
    t = dict.fromkeys(TALLY_KEYS, 0)
    t["env_steps"] = len(done)
    t["captures"] = int(details[:, 0].sum())
    t["multi_capture_steps"] = int((details[:, 0] >= 2).sum())
    if pp:
        t["one_prey_steps"] = int((before["prey_alive"].sum(1) == 1).sum())
        moved = (before["agent_pos"] != after["agent_pos"]).any(2).sum(1)
        t["blocked_moves"] = int((details[:, 1] - moved)[~done].sum())
        won = done & ~after["info_alive"].any(1)
        assert (np.asarray(success)[won] == 1).all()
        t["success_episodes"] = int(won.sum())
    else:
        t["blocked_moves"] = int(details[:, 2].sum())
        fin = details[:, 5] == 1
        # the step's own penalties (at most one per agent, averaged over the team) can pull the reward just below final_reward
        assert done[fin].all() and ((np.asarray(reward) >= cfg.final_reward - 1.0) == fin).all()
        t["final_reward_steps"] = int(fin.sum())
        t["lazy"] = int(details[:, 3].sum())
        t["revisits"] = int(details[:, 4].sum())
    return t


# --------------------------------------------------------------------------------------------------------------------------
# the cases
# --------------------------------------------------------------------------------------------------------------------------
def env_form(cfg):
    """The kernel form cm_env_step launches for `cfg` (make_cfg keywords): lanes per env by the rule of cm_env.hip:227, the
    256-thread wide form by the rule of :296."""
    big = max(cfg["n_agents"], cfg.get("n_preys", 0))
    lpe = 16 if big <= 8 else (32 if big <= 32 and cfg["n_envs"] >= 8192 else 64)
    return lpe, lpe == 64 and cfg["n_envs"] <= 1536


# floors of the Predator-Prey cases (oracle tallies, scripted run)
FLOOR_SUCCESS, FLOOR_MULTI, FLOOR_ONE_PREY, FLOOR_BLOCKED, RATE_RATIO = 8, 8, 50, 50, 3.0

_PP10 = dict(scenario="pp", n_agents=4, n_preys=4, grid=10, rsen=1, load=2, max_steps=200)
_TEAM12 = dict(scenario="pp", n_agents=12, n_preys=6, grid=10, rsen=1, load=2, max_steps=40)
_CO = dict(scenario="co", max_steps=400, max_path_length=400)

# name -> cfg: make_cfg keywords; steps; every: compare every n-th step and the last; form: (lanes per env, wide);
# p_random of the script; rate: the capture rate must be RATE_RATIO times the random team's (the two cases whose prey count a
# random team can also work through).  Every case meets every floor, the two short-horizon ones included
CASES = {
    # 16 lanes per env, 61 envs = 15 full waves of four envs and one ragged wave
    "pp10_l16": dict(cfg=dict(_PP10, n_envs=61), steps=120, form=(16, False), rate=True),
    "pp10_cap3": dict(cfg=dict(scenario="pp", n_envs=96, n_agents=8, n_preys=8, grid=10, rsen=1, load=3, max_steps=30), steps=70,
                      form=(16, False), rate=True),
    # the Gilbert-Elliott link state is carried across the resets a success causes
    "pp12_ge": dict(cfg=dict(scenario="pp", n_envs=100, n_agents=5, n_preys=7, grid=12, rsen=2, load=2, max_steps=30, rcom=3,
                             channel="GE"), steps=60, form=(16, False)),
    "pp20_iid_wide": dict(cfg=dict(scenario="pp", n_envs=61, n_agents=24, n_preys=24, grid=20, rsen=1, load=2, max_steps=40,
                                   channel="IID", ploss=0.3), steps=60, form=(64, True)),
    "pp30_wide": dict(cfg=dict(scenario="pp", n_envs=32, n_agents=72, n_preys=12, grid=30, rsen=2, load=4, max_steps=80), steps=80,
                      form=(64, True)),
    # map 40: coordinates need all six bits of their field
    "pp40_wide": dict(cfg=dict(scenario="pp", n_envs=16, n_agents=128, n_preys=16, grid=40, rsen=2, load=4, max_steps=80), steps=80,
                      form=(64, True)),
    # B > 1536 leaves the wide form: one wave per env
    "pp_narrow64": dict(cfg=dict(_TEAM12, n_envs=1600), steps=50, every=10, form=(64, False)),
    # B >= 8192 with at most 32 agents: two envs per wave
    "pp_l32": dict(cfg=dict(_TEAM12, n_envs=8192), steps=40, every=10, form=(32, False)),
    # pp10_l16 under a per-env condition table: two ranges, two loss rates (cm_env_cond.hip)
    "pp10_cond": dict(cfg=dict(_PP10, n_envs=61, channel="IID", ploss=0.1, rcom=2), steps=120, form=(16, False),
                      conditions=[dict(Rcom=2, pl=0.1), dict(Rcom=4, pl=0.5)], condition_of=[0] * 30 + [1] * 31),
    "co10": dict(cfg=dict(_CO, n_envs=16, n_agents=6, grid=10, rsen=1), steps=40, form=(16, False)),
    "co10_hard": dict(cfg=dict(_CO, n_envs=16, n_agents=6, grid=10, rsen=1, obst="Hard"), steps=40, form=(16, False)),
    "co20_wide": dict(cfg=dict(_CO, n_envs=8, n_agents=24, grid=20, rsen=2), steps=40, form=(64, True)),
    # map 40: 42 cells a side, two visited words per row
    "co40_two_words": dict(cfg=dict(_CO, n_envs=4, n_agents=96, grid=40, rsen=2, channel="IID", ploss=0.3), steps=40,
                           form=(64, True)),
}
P_RANDOM = 0.2
PP_CASES = [k for k, c in CASES.items() if c["cfg"]["scenario"] == "pp"]
CO_CASES = [k for k, c in CASES.items() if c["cfg"]["scenario"] == "co"]


class OracleSlices:
    """The oracle's way to play a condition table: one OracleEnv per run of envs with one condition, each with the
    condition's range and loss rate and the Philox env ids of its slice; attributes are the slices' joined along the batch."""
    JOINED = ("agent_pos", "prey_pos", "prey_alive", "step_count", "total_capture", "success", "ge_state", "rng_step", "agent_cond",
              "obs", "reward", "done", "details", "dist_adj", "channels", "prey_alive_info")

    def __init__(self, cfg, conditions, condition_of, rng_mode, seed):
        of = np.asarray(condition_of)
        cuts = [0] + [b for b in range(1, len(of)) if of[b] != of[b - 1]] + [len(of)]
        self.envs = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            c = conditions[of[lo]]
            self.envs.append(O.OracleEnv(O.make_cfg(**dict(cfg, n_envs=hi - lo, rcom=c["Rcom"], ploss=c["pl"]), env_id_offset=lo,
                                                    rng_mode=rng_mode, seed=seed)))
        e = self.envs[0]
        self.cfg, self.B, self.N, self.M = e.cfg, len(of), e.N, e.M
        self._join()

    def _join(self):
        for k in self.JOINED:
            setattr(self, k, np.concatenate([getattr(e, k) for e in self.envs]))

    def reset(self):
        for e in self.envs:
            e.reset()
        self._join()

    def step(self, actions, n_threads=1):
        lo = 0
        for e in self.envs:
            e.step(actions[lo:lo + e.B], n_threads=n_threads)
            lo += e.B
        self._join()

    def load_state(self, **arrays):
        lo = 0
        for e in self.envs:
            e.load_state(**{k: v[lo:lo + e.B] for k, v in arrays.items()})
            lo += e.B
        self._join()


def make_oracle(case, seed=SEED):
    c = CASES[case] if case in CASES else DENSE[case]
    if c.get("conditions"):
        return OracleSlices(c["cfg"], c["conditions"], c["condition_of"], O.RNG_PHILOX, seed)
    return O.OracleEnv(O.make_cfg(**c["cfg"], rng_mode=O.RNG_PHILOX, seed=seed))


STATE_KEYS = ("agent_pos", "visited", "step_count", "total_capture", "success", "ge_state", "rng_step")


@functools.lru_cache(maxsize=None)
def near_complete_snapshot(case, seed=SEED):
    """CO: the oracle alone under sweep() until every env has total_capture >= n_empty_cells - 3 N; every env's whole state is
    taken at the first step it got there (an env's state is its own rows, its Philox step included), so that no env finishes
    and starts over while the slower ones catch up."""
    env = make_oracle(case, seed)
    env.reset()
    rng = np.random.RandomState(seed)
    free = free_cells(env.cfg.grid, env.cfg.obst_hard)
    snap = {k: np.array(getattr(env, k)) for k in STATE_KEYS}
    have = np.zeros(env.B, bool)
    for _ in range(env.cfg.max_steps - CASES[case]["steps"] - 1):
        env.step(sweep(state_of(env), rng, P_RANDOM, free), n_threads=8)
        assert not env.done.any(), "an env ended before it reached the snapshot"
        new = ~have & (env.total_capture >= env.n_empty_cells - 3 * env.N)
        for k in STATE_KEYS:
            snap[k][new] = getattr(env, k)[new]
        have |= new
        if have.all():
            return snap
    raise AssertionError(f"{case}: {int((~have).sum())} envs did not come near full coverage")


def assert_same(eh, eo, where):
    """test_hip_env_parity._lockstep's comparison, field for field, all exact."""
    w = where
    np.testing.assert_array_equal(eh.done, eo.done, err_msg=w)
    np.testing.assert_array_equal(eh.reward, eo.reward, err_msg=w)
    np.testing.assert_array_equal(eh.reward32, eo.reward.astype(np.float32), err_msg=w)
    np.testing.assert_array_equal(eh.details, eo.details, err_msg=w)
    np.testing.assert_array_equal(eh.agent_pos, eo.agent_pos, err_msg=w)
    np.testing.assert_array_equal(eh.step_count, eo.step_count, err_msg=w)
    np.testing.assert_array_equal(eh.success, eo.success, err_msg=w)
    np.testing.assert_array_equal(eh.rng_step, eo.rng_step, err_msg=w)
    if eo.M:
        alive = eo.prey_alive.astype(bool)
        np.testing.assert_array_equal(eh.prey_alive.astype(bool), alive, err_msg=w)
        np.testing.assert_array_equal(eh.prey_pos[alive], eo.prey_pos[alive], err_msg=w)
        np.testing.assert_array_equal(eh.prey_alive_info, eo.prey_alive_info[:, :eo.M], err_msg=w)
    else:
        np.testing.assert_array_equal(eh.visited, eo.visited, err_msg=w)
        np.testing.assert_array_equal(eh.total_capture, eo.total_capture, err_msg=w)
    np.testing.assert_array_equal(eh.obs, eo.obs, err_msg=w)
    np.testing.assert_array_equal(eh.dist_adj, eo.dist_adj, err_msg=w)
    np.testing.assert_array_equal(eh.channels, eo.channels, err_msg=w)
    if eo.cfg.channel == O.CH["GE"]:
        np.testing.assert_array_equal(eh.ge_state, eo.ge_state, err_msg=w)


def play(case, scripted=True, other=None, seed=SEED):
    """`case` through the oracle on the Philox stream: a reset (CO: then the near-complete snapshot loaded), then its steps with
    actions from the script - or uniform ones - computed on the oracle's state.  other: a second env with the OracleEnv face
    that takes the same calls and is compared with assert_same every c['every']-th step and the last.  ->
    the oracle's tallies summed over the window, plus for CO 'finished' (envs that had a final-reward step) and 'went_on'
    (those of them that were stepped again after the reset it causes)."""
    c = CASES[case]
    eo = make_oracle(case, seed)
    pp = bool(eo.M)
    envs = [eo] + ([other] if other is not None else [])
    for e in envs:
        e.reset()
    if not pp:
        snap = near_complete_snapshot(case, seed)
        for e in envs:
            e.load_state(**snap)
    rng = np.random.RandomState(seed + 1)
    free = None if pp else free_cells(eo.cfg.grid, eo.cfg.obst_hard)
    total = dict.fromkeys(TALLY_KEYS, 0)
    finished = np.zeros(eo.B, bool)
    went_on = np.zeros(eo.B, bool)
    steps, every = c["steps"], c.get("every", 1)
    for t in range(steps):
        before = state_of(eo)
        if not scripted:
            a = uniform(before, rng)
        else:
            a = chase(before, rng, P_RANDOM) if pp else sweep(before, rng, P_RANDOM, free)
        went_on |= finished
        for e in envs:
            e.step(a, n_threads=8)
        if other is not None and (t % every == 0 or t == steps - 1):
            assert_same(other, eo, f"{case} step {t}")
        after = state_of(eo)
        if pp:
            after["info_alive"] = np.array(eo.prey_alive_info, bool)[:, :eo.M]
        for k, v in tally(before, after, eo.details, eo.done, eo.success, eo.reward, eo.cfg).items():
            total[k] += v
        if not pp:
            finished |= eo.details[:, 5] == 1
    if not pp:
        total["finished"], total["went_on"] = int(finished.sum()), int((finished & went_on).sum())
    return total


def check_pp_floors(case, t):
    """The floors of tests/test_purposeful_teams_cpu.py on a scripted run's tallies (the rate against the random team is that
    test's alone: it needs the second run)."""
    assert t["success_episodes"] >= FLOOR_SUCCESS, (case, t)
    assert t["multi_capture_steps"] >= FLOOR_MULTI, (case, t)
    assert t["one_prey_steps"] >= FLOOR_ONE_PREY, (case, t)
    assert t["blocked_moves"] >= FLOOR_BLOCKED, (case, t)


def check_co_floors(case, t):
    B = CASES[case]["cfg"]["n_envs"]
    assert 2 * t["finished"] >= B, (case, t)
    assert t["went_on"] >= 1, (case, t)


# --------------------------------------------------------------------------------------------------------------------------
# dense starts: late-game states for the rollout kernels, which take their actions from the policy and not from a script
# --------------------------------------------------------------------------------------------------------------------------
_COND = dict(channel="IID", ploss=0.1, rcom=2, conditions=[dict(Rcom=2, pl=0.1), dict(Rcom=4, pl=0.5)])
DENSE = {
    "headline_full": dict(cfg=dict(_PP10, n_envs=64)),                   # four full workgroups of 16 envs
    "headline_ragged": dict(cfg=dict(_PP10, n_envs=209)),                # 13 * 16 + 1: the ragged build
    "cond_full": dict(cfg=dict(_PP10, n_envs=64, **{k: _COND[k] for k in ("channel", "ploss", "rcom")}),
                      conditions=_COND["conditions"], condition_of=[0] * 32 + [1] * 32),
    "cond_ragged": dict(cfg=dict(_PP10, n_envs=209, **{k: _COND[k] for k in ("channel", "ploss", "rcom")}),
                        conditions=_COND["conditions"], condition_of=[0] * 100 + [1] * 109),
    "set_of_two": dict(cfg=dict(_PP10, n_envs=64)),
    # sensing range 2: the observation width the one-launch step of mid-size Predator-Prey teams is built for (cm_fused.hip).
    # Two preys: 24 uniform agents capture 0.022 per env-step from a reset with four, and a window that starts with two of them
    # alive cannot hold four times that
    "fused_map20": dict(cfg=dict(scenario="pp", n_envs=13, n_agents=24, n_preys=2, grid=20, rsen=2, load=2, max_steps=200)),
}
DENSE_STATE = ("agent_pos", "prey_pos", "prey_alive", "step_count", "success", "ge_state", "rng_step", "agent_cond")
DENSE_OUTS = ("obs", "dist_adj", "channels")
DENSE_WINDOW = 32


def _uniform_captures(probe, rows, mc, replicas, lookahead):
    """[B] mean captures of a team of uniform random actions from the states `rows`, inside the episode they are in, over the
    next `lookahead` steps."""
    score = np.zeros(probe.B)
    for _ in range(replicas):
        probe.load_state(**{k: rows[k] for k in DENSE_STATE})
        same_episode = np.ones(probe.B, bool)
        for _ in range(lookahead):
            probe.step(mc.randint(0, 5, size=(probe.B, probe.N)).astype(np.int32), n_threads=8)
            score += probe.details[:, 0] * same_episode
            same_episode &= probe.done == 0
    return score / replicas


@functools.lru_cache(maxsize=None)
def dense_start(name, seed=SEED, steps=1600, lookahead=6, replicas=(2, 64), keep=6):
    """A mid-hunt start for every env of DENSE[name].  The oracle alone plays chase() for `steps` steps; every state it passes
    through with one or two live preys is a candidate, scored by what a team of uniform random actions - the stand-in for a
    freshly seeded net - captures from it (_uniform_captures on a second oracle): a first pass with replicas[0] continuations
    keeps the keep * B best, a second with replicas[1] picks the B best of those.  An env's state is its own rows (positions,
    alive flags, step count, success, Philox step), and any such rows are a state the env can be in, so rows of different
    steps and envs make one batch; under a condition table a candidate stays among the envs of its condition, whose range and
    loss rate its emission was made with.  -> the state rows (DENSE_STATE) and what the env emitted at that state (DENSE_OUTS),
    read-only."""
    env, probe = make_oracle(name, seed), make_oracle(name, seed)
    env.reset()
    probe.reset()
    rng, mc = np.random.RandomState(seed), np.random.RandomState(seed + 2)
    keys = DENSE_STATE + DENSE_OUTS
    of = np.asarray(DENSE[name].get("condition_of", [0] * env.B))
    groups = [np.flatnonzero(of == c) for c in np.unique(of)]
    grab = lambda: {k: np.array(getattr(env, k)) for k in keys}                       # noqa: E731
    pool = [{k: np.repeat(v[g], keep, axis=0) for k, v in grab().items()} for g in groups]
    pool_score = [np.full(keep * len(g), -1.0) for g in groups]
    for _ in range(steps):
        env.step(chase(state_of(env), rng, P_RANDOM), n_threads=8)
        now = grab()
        live = now["prey_alive"].sum(1)
        score = np.where((live >= 1) & (live <= 2), _uniform_captures(probe, now, mc, replicas[0], lookahead), -1.0)
        for i, g in enumerate(groups):                                    # the best of the kept and the new rows
            both = np.concatenate([pool_score[i], score[g]])
            top = np.argsort(-both, kind="stable")[:keep * len(g)]
            pool[i] = {k: np.concatenate([pool[i][k], now[k][g]])[top] for k in keys}
            pool_score[i] = both[top]
    assert all((ps >= 0).all() for ps in pool_score)
    fine = [np.zeros(keep * len(g)) for g in groups]
    for j in range(keep):                                                 # second pass: a batch holds one share of every pool
        rows = {k: np.concatenate([pool[i][k][j::keep] for i in range(len(groups))]) for k in DENSE_STATE}
        got = _uniform_captures(probe, rows, mc, replicas[1], lookahead)
        lo = 0
        for i, g in enumerate(groups):
            fine[i][j::keep] = got[lo:lo + len(g)]
            lo += len(g)
    best = {}
    for k in keys:
        best[k] = np.concatenate([pool[i][k][np.argsort(-fine[i], kind="stable")[:len(g)]] for i, g in enumerate(groups)])
        best[k].setflags(write=False)
    return best
