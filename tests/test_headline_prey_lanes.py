"""The prey trials of the map-10 rollout builds (rollout_w_kernel<.., 1>, pp10::step): lane sl of an env's 16-lane
group runs trial sl >> 2 of prey sl & 3, and lane j takes the first passing one of its prey's four over row-shift DPP moves; the
generic env body, which the single-step launches run, keeps prey j's trials one after the other in lane j.  Chunked launches are
compared with single-step launches bit for bit: every trajectory buffer, and the env handle's state after EACH chunk.

Structural cases: B = 16 (one full workgroup) and 19 (the ragged build), one and two hops, chunks (3, 7) and (7, 3),
max_env_steps = 5 (every env resets inside a chunk).

Coverage case: the combine has six outcomes per prey and step - first passing trial 0, 1, 2, 3, no trial at all (the prey is dead
or captured this step), the fifth draw - and a small batch does not reach the late ones.  A numpy restatement of the trial rule
(words from oracle.philox) runs over the states the SINGLE-STEP run recorded, classifies every prey-step, and is itself held
against that run: the prey positions and alive flags it predicts are the ones recorded behind the step.  Prey-steps of envs that
reset in the step are left out of the counts (the state behind the step is the respawn), never out of the comparison of the two
runs.  B and the step count were sized on the CPU with the oracle's port of the rollout (env step + policy forward + sampler), which
draws the same stream: B = 32 needs 14 steps to meet the counts asked below (trial 3 is the last to get there: 9 at 13 steps), B = 16
needs 40 and B = 48 still 8; 32 x 14 is the fewest env-steps of the three.  With 200-step episodes no env resets in 14 steps.

Counts seen on the MI355X (and by the CPU port, which draws the same stream): first passing trial 0 1 627 times, trial 1 87,
trial 2 30, trial 3 11, no trial 23, the fifth draw 14, of 1 792 prey-steps; none left out."""
import functools

import numpy as np
import pytest

BASE = 5                                                    # the sampler's Philox base in front of the first step
SEED = 29
BUFS = ("obs", "actions", "probs", "attn", "reward", "reward64", "done", "details", "prey_alive", "success", "path_len")
N = M = 4
GRID = 10
COV_B, COV_STEPS, COV_CHUNKS = 32, 14, (5, 9)
NONE, FIFTH = 4, 5                                          # outcome classes next to "first passing trial 0 .. 3"
DR = np.array([1, 0, -1, 0, 0])                             # 0 down, 1 left, 2 up, 3 right, 4 stay (predator_prey.py:244-253)
DC = np.array([0, -1, 0, 1, 0])
THRESHOLDS = (751619276, 1503238553, 2254857830, 3006477107)   # floor(cdf * 2^32), cdf = .175 .35 .525 .7 (predator_prey.py:401)
SITE_PREY = 2


@functools.lru_cache(maxsize=None)
def _run(chunks, B, hops, steps, max_env_steps):
    """Trajectory buffers after `steps` steps, the env state behind every chunk, and the state in front of the first step;
    chunks None: single-step launches, the state behind every step."""
    import torch
    from com_marl_amd import envs as E, nets
    from com_marl_amd.rollout import RolloutEngine
    params = dict(load=2, max_env_steps=max_env_steps, capture_reward=10, step_cost=0.1, rm=0, penalty=0, revisit_penalty=0.5,
                  lazy_penalty=1, grid_size=GRID, Rsen=1, n_agents=N, n_preys=M, n_gcn_layers=hops, mode="train", trRcom=9,
                  trpl=0.0, obstComplex="Easy", add_clock=0)
    env = E.GridEnvBatch("pp", params, B, device="cuda:0", seed=SEED, env_id_offset=0)
    spec = E.EnvSpec(E._Box(np.zeros(env.d * N), np.ones(env.d * N)), E._Discrete(5))
    torch.manual_seed(SEED)
    pol = nets.CommCategoricalMLPPolicy(spec, n_agents=N, n_gcn_layers=hops, device="cuda:0")
    pol.set_rng(SEED)
    eng = RolloutEngine(env, pol, steps, fused=True, persistent=chunks is not None)
    eng.reset()
    eng.bump(BASE)
    torch.cuda.synchronize()
    first = env.get_state()
    states, t0 = [], 0
    for n in chunks or (1,) * steps:
        if chunks is not None:
            assert eng.steps_fused(t0, n)
        else:
            eng.step(t0)
        t0 += n
        torch.cuda.synchronize()
        env.check_status()
        states.append(env.get_state())
    assert t0 == steps
    out = {k: getattr(eng, k).cpu().numpy() for k in BUFS}
    for v in out.values():
        v.setflags(write=False)
    return out, states, first


def _assert_same(a, sa, b, sb, chunks):
    for k in BUFS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    t = 0
    for i, n in enumerate(chunks):
        t += n
        x, y = sa[i], sb[t - 1]
        assert sorted(x) == sorted(y)
        for kk in sorted(y):
            np.testing.assert_array_equal(x[kk], y[kk], err_msg=f"state.{kk} after chunk {i} ({n} steps, step {t})")


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [(3, 7), (7, 3)])
@pytest.mark.parametrize("hops", [1, 2])
@pytest.mark.parametrize("B", [16, 19])
def test_lane_trials_equal_serial_trials(B, hops, chunks):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need the MI355X")
    a, sa, _ = _run(chunks, B, hops, 10, 5)
    b, sb, _ = _run(None, B, hops, 10, 5)
    assert b["done"][4].all() and b["done"][9].all(), "every env resets behind its fifth step, inside a chunk"
    assert len(np.unique(b["actions"])) > 1, "the sampler drew one action only"
    assert any(not np.array_equal(sb[0]["prey_pos"], s["prey_pos"]) for s in sb[1:4]), "no prey moved"
    _assert_same(a, sa, b, sb, chunks)


def _agents_next(agents, r, c):
    """Agents at cell distance 1 from (r, c), which may lie one step outside the grid.  agents [n, N, 2], r and c [n]."""
    return ((np.abs(agents[:, :, 0] - r[:, None]) + np.abs(agents[:, :, 1] - c[:, None])) == 1).sum(1)


def _move_of(word):
    return sum(int(word) >= t for t in THRESHOLDS)


def trial_rule(agents, prey, alive, rng_step, env_ids, seed, philox):
    """One step's prey phase, load = 2 (predator_prey.py:396-432): `agents` [n, N, 2] AFTER the agents moved, `prey` [n, M, 2],
    `alive` [n, M] and `rng_step` [n] in front of the step.  Returns the outcome class of every prey [n, M] (first passing trial
    0 .. 3, NONE, FIFTH) and the prey positions / alive flags behind the step (no reset)."""
    n = len(agents)
    cls = np.full((n, M), NONE)
    mv = np.full((n, M), 4)
    cnt = np.stack([_agents_next(agents, prey[:, j, 0], prey[:, j, 1]) for j in range(M)], 1)
    key = (seed & 0xffffffff, seed >> 32)
    one = np.ones(1, int)
    for e in range(n):
        for j in range(M):
            if not alive[e, j] or cnt[e, j] >= 2:               # dead, or captured this step: no trial
                continue
            free = lambda m: _agents_next(agents[e:e + 1], one * (prey[e, j, 0] + DR[m]), one * (prey[e, j, 1] + DC[m]))[0] == 0
            words = philox((env_ids[e], rng_step[e], SITE_PREY, 2 * j), key)
            for t in range(4):                                   # the first of <= 5 draws whose target has no predator neighbour
                m = _move_of(words[t])
                if free(m):
                    cls[e, j], mv[e, j] = t, m
                    break
            else:
                m = _move_of(philox((env_ids[e], rng_step[e], SITE_PREY, 2 * j + 1), key)[0])
                cls[e, j] = FIFTH
                mv[e, j] = m if free(m) else 4
    # captures and moves in index order (:416-432, :276-301): the target must be inside, hold no agent and no live prey
    prey, live = prey.copy(), alive.astype(bool).copy()
    for j in range(M):
        stays = live[:, j] & (cnt[:, j] < 2)
        live[:, j] = stays
        r, c = prey[:, j, 0] + DR[mv[:, j]], prey[:, j, 1] + DC[mv[:, j]]
        ok = stays & (mv[:, j] != 4) & (r >= 0) & (r < GRID) & (c >= 0) & (c < GRID)
        ok &= ~((agents[:, :, 0] == r[:, None]) & (agents[:, :, 1] == c[:, None])).any(1)
        ok &= ~((prey[:, :, 0] == r[:, None]) & (prey[:, :, 1] == c[:, None]) & live).any(1)
        prey[ok, j, 0], prey[ok, j, 1] = r[ok], c[ok]
    return cls, prey, live


def outcome_counts(first, states, done, seed, philox):
    """The outcome classes over a recorded run: `states[t]` behind step t, `first` in front of step 0, `done` [T, B].  Holds the
    restatement against the recording, and returns (counts of the six classes, prey-steps left out, prey-steps in all)."""
    counts, left_out = np.zeros(6, int), 0
    prev = first
    for t, cur in enumerate(states):
        keep = done[t] == 0                                      # a resetting env's recorded state is its respawn
        ids = np.flatnonzero(keep)
        cls, prey, live = trial_rule(cur["agent_pos"][keep], prev["prey_pos"][keep], prev["prey_alive"][keep],
                                     prev["rng_step"][keep], ids, seed, philox)
        np.testing.assert_array_equal(live, cur["prey_alive"][keep] != 0, err_msg=f"alive flags behind step {t}")
        np.testing.assert_array_equal(prey[live], cur["prey_pos"][keep][live], err_msg=f"prey positions behind step {t}")
        counts += np.bincount(cls.ravel(), minlength=6)
        left_out += M * int((~keep).sum())
        prev = cur
    return counts, left_out, M * done.size


@pytest.mark.gpu
def test_every_trial_outcome_is_compared():
    import torch
    from oracle import oracle as O
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need the MI355X")
    a, sa, _ = _run(COV_CHUNKS, COV_B, 2, COV_STEPS, 200)
    b, sb, first = _run(None, COV_B, 2, COV_STEPS, 200)
    counts, left_out, total = outcome_counts(first, sb, b["done"], SEED, O.philox)
    print("outcomes (trial 0, 1, 2, 3, none, fifth):", counts.tolist(), "left out", left_out, "of", total)
    assert (counts[:4] >= 10).all() and counts[NONE] >= 10 and counts[FIFTH] >= 1, counts
    assert left_out <= 0.05 * total, (left_out, total)
    _assert_same(a, sa, b, sb, COV_CHUNKS)
