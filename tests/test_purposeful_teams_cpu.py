"""Are the inputs of tests/test_purposeful_teams_env.py what their names say?  CPU only, the oracle alone (as
tests/test_acting_regimes_cpu.py does for the acting regimes): the obstacle layout the sweeping script walks on is the env's, the
scripts are deterministic, every case runs in the kernel form it names, and every case reaches the regime it is there for -
success-ended episodes, several captures in a step, a last live prey, blocked moves; full coverage and the episode after it -
where a team of uniform random actions at the same config and seed does not.  The tallies are printed per case."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import purposeful_teams as P


@pytest.mark.parametrize("grid", [10, 20, 30, 40])
@pytest.mark.parametrize("obst", ["Easy", "Hard"])
def test_free_cells_are_the_envs(grid, obst):
    """n_empty_cells is counted after the first spawn (coverage.py:228-230): the free cells less one per agent.  Over a random
    run, resets included, no agent ever stands on a cell the helper calls an obstacle."""
    N = 6 * (grid // 10) ** 2
    env = O.OracleEnv(O.make_cfg("co", 8, N, grid, 1, max_steps=12, obst=obst, rng_mode=O.RNG_PHILOX, seed=P.SEED))
    free = P.free_cells(grid, obst == "Hard")
    assert free.shape == (env.S, env.S) and int(free.sum()) - N == env.n_empty_cells
    rng = np.random.RandomState(grid)
    env.reset()
    for _ in range(30):
        assert free[env.agent_pos[..., 0], env.agent_pos[..., 1]].all()
        assert not (env.visited_dense().astype(bool) & ~free).any()
        env.step(rng.randint(0, 5, size=(env.B, env.N)).astype(np.int32))


def test_scripts_are_deterministic_and_purposeful():
    for case, script in (("pp10_l16", "chase"), ("co10_hard", "sweep")):
        env = P.make_oracle(case)
        env.reset()
        s = P.state_of(env)
        free = None if env.M else P.free_cells(env.cfg.grid, env.cfg.obst_hard)
        run = (lambda seed, p: P.chase(s, np.random.RandomState(seed), p)) if env.M else \
            (lambda seed, p: P.sweep(s, np.random.RandomState(seed), p, free))
        np.testing.assert_array_equal(run(5, 0.2), run(5, 0.2))
        assert (run(5, 0.2) != run(6, 0.2)).any()
        pure = run(5, 0.0)
        np.testing.assert_array_equal(pure, run(6, 0.0))                  # no random share: the draws do not matter
        assert pure.dtype == np.int32 and pure.min() >= 0 and pure.max() <= 4
        if env.M:       # the move shortens the distance to the nearest live prey by one, or the agent is next to it and stays
            ap, pp = s["agent_pos"], s["prey_pos"]
            d = lambda a: (np.abs(a[:, :, None, :] - pp[:, None, :, :]).sum(-1)).min(2)     # noqa: E731 (every prey is alive)
            d0, d1 = d(ap), d(ap + np.stack([P.DR[pure], P.DC[pure]], -1))
            assert ((d0 <= 1) == (pure == 4)).all() and (d1[pure != 4] == d0[pure != 4] - 1).all()
        else:           # the step leads onto a free cell (a fresh reset has unvisited cells in reach of everyone)
            ap = s["agent_pos"]
            assert (pure < 4).all() and free[ap[..., 0] + P.DR[pure], ap[..., 1] + P.DC[pure]].all()


def test_every_case_names_its_form():
    assert set(P.CASES) == set(P.PP_CASES) | set(P.CO_CASES) and len(P.CASES) == 13
    for case, c in P.CASES.items():
        assert P.env_form(c["cfg"]) == c["form"], case
    forms = {c["form"] for c in P.CASES.values()}
    assert forms == {(16, False), (32, False), (64, False), (64, True)}


@pytest.mark.parametrize("case", P.PP_CASES)
def test_pp_case_reaches_its_regime(case):
    scripted = P.play(case, scripted=True)
    random = P.play(case, scripted=False)
    print(f"\n{case}: scripted {scripted}\n{case}: random   {random}")
    P.check_pp_floors(case, scripted)
    if P.CASES[case].get("rate"):
        assert scripted["captures"] / scripted["env_steps"] >= P.RATE_RATIO * random["captures"] / random["env_steps"]


@pytest.mark.parametrize("case", P.CO_CASES)
def test_co_case_finishes(case):
    t = P.play(case, scripted=True)
    print(f"\n{case}: scripted {t}")
    P.check_co_floors(case, t)
    assert t["revisits"] > 0 and t["blocked_moves"] > 0


def test_reference_recordings_hold_the_regimes_they_are_named_for():
    """The three recordings of the reference itself (oracle/gen_golden.py) that tests/test_oracle_golden.py and
    tests/test_hip_env_parity.py replay: a map-30 hunt that ends by success and starts over, Coverage maps 20 and 40 swept to
    full coverage with the next episode begun."""
    import os
    from tests.test_oracle_golden import GOLDEN
    z = np.load(os.path.join(GOLDEN, "env_pp_map30_cap4_hunt.npz"))
    won = (z["done"] == 1) & ~z["prey_alive_info"].any(2)
    t, b = np.argwhere(won)[0]
    assert t < len(z["done"]) - 5 and z["success"][t + 1, b] == 1 and z["prey_alive"][t + 1, b].all()     # re-spawned, played on
    assert (z["details"][:, :, 0] >= 2).any() and (z["prey_alive"][:-1].sum(2) == 1).sum() >= 3
    for name, two_words in (("env_co_map20_full", False), ("env_co_map40_full", True)):
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        full = z["total_capture"][:-1, 0] + z["details"][:, 0, 0] == int(z["n_empty_cells"])
        t = int(np.flatnonzero(full)[0])
        assert z["done"][t, 0] == 1 and z["reward"][t, 0] >= 99.0 and t < len(full) - 5
        assert z["total_capture"][t + 1, 0] == 0 and z["total_capture"][-1, 0] > 0                         # the next episode runs
        assert z["visited"].shape[-1] == (42 if two_words else 22)
        if two_words:
            assert z["visited"][t, 0, :, 32:].sum() > 200                                                  # columns of the second word
