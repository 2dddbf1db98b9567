"""The draw stage of the map-10 rollout builds (rollout_w_kernel<.., 1>): one 64-lane Philox call on every even step
of a chunk leaves the action words and the prey trial words of TWO steps in LDS, where the policy tile and the env step pick them
up.  The single-step launches (the generic build) keep one Philox call per draw and step, so chunked launches are compared with
them bit for bit: every trajectory buffer, and the env handle's state after EACH chunk.

Chunk lengths 1, 2, 3 and 7: odd and even lengths, an unread second half, and a launch boundary at an odd offset, so that the
pairing by the loop index, the env's rng_step and the sampler's Philox base all cross it.  max_env_steps = 5: every env resets
inside a chunk, and the rng_step a pair was drawn for has to survive the reset.  The sampler's Philox base is non-zero."""
import functools

import numpy as np
import pytest

STEPS = 10
BASE = 5                                                    # the sampler's Philox base in front of the first step
BUFS = ("obs", "actions", "probs", "attn", "reward", "reward64", "done", "details", "prey_alive", "success", "path_len")


@functools.lru_cache(maxsize=None)
def _run(chunks, B, hops):
    """Trajectory buffers after the 10 steps and the env state behind every chunk; chunks None: single-step launches, the state
    behind every step."""
    import torch
    from com_marl_amd import envs as E, nets
    from com_marl_amd.rollout import RolloutEngine
    N = 4
    params = dict(load=2, max_env_steps=5, capture_reward=10, step_cost=0.1, rm=0, penalty=0, revisit_penalty=0.5,
                  lazy_penalty=1, grid_size=10, Rsen=1, n_agents=N, n_preys=N, n_gcn_layers=hops, mode="train", trRcom=9, trpl=0.0,
                  obstComplex="Easy", add_clock=0)
    env = E.GridEnvBatch("pp", params, B, device="cuda:0", seed=29, env_id_offset=0)
    spec = E.EnvSpec(E._Box(np.zeros(env.d * N), np.ones(env.d * N)), E._Discrete(5))
    torch.manual_seed(29)
    pol = nets.CommCategoricalMLPPolicy(spec, n_agents=N, n_gcn_layers=hops, device="cuda:0")
    pol.set_rng(29)
    eng = RolloutEngine(env, pol, STEPS, fused=True, persistent=chunks is not None)
    eng.reset()
    eng.bump(BASE)
    states, t0 = [], 0
    for n in chunks or (1,) * STEPS:
        if chunks is not None:
            assert eng.steps_fused(t0, n)
        else:
            eng.step(t0)
        t0 += n
        torch.cuda.synchronize()
        env.check_status()
        states.append(env.get_state())
    assert t0 == STEPS
    assert int(eng.step_base.item()) == BASE
    out = {k: getattr(eng, k).cpu().numpy() for k in BUFS}
    for v in out.values():
        v.setflags(write=False)
    return out, states


# 16: one full workgroup.  19: the ragged build (one full workgroup, one with three live groups).
@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [(3, 7), (1, 2, 7), (7, 3)])
@pytest.mark.parametrize("hops", [1, 2])
@pytest.mark.parametrize("B", [16, 19])
def test_chunked_draws_equal_single_step_draws(B, hops, chunks):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need the MI355X")
    a, sa = _run(chunks, B, hops)
    b, sb = _run(None, B, hops)
    assert b["done"][4].all() and b["done"][9].all(), "every env resets behind its fifth step, inside a chunk"
    assert not np.array_equal(b["attn"][0], b["attn"][STEPS - 1]), "the rollout did not move"
    assert len(np.unique(b["actions"])) > 1, "the sampler drew one action only"
    for k in BUFS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    t = 0
    for i, n in enumerate(chunks):
        t += n
        x, y = sa[i], sb[t - 1]
        assert sorted(x) == sorted(y)
        for kk in sorted(y):
            np.testing.assert_array_equal(x[kk], y[kk], err_msg=f"state.{kk} after chunk {i} ({n} steps, step {t})")
