"""The carried map-10 rollout build (rollout_w_kernel SHAPE 1) stores the env state arrays once per launch, from its last step,
and addresses its trajectory buffers by 32-bit step offsets from the launch's bases.  Three chunks in a row (2, 7 and 12 steps:
the 2-step chunk is the smallest launch in which a deferred write-back can go wrong, and the state a chunk leaves is what the
next one starts from) against the same 21 steps as single-step launches: every trajectory buffer, and the env handle's state
after EACH chunk, bit for bit.  max_env_steps = 5, so auto-resets fall inside every chunk but the first.
The other side of the SHAPE 1 condition - greedy actions, no probs buffer, no attention buffer - takes the generic carried
build and must equal its stepwise run just the same."""
import functools

import numpy as np
import pytest

CHUNKS = (2, 7, 12)
STEPS = sum(CHUNKS)
BUFS = ("obs", "actions", "probs", "attn", "reward", "reward64", "done", "details", "prey_alive", "success", "path_len")


@functools.lru_cache(maxsize=None)
def _run(persistent, B, greedy=False, store_probs=True, store_attn=True):
    """Trajectory buffers after the 21 steps and the env state after steps 2, 9 and 21."""
    import torch
    from com_marl_amd import envs as E, nets
    from com_marl_amd.rollout import RolloutEngine
    N = 4
    params = dict(load=2, max_env_steps=5, capture_reward=10, step_cost=0.1, rm=0, penalty=0, revisit_penalty=0.5,
                  lazy_penalty=1, grid_size=10, Rsen=1, n_agents=N, n_preys=N, n_gcn_layers=2, mode="train", trRcom=9, trpl=0.0,
                  obstComplex="Easy", add_clock=0)
    env = E.GridEnvBatch("pp", params, B, device="cuda:0", seed=11, env_id_offset=0)
    spec = E.EnvSpec(E._Box(np.zeros(env.d * N), np.ones(env.d * N)), E._Discrete(5))
    torch.manual_seed(11)
    pol = nets.CommCategoricalMLPPolicy(spec, n_agents=N, device="cuda:0")
    pol.set_rng(11)
    eng = RolloutEngine(env, pol, STEPS, fused=True, persistent=persistent, store_probs=store_probs, store_attn=store_attn)
    eng.reset()
    states, t0 = [], 0
    for n in CHUNKS:
        if persistent:
            assert eng.steps_fused(t0, n, greedy=greedy)
        else:
            for t in range(t0, t0 + n):
                eng.step(t, greedy=greedy)
        t0 += n
        torch.cuda.synchronize()
        env.check_status()
        states.append(env.get_state())
    out = {k: getattr(eng, k).cpu().numpy() for k in BUFS if getattr(eng, k) is not None}
    for v in out.values():
        v.setflags(write=False)
    return out, states


def _compare(B, **kw):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need the MI355X")
    a, sa = _run(True, B, **kw)
    b, sb = _run(False, B, **kw)
    assert b["done"][:CHUNKS[0] + CHUNKS[1]].any() and b["done"][CHUNKS[0] + CHUNKS[1]:].any(), "no auto-reset inside the chunks"
    assert sorted(a) == sorted(b)
    for k in sorted(b):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for i, (x, y) in enumerate(zip(sa, sb)):
        for kk in sorted(y):
            np.testing.assert_array_equal(x[kk], y[kk], err_msg=f"state.{kk} after chunk {i} ({CHUNKS[i]} steps)")
    return a


# 16: one full workgroup.  19: the ragged build (one full workgroup, one with three live groups and thirteen idle ones, which
# never write).  64: four workgroups.
@pytest.mark.gpu
@pytest.mark.parametrize("B", [16, 19, 64])
def test_chunked_rollout_equals_single_step_launches_state_after_each_chunk(B):
    a = _compare(B)
    assert set(BUFS) <= set(a)


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(greedy=True), dict(store_probs=False), dict(store_attn=False)],
                         ids=["greedy", "no_probs", "no_attn"])
def test_handles_outside_the_map10_condition_equal_single_step_launches(kw):
    a = _compare(16, **kw)
    assert ("probs" in a) == kw.get("store_probs", True) and ("attn" in a) == kw.get("store_attn", True)
