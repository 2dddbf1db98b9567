"""The ONE-HOP map-10 rollout builds (rollout_w_kernel<1, .., 1>: n_gcn_layers = 1), which share the lean policy tile of the
headline build - the two small head layers resident in AGPRs, fragment batches requested at the running layer's middle, bias reads
in front of them - and which no other test reaches.  The same construction as tests/test_headline_chunk_writeback.py: chunks of
2 and 7 steps (carried SHAPE 1 launches) against the same 9 steps as single-step launches (the generic build, whose tile is
unchanged): every trajectory buffer, and the env handle's state after EACH chunk, bit for bit.  max_env_steps = 5, so an
auto-reset falls inside the second chunk."""
import functools

import numpy as np
import pytest

CHUNKS = (2, 7)
STEPS = sum(CHUNKS)
BUFS = ("obs", "actions", "probs", "attn", "reward", "reward64", "done", "details", "prey_alive", "success", "path_len")


@functools.lru_cache(maxsize=None)
def _run(persistent, B):
    """Trajectory buffers after the 9 steps and the env state after steps 2 and 9."""
    import torch
    from com_marl_amd import envs as E, nets
    from com_marl_amd.rollout import RolloutEngine
    N = 4
    params = dict(load=2, max_env_steps=5, capture_reward=10, step_cost=0.1, rm=0, penalty=0, revisit_penalty=0.5,
                  lazy_penalty=1, grid_size=10, Rsen=1, n_agents=N, n_preys=N, n_gcn_layers=1, mode="train", trRcom=9, trpl=0.0,
                  obstComplex="Easy", add_clock=0)
    env = E.GridEnvBatch("pp", params, B, device="cuda:0", seed=13, env_id_offset=0)
    spec = E.EnvSpec(E._Box(np.zeros(env.d * N), np.ones(env.d * N)), E._Discrete(5))
    torch.manual_seed(13)
    pol = nets.CommCategoricalMLPPolicy(spec, n_agents=N, n_gcn_layers=1, device="cuda:0")
    pol.set_rng(13)
    eng = RolloutEngine(env, pol, STEPS, fused=True, persistent=persistent)
    eng.reset()
    states, t0 = [], 0
    for n in CHUNKS:
        if persistent:
            assert eng.steps_fused(t0, n)
        else:
            for t in range(t0, t0 + n):
                eng.step(t)
        t0 += n
        torch.cuda.synchronize()
        env.check_status()
        states.append(env.get_state())
    out = {k: getattr(eng, k).cpu().numpy() for k in BUFS}
    for v in out.values():
        v.setflags(write=False)
    return out, states


# 16: one full workgroup.  19: the ragged build (one full workgroup, one with three live groups).
@pytest.mark.gpu
@pytest.mark.parametrize("B", [16, 19])
def test_one_hop_chunked_rollout_equals_single_step_launches(B):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need the MI355X")
    a, sa = _run(True, B)
    b, sb = _run(False, B)
    assert b["done"][CHUNKS[0]:].any(), "no auto-reset inside the second chunk"
    assert not np.array_equal(b["attn"][0], b["attn"][STEPS - 1]), "the rollout did not move"
    for k in BUFS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for i, (x, y) in enumerate(zip(sa, sb)):
        assert sorted(x) == sorted(y)
        for kk in sorted(y):
            np.testing.assert_array_equal(x[kk], y[kk], err_msg=f"state.{kk} after chunk {i} ({CHUNKS[i]} steps)")
