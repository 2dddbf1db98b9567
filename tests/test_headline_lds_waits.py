"""The lean policy tile with its first layer requested one step ahead ("no wait that drains a look-ahead batch"): the
carried SHAPE 1 launches against the same steps as single-step launches of the same engine (the generic body, whose tile reads
everything where it always did) - every trajectory buffer, and the env handle's state behind EVERY chunk, bit for bit.

What the chunk sequences reach: a launch whose only step is step 0 (its first-layer request is the one behind the staging
barrier) and whose request in the env phase is the discarded one; launches that start on even and on odd steps of the run while
the loop index, which alone decides where the draw stage runs, starts at 0 every time; chunks of odd and of even length, so the
last (discarded) request falls on either kind of step.  max_env_steps = 5: auto-resets fall inside the chunks.  B = 16 is one
full workgroup, B = 19 the ragged build with idle groups and, in its second workgroup, three waves without an env (which request
the first layer themselves).  One and two hops; and the same tile under rollout_wm (a PolicySet of two members, one
cm_rollout_chunk_multi launch per chunk) against its members' single-step launches."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEQS = ((1, 2, 3, 7), (7, 3, 2, 1))
STEPS = 13
BUFS = ("obs", "actions", "probs", "attn", "reward", "reward64", "done", "details", "prey_alive", "success", "path_len")


def _params(hops):
    return dict(load=2, max_env_steps=5, capture_reward=10, step_cost=0.1, rm=0, penalty=0, revisit_penalty=0.5, lazy_penalty=1,
                grid_size=10, Rsen=1, n_agents=4, n_preys=4, n_gcn_layers=hops, mode="train", trRcom=9, trpl=0.0,
                obstComplex="Easy", add_clock=0)


def _policy(env, hops, seed):
    import torch
    from com_marl_amd import envs as E, nets
    spec = E.EnvSpec(E._Box(np.zeros(env.d * 4), np.ones(env.d * 4)), E._Discrete(5))
    torch.manual_seed(seed)
    pol = nets.CommCategoricalMLPPolicy(spec, n_agents=4, n_gcn_layers=hops, device="cuda:0")
    pol.set_rng(13)
    return pol


def _play(torch, eng, chunks):
    """The 13 steps as `chunks` (persistent launches), or step by step with a state snapshot at the same places (chunks of a
    non-persistent engine)."""
    eng.reset()
    states, t0 = [], 0
    for n in chunks:
        if eng._persistent:
            assert eng.steps_fused(t0, n)
        else:
            for t in range(t0, t0 + n):
                eng.step(t)
        t0 += n
        torch.cuda.synchronize()
        eng.env.check_status()
        states.append(eng.env.get_state())
    out = {k: getattr(eng, k).cpu().numpy() for k in BUFS}
    for v in out.values():
        v.setflags(write=False)
    return out, states


@functools.lru_cache(maxsize=None)
def _run(persistent, B, hops, chunks, off=0, seed=13):
    import torch
    from com_marl_amd import envs as E
    from com_marl_amd.rollout import RolloutEngine
    env = E.GridEnvBatch("pp", _params(hops), B, device="cuda:0", seed=13, env_id_offset=off)
    eng = RolloutEngine(env, _policy(env, hops, seed), STEPS, fused=True, persistent=persistent)
    assert bool(eng._persistent) == persistent
    return _play(torch, eng, chunks)


def _same(a, sa, b, sb, chunks, cols=slice(None)):
    for k in BUFS:
        np.testing.assert_array_equal(a[k][:, cols], b[k], err_msg=k)
    assert len(sa) == len(sb) == len(chunks)
    for i, (x, y) in enumerate(zip(sa, sb)):
        assert sorted(x) == sorted(y)
        for kk in sorted(y):
            np.testing.assert_array_equal(x[kk][cols], y[kk], err_msg=f"state.{kk} after chunk {i} ({chunks[i]} steps)")


@pytest.mark.parametrize("chunks", SEQS, ids=["1-2-3-7", "7-3-2-1"])
@pytest.mark.parametrize("hops", [1, 2])
@pytest.mark.parametrize("B", [16, 19])
def test_chunks_equal_single_step_launches(B, hops, chunks):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need the MI355X")
    assert sum(chunks) == STEPS
    a, sa = _run(True, B, hops, chunks)
    b, sb = _run(False, B, hops, chunks)
    assert b["done"][1:STEPS - 1].any(), "no auto-reset inside the run"
    assert not np.array_equal(b["attn"][0], b["attn"][STEPS - 1]), "the rollout did not move"
    _same(a, sa, b, sb, chunks)


@pytest.mark.parametrize("chunks", SEQS, ids=["1-2-3-7", "7-3-2-1"])
def test_policy_set_chunks_equal_its_members_single_step_launches(chunks):
    import torch
    from com_marl_amd import envs as E, nets
    from com_marl_amd.rollout import RolloutEngine
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need the MI355X")
    sizes, hops = [16, 16], 2
    env = E.GridEnvBatch("pp", _params(hops), sum(sizes), device="cuda:0", seed=13, env_id_offset=0)
    pols = [_policy(env, hops, 13 + k) for k in range(len(sizes))]
    eng = RolloutEngine(env, nets.PolicySet(pols), STEPS, groups=sizes)
    assert eng.multi_form == "wave"
    eng.policy.sync_weights()
    a, sa = _play(torch, eng, chunks)
    for k, (lo, hi) in enumerate(eng.groups):
        b, sb = _run(False, hi - lo, hops, chunks, off=lo, seed=13 + k)
        _same(a, sa, b, sb, chunks, cols=slice(lo, hi))
