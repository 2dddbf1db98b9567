"""The headline rollout kernel's env step on registers (rollout_w_kernel SHAPE 1, cm_env_pp10_dev.h): the carried persistent
launch at the benchmark's shape against stepwise two-launch stepping, long enough that every env auto-resets at least twice,
and the register budget of that instantiation on the gfx950 ISA."""
import numpy as np
import pytest

from tests import isa

HEADLINE = "_ZN2cm16rollout_w_kernelILi2ELb1ELb1ELb0ELb1ELi1E"   # <2 hops, PRE, full workgroups, no tape, CARRY, SHAPE 1>


def _run(torch, persistent, B=4096, steps=460, chunk=50):
    from com_marl_amd import envs as E, nets
    from com_marl_amd.rollout import RolloutEngine
    N = 4
    params = dict(load=2, max_env_steps=200, capture_reward=10, step_cost=0.1, rm=0, penalty=0, revisit_penalty=0.5,
                  lazy_penalty=1, grid_size=10, Rsen=1, n_agents=N, n_preys=N, n_gcn_layers=2, mode="train", trRcom=9, trpl=0.0,
                  obstComplex="Easy", add_clock=0)
    env = E.GridEnvBatch("pp", params, B, device="cuda:0", seed=5, env_id_offset=0)
    spec = E.EnvSpec(E._Box(np.zeros(env.d * N), np.ones(env.d * N)), E._Discrete(5))
    torch.manual_seed(5)
    pol = nets.CommCategoricalMLPPolicy(spec, n_agents=N, device="cuda:0")
    pol.set_rng(5)
    eng = RolloutEngine(env, pol, steps, fused=persistent, persistent=persistent)
    eng.reset()
    if persistent:
        for t0 in range(0, steps, chunk):
            assert eng.steps_fused(t0, min(chunk, steps - t0))
    else:
        for t in range(steps):
            eng.step(t)
    torch.cuda.synchronize()
    env.check_status()
    bufs = {k: getattr(eng, k) for k in ("obs", "actions", "probs", "attn", "reward", "reward64", "done", "details",
                                         "prey_alive", "success", "path_len")}
    out = {k: v.cpu().numpy() for k, v in bufs.items() if v is not None}
    out["state"] = env.get_state()
    return out


# 4096: the benchmark's batch, every workgroup full.  209 = 13 * 16 + 1: the ragged build, whose last wave has a single live
# group beside three idle ones (their lanes leave the step early: nothing the live group computes may depend on them).
@pytest.mark.gpu
@pytest.mark.parametrize("B", [4096, 209], ids=["full", "ragged"])
def test_headline_persistent_rollout_matches_stepwise_launches_across_resets(B):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need the MI355X")
    a = _run(torch, True, B=B)
    b = _run(torch, False, B=B)
    # every env finished an episode at least twice inside the window (200-step limit or all preys captured)
    assert (b["done"].sum(axis=0) >= 2).all()
    for k in sorted(b):
        if k == "state":
            for kk in b[k]:
                np.testing.assert_array_equal(a[k][kk], b[k][kk], err_msg=f"state.{kk}")
        else:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_headline_rollout_kernel_has_no_scratch_and_no_vgpr_spill():
    k = isa.kernel(isa.listing("cm_rollout_w"), HEADLINE)
    assert k.private_segment_fixed_size == 0
    assert k.vgpr_spill_count == 0
