"""Multi-policy rollouts on one MI355X:
  1. per-step time of cm_rollout_chunk (one policy) and of cm_rollout_chunk_multi with K in {1, 4, 64, 256} policies, PP map10,
     4096 envs, 50-step chunks (HIP events around back-to-back chunks, tails included, after warm-up; the list is run twice);
  2. wall time of eval_models (K = 64, 64 episodes each, one 4096-env wrapper) against 64 sequential eval_model calls on 64-env
     wrappers, with the two results compared;
  3. (`co`) the loop form on Coverage map20 (teams of 24, 2048 envs): per-step time of one policy and of a PolicySet with K in
     {1, 4, 16, 64} equal groups - every member's forward in one cm_policy_forward_multi launch where the library has it, else
     one cm_policy_forward per member - 50-step chunks, stepped eagerly and replayed from a hipGraph, the list run twice; and
     the wall time of eval_models_co with K = 16;
  4. (`obsdp`, `cent`) the loop form with Obs-DP / CENT policies on PP map10 (teams of 4, 4096 envs): per-step time of one policy
     and of a PolicySet with K in {1, 4, 16, 64} equal groups - every member's forward in one cm_mlp_policy_forward_multi launch
     where the library has it, else one cm_mlp_policy_forward per member - 50-step chunks, eager and from a hipGraph, the list
     run twice; and the wall time of eval_models with K = 16.
`python tools/multi_policy_time.py [pp|co|obsdp|cent]` runs one part, no argument all of them."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from com_marl_amd import envs as E, nets  # noqa: E402
from com_marl_amd.evaluate import eval_model, eval_models, eval_models_co  # noqa: E402
from com_marl_amd.rollout import RolloutEngine  # noqa: E402

B, H, REPS = 4096, 50, 20
PARAMS = dict(load=2, max_env_steps=200, capture_reward=10, step_cost=0.1, rm=0, penalty=0, grid_size=10, Rsen=1, n_agents=4,
              n_preys=4, n_gcn_layers=2, mode="train", trRcom=9, trpl=0)


def policies(d, K):
    spec = E.EnvSpec(E._Box(np.zeros(4 * d), np.ones(4 * d)), E._Discrete(5))
    out = []
    for k in range(K):
        torch.manual_seed(k)
        p = nets.CommCategoricalMLPPolicy(spec, n_agents=4, device="cuda:0")
        p.set_rng(3)
        out.append(p)
    return out


def per_step_us(eng):
    eng.policy.sync_weights()
    eng.reset()
    for _ in range(3):
        assert eng.steps_fused(0, H, tail=True)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        eng.steps_fused(0, H, tail=True)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (REPS * H)


CO_B = 2048
CO_PARAMS = dict(load=2, max_env_steps=50, capture_reward=2, step_cost=0, rm=0, penalty=1, revisit_penalty=0.5, lazy_penalty=1,
                 grid_size=20, Rsen=2, n_agents=24, n_preys=0, n_gcn_layers=2, mode="train", trRcom=9, trpl=0)


def loop_step_us(eng, use_graph):
    """Per-step time of H-step chunks of the loop form: REPS chunks between two HIP events, after two warm-up chunks."""
    eng.policy.sync_weights()
    eng.reset()
    for _ in range(2):
        eng.run_chunk(use_graph=use_graph, weights_synced=True)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        eng.run_chunk(use_graph=use_graph, weights_synced=True)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (REPS * H)


def co_main():
    env = E.GridEnvBatch("co", CO_PARAMS, CO_B, device="cuda:0", seed=3)
    spec = E.EnvSpec(E._Box(np.zeros(env.N * env.d), np.ones(env.N * env.d)), E._Discrete(5))
    pols = []
    for k in range(64):
        torch.manual_seed(k)
        p = nets.CommCategoricalMLPPolicy(spec, n_agents=env.N, device="cuda:0")
        p.set_rng(3)
        pols.append(p)
    engines = [("one policy", RolloutEngine(env, pols[0], H))]
    for K in (1, 4, 16, 64):
        engines.append((f"PolicySet, K={K}", RolloutEngine(env, nets.PolicySet(pols[:K]), H, groups=[CO_B // K] * K)))
    for rep in range(2):
        for name, eng in engines:
            eager, graph = loop_step_us(eng, False), loop_step_us(eng, True)
            print(f"[{rep}] co_map20 {name:18s} forward={getattr(eng, 'multi_forward', None) or '-':6s} eager {eager:8.2f}  graph {graph:8.2f} "
                  f"us per step ({CO_B} envs, {H}-step chunks)", flush=True)
    del engines

    K, EP, T = 16, CO_B // 16, 50
    wrap = lambda: E.CoverageWrapper(True, params=CO_PARAMS, n_envs=K * EP, device="cuda:0", seed=3)  # noqa: E731
    eval_models_co(wrap(), pols[:K], 0, n_eval_episodes=EP, max_env_steps=T)             # warm-up on a wrapper of its own
    for rep in range(2):
        w = wrap()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eval_models_co(w, pols[:K], 0, n_eval_episodes=EP, max_env_steps=T)
        print(f"[{rep}] eval_models_co K={K} x {EP} episodes ({T} steps, {K * EP} envs): {time.perf_counter() - t0:.3f} s", flush=True)


def mlp_main(kind):
    env = E.GridEnvBatch("pp", PARAMS, B, device="cuda:0", seed=3)
    spec = E.EnvSpec(E._Box(np.zeros(env.N * env.d), np.ones(env.N * env.d)), E._Discrete(5))
    cls = nets.DecCategoricalMLPPolicy if kind == "obsdp" else nets.CentralizedCategoricalMLPPolicy
    pols = []
    for k in range(64):
        torch.manual_seed(k)
        p = cls(spec, n_agents=env.N, device="cuda:0")
        p.set_rng(3)
        pols.append(p)
    engines = [("one policy", RolloutEngine(env, pols[0], H))]
    for K in (1, 4, 16, 64):
        engines.append((f"PolicySet, K={K}", RolloutEngine(env, nets.PolicySet(pols[:K]), H, groups=[B // K] * K)))
    for rep in range(2):
        for name, eng in engines:
            eager, graph = loop_step_us(eng, False), loop_step_us(eng, True)
            print(f"[{rep}] pp_map10 {kind:5s} {name:18s} forward={getattr(eng, 'multi_forward', None) or '-':6s} eager {eager:8.2f}  "
                  f"graph {graph:8.2f} us per step ({B} envs, {H}-step chunks)", flush=True)
    del engines

    K, EP, T = 16, B // 16, 50
    wrap = lambda: E.PredatorPreyWrapper(True, params=PARAMS, n_envs=K * EP, device="cuda:0", seed=3)  # noqa: E731
    eval_models(wrap(), pols[:K], 0, n_eval_episodes=EP, max_env_steps=T)                # warm-up on a wrapper of its own
    for rep in range(2):
        w = wrap()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eval_models(w, pols[:K], 0, n_eval_episodes=EP, max_env_steps=T)
        print(f"[{rep}] eval_models {kind} K={K} x {EP} episodes ({T} steps, {K * EP} envs): {time.perf_counter() - t0:.3f} s", flush=True)


def main():
    env = E.GridEnvBatch("pp", PARAMS, B, device="cuda:0", seed=3)
    pols = policies(env.d, 256)
    engines = [("cm_rollout_chunk, 1 policy", RolloutEngine(env, pols[0], H))]
    for K in (1, 4, 64, 256):
        eng = RolloutEngine(env, nets.PolicySet(pols[:K]), H, groups=[B // K] * K)
        assert eng.multi_form == "wave"
        engines.append((f"cm_rollout_chunk_multi, K={K}", eng))
    for rep in range(2):
        for name, eng in engines:
            print(f"[{rep}] {name:32s} {per_step_us(eng):7.2f} us per step ({B} envs, {H}-step chunks)", flush=True)
    del engines

    K, EP = 64, 64
    wrap = lambda n, off: E.PredatorPreyWrapper(True, params=PARAMS, n_envs=n, device="cuda:0", seed=3, env_id_offset=off)  # noqa: E731
    # warm-ups on wrappers of their own: an env's episode streams advance with every evaluation it plays, so the timed calls
    # get fresh wrappers and must then return the same results
    eval_models(wrap(K * EP, 0), pols[:K], 0, n_eval_episodes=EP)
    big = wrap(K * EP, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    multi = eval_models(big, pols[:K], 0, n_eval_episodes=EP)
    t_multi = time.perf_counter() - t0
    eval_model(wrap(EP, 0), pols[0], 0, n_eval_episodes=EP)
    small = [wrap(EP, k * EP) for k in range(K)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    seq = [eval_model(small[k], pols[k], 0, n_eval_episodes=EP) for k in range(K)]
    t_seq = time.perf_counter() - t0
    print(f"eval_models K={K} x {EP} episodes (200 steps): {t_multi:.3f} s; 64 sequential eval_model calls: {t_seq:.3f} s "
          f"({t_seq / t_multi:.1f}x); results identical: {multi == seq}", flush=True)


if __name__ == "__main__":
    part = sys.argv[1] if len(sys.argv) > 1 else "all"
    if part in ("pp", "all"):
        main()
    if part in ("co", "all"):
        co_main()
    for kind in ("obsdp", "cent"):
        if part in (kind, "all"):
            mlp_main(kind)
