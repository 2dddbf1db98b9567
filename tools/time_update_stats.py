"""What the per-step update statistics and the KL early stop cost: medians of CentralizedMAPPO.train_once with update_stats off /
on / target_kl set, the three legs alternating in one process (drift hits all alike), at the benchmark's reference epoch size
(PP map10 N=4, 64 envs, 30 000 agent-steps per epoch: the launch-bound, replayed regime) and at 4096 envs; then
cm_ppo_update_stats alone at both minibatch shapes (device events around a run of launches).

On a tree without the feature (no update_stats keyword) only the "off" leg runs: that is the parent's number.

Usage:  python tools/time_update_stats.py [--rounds 7] [--target-kl 0.02] [--shapes ref,4096] [--legs off,on,gated]

--legs selects the legs and their order within a round (a leg alone, or the order reversed, tells what of a difference is the
leg's and what is its place in the round)."""
import argparse
import inspect
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from com_marl_amd import _lib as L  # noqa: E402
from com_marl_amd import envs as E, nets  # noqa: E402
from com_marl_amd.algos import CentralizedMAPPO  # noqa: E402
from com_marl_amd.sampler import CentralizedMAOnPolicyVectorizedSampler  # noqa: E402

HAS_FEATURE = "update_stats" in inspect.signature(CentralizedMAPPO.__init__).parameters


class _Shell:                                       # what the sampler needs from the env object
    def __init__(self, batch, spec):
        self.batch, self.spec, self.bound_return = batch, spec, 0.0


def make_leg(c, n_envs, seed, dev, **switches):
    env = E.GridEnvBatch(c["scenario"], bench.env_params(c), n_envs, device=dev, seed=seed)
    spec = E.EnvSpec(E._Box(np.zeros(env.d * env.N), np.ones(env.d * env.N)), E._Discrete(5))
    torch.manual_seed(seed)
    policy = bench.make_policy("commdp", spec, env.N, dev)
    policy.set_rng(seed)
    critic = nets.CommBaseCritic(spec, n_agents=env.N, device=dev)
    algo = CentralizedMAPPO(env_spec=spec, policy=policy, baseline=critic, device=dev, max_path_length=c["max_env_steps"],
                            discount=0.99, center_adv=True, positive_adv=False, gae_lambda=0.97, policy_ent_coeff=0.1,
                            entropy_method="regularized", clip_grad_norm=7, optimization_n_minibatches=3, optimization_mini_epochs=10,
                            **switches)
    smp = CentralizedMAOnPolicyVectorizedSampler(algo, _Shell(env, spec), n_envs=n_envs)
    smp.start_worker()
    return dict(env=env, algo=algo, smp=smp, itr=0, times=[], epoch_times=[])


def epoch(leg, batch_size, dev, timed):
    paths = leg["smp"].obtain_samples(leg["itr"], batch_size=batch_size)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    leg["algo"].train_once(itr=leg["itr"], paths=paths)
    torch.cuda.synchronize(dev)
    if timed:
        leg["times"].append(time.perf_counter() - t0)
        leg["epoch_times"].append(leg["algo"].stats["EpochTime"])     # the optimiser steps alone (up to their synchronise)
    leg["itr"] += 1


def kernel_alone(P, T, N, A, dev, reps=200):
    """cm_ppo_update_stats on a [P,T] minibatch, microseconds per call (both launches), from device events."""
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(P, T, N, A, generator=g).to(dev)
    actions = torch.randint(0, A, (P, T, N), generator=g, dtype=torch.int32).to(dev)
    old_ll = (torch.randn(P, T, generator=g) * 0.1 - 6).to(dev)
    lens = torch.full((P,), T, dtype=torch.int32, device=dev)
    rows = torch.zeros(256, L.UPD_COLS, dtype=torch.float64, device=dev)
    cursor, gate = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    nb = L.lib().cm_ppo_update_stats_ws_bytes(P, T)
    ws = torch.empty(nb // 8, dtype=torch.float64, device=dev)

    def go(n):
        for _ in range(n):
            L.run("cm_ppo_update_stats", P, T, N, A, L.ptr(logits), L.ptr(actions), L.ptr(old_ll), L.ptr(lens), 0.1, 0.03, L.ptr(rows), 256,
                  L.ptr(cursor), L.ptr(gate), L.ptr(ws), nb, device=dev)
    go(20)
    out = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        a.record()
        go(reps)
        b.record()
        torch.cuda.synchronize(dev)
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--target-kl", type=float, default=0.02)
    ap.add_argument("--shapes", default="ref,4096")
    ap.add_argument("--legs", default="off,on,gated")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    dev = torch.device("cuda:0")
    c = dict(bench.CONFIGS["pp_map10"])
    shapes = {"ref": (64, 60000 * c["n_agents"] // 8), "4096": (4096, None)}
    legs_kw = {"off": {}}
    if HAS_FEATURE:
        legs_kw = {"off": dict(update_stats=False), "on": dict(update_stats=True), "gated": dict(target_kl=args.target_kl)}
        legs_kw = {k: legs_kw[k] for k in args.legs.split(",")}
    out = dict(has_feature=HAS_FEATURE, rounds=args.rounds, target_kl=args.target_kl, shapes={})
    for name in args.shapes.split(","):
        n_envs, bs = shapes[name]
        bs = bs or n_envs * c["n_agents"] * c["max_env_steps"]
        legs = {k: make_leg(c, n_envs, args.seed, dev, **kw) for k, kw in legs_kw.items()}
        for r in range(args.warmup + args.rounds):
            for leg in legs.values():
                epoch(leg, bs, dev, timed=r >= args.warmup)
        res = dict(envs=n_envs, batch_size_agent_steps=bs)
        for k, leg in legs.items():
            st = leg["algo"].stats
            res[k] = dict(train_once_ms_median=1e3 * float(np.median(leg["times"])), train_once_ms_min=1e3 * min(leg["times"]),
                          train_once_ms_max=1e3 * max(leg["times"]), steps_ms_median=1e3 * float(np.median(leg["epoch_times"])),
                          policy_steps=st.get("PolicySteps"), approx_kl=st.get("ApproxKL"), clip_fraction=st.get("ClipFraction"))
        P = -(-(st["NumTrajs"] // c["n_agents"]) // 3)
        T = int(st["MaxPathLength"])
        res["minibatch"] = dict(P=P, T=T)
        if HAS_FEATURE:
            res["kernel_alone_us"] = kernel_alone(P, T, c["n_agents"], 5, dev)
        out["shapes"][name] = res
        del legs
    print(json.dumps(out))


if __name__ == "__main__":
    main()
