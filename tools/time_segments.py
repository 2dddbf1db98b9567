"""Whole-episode epochs against fixed-length segment epochs at bench.py's train-loop configuration (PP map10, N = 4, Comm-DP,
3 minibatches x 10 mini-epochs, 4096 envs): today's obtain_samples + train_once, and CentralizedMAPPO(segment_steps=n) for
n = 32 and 128.  Every mode has its own envs, nets and sampler; the modes take turns epoch by epoch in ONE process, so that
drift of the machine hits all alike, and the per-epoch times are reduced by their median.

Per mode: env-steps the sampler ran and env-steps that reached the update per epoch (their ratio is the kept share: a
whole-episode rollout throws the unfinished tail of every env away, a segment keeps everything), seconds per epoch (rollout +
update, host clock around device synchronises), trained env-steps per second, and the update graphs' captured / reused
counters behind each of the last three epochs (null where the minibatch is too large for the graphs).

Usage:  python tools/time_segments.py [--envs 4096] [--epochs 5] [--warmup 2] [--segments 32,128]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from com_marl_amd import envs as E, nets  # noqa: E402
from com_marl_amd.algos import CentralizedMAPPO  # noqa: E402
from com_marl_amd.sampler import CentralizedMAOnPolicyVectorizedSampler  # noqa: E402


class _Shell:                                       # what the sampler needs from the env object
    def __init__(self, batch, spec):
        self.batch, self.spec, self.bound_return = batch, spec, 0.0


class _Mode:
    def __init__(self, name, segment_steps, cfg, n_envs, dev, seed):
        self.name, self.dev = name, dev
        env = E.GridEnvBatch(cfg["scenario"], bench.env_params(cfg), n_envs, device=dev, seed=seed)
        spec = E.EnvSpec(E._Box(np.zeros(env.d * env.N), np.ones(env.d * env.N)), E._Discrete(5))
        torch.manual_seed(seed)
        policy = bench.make_policy("commdp", spec, env.N, dev)
        policy.set_rng(seed)
        torch.manual_seed(seed + 1)
        critic = nets.CommBaseCritic(spec, n_agents=env.N, device=dev)
        mpl = cfg["max_env_steps"]
        self.algo = CentralizedMAPPO(env_spec=spec, policy=policy, baseline=critic, device=dev, max_path_length=mpl, discount=0.99,
                                     center_adv=True, positive_adv=False, gae_lambda=0.97, policy_ent_coeff=0.1,
                                     entropy_method="regularized", clip_grad_norm=7, optimization_n_minibatches=3,
                                     optimization_mini_epochs=10, segment_steps=segment_steps)
        self.smp = CentralizedMAOnPolicyVectorizedSampler(self.algo, _Shell(env, spec), n_envs=n_envs)
        self.smp.start_worker()
        self.env, self.batch_size = env, n_envs * env.N * mpl
        self.rows, self.itr = [], 0

    def epoch(self):
        torch.cuda.synchronize(self.dev)
        t0 = time.perf_counter()
        paths = self.smp.obtain_samples(self.itr, batch_size=self.batch_size)
        torch.cuda.synchronize(self.dev)
        t1 = time.perf_counter()
        self.algo.train_once(itr=self.itr, paths=paths)
        torch.cuda.synchronize(self.dev)
        t2 = time.perf_counter()
        self.itr += 1
        ug = getattr(self.algo, "_update_graphs", None)
        self.rows.append(dict(rollout_s=t1 - t0, update_s=t2 - t1, steps_run=self.smp.last_steps_run * self.env.B,
                              steps_kept=self.algo.stats["EnvSteps"], graphs=None if ug is None else [ug.captured, ug.reused]))

    def report(self, warmup):
        rows = self.rows[warmup:]
        med = lambda k: float(np.median([r[k] for r in rows]))                  # noqa: E731
        s = float(np.median([r["rollout_s"] + r["update_s"] for r in rows]))
        run, kept = med("steps_run"), med("steps_kept")
        return dict(mode=self.name, epochs=len(rows), env_steps_run_per_epoch=run, env_steps_kept_per_epoch=kept, kept_share=kept / run,
                    rollout_s_per_epoch=med("rollout_s"), update_s_per_epoch=med("update_s"), s_per_epoch=s,
                    s_per_epoch_min_max=[min(r["rollout_s"] + r["update_s"] for r in rows), max(r["rollout_s"] + r["update_s"] for r in rows)],
                    trained_env_steps_per_s=kept / s, update_graphs_captured_reused_last3=[r["graphs"] for r in rows[-3:]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--segments", default="32,128")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_segments.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    cfg = dict(bench.CONFIGS["pp_map10"])
    modes = [_Mode("whole_episodes", None, cfg, args.envs, dev, args.seed)]
    modes += [_Mode(f"segments_{n}", int(n), cfg, args.envs, dev, args.seed) for n in args.segments.split(",") if n]
    for _ in range(args.warmup + args.epochs):
        for m in modes:
            np.random.seed(args.seed + m.itr)
            m.epoch()
    for m in modes:
        print(json.dumps(m.report(args.warmup)))


if __name__ == "__main__":
    main()
