"""Update time of the deterministic update mode against the default at the train loop's 4096 envs (bench.py's train_loop leg:
PP map10 N=4, Comm-DP, 3 minibatches x 10 mini-epochs): update_s_per_epoch of each, alternated over --rounds so that drift
hits both alike.

Usage:  python tools/deterministic_update_time.py [--envs 4096] [--epochs 2] [--rounds 2]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import com_marl_amd  # noqa: E402
from com_marl_amd import envs as E  # noqa: E402
from com_marl_amd.train_bench import train_loop_measurement  # noqa: E402

MODES = {"default": False, "deterministic": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    c = dict(bench.CONFIGS["pp_map10"])
    res = {m: [] for m in MODES}
    for _ in range(args.rounds):
        for mode, on in MODES.items():
            com_marl_amd.set_deterministic(on)
            env = E.GridEnvBatch(c["scenario"], bench.env_params(c), args.envs, device=dev, seed=args.seed)
            spec = E.EnvSpec(E._Box(np.zeros(env.d * env.N), np.ones(env.d * env.N)), E._Discrete(5))
            torch.manual_seed(args.seed)
            policy = bench.make_policy("commdp", spec, env.N, dev)
            policy.set_rng(args.seed)
            r = train_loop_measurement(env, policy, c, spec, 1, 0, dev, args.seed, epochs=args.epochs)
            res[mode].append(r["update_s_per_epoch"])
            del env, policy
    com_marl_amd.set_deterministic(None)
    base, det = min(res["default"]), min(res["deterministic"])
    print(json.dumps(dict(envs=args.envs, epochs=args.epochs, update_s_per_epoch=res,
                          best_default=base, best_deterministic=det, overhead=det / base - 1.0)))


if __name__ == "__main__":
    main()
