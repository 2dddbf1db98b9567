"""Checkpoint scoring on one MI355X: wall time of evaluate.eval_summary against evaluate.eval_models, whole calls,
each ending in a synchronise, on
  pp_map10   PP map 10, teams of 4, 4096 envs, K = 64 default-shape policies with seeded random weights, 64 episodes each;
  pp_map30   PP map 30, teams of 72, communication range 5, 1024 envs, K = 4, 256 episodes each (the adjacency is recorded per
             step: the reduction walks it);
max_env_steps = 200, greedy, every policy's episodes played in one round.  Both paths are warmed up first, then alternate for
three rounds; every call gets a fresh wrapper of the same params and seed, so all of them play the same episodes, and the first
pair's scores are compared within the bounds of tests/test_eval_summary.py before anything is timed.  Per workload the tool
also prints the bytes cm_episode_stats has to read by its semantics (from the episodes' lengths), for the bytes/s of a
`rocprofv3 --kernel-trace --stats` run of this tool.
`python tools/eval_summary_time.py [pp_map10|pp_map30]` runs one workload, no argument both."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from com_marl_amd import envs as E, nets  # noqa: E402
from com_marl_amd.evaluate import VECTORS, eval_models, eval_summary  # noqa: E402
from tests import episode_ref as R  # noqa: E402

T, ROUNDS = 200, 3
WORKLOADS = {
    "pp_map10": dict(envs=4096, K=64, params=dict(load=2, max_env_steps=T, capture_reward=10, step_cost=0.1, rm=0, penalty=0,
                                                  grid_size=10, Rsen=1, n_agents=4, n_preys=4, n_gcn_layers=2, mode="train",
                                                  trRcom=9, trpl=0)),
    "pp_map30": dict(envs=1024, K=4, params=dict(load=4, max_env_steps=T, capture_reward=10, step_cost=0.1, rm=0, penalty=0,
                                                 grid_size=30, Rsen=2, n_agents=72, n_preys=72, n_gcn_layers=2, mode="train",
                                                 trRcom=5, trpl=0)),
}


def compare(summary, out):
    """One policy's eval_summary dict against its eval_models tuple: the bounds of tests/test_eval_summary.py."""
    data, succ, rew, bound = out
    tab, delta = np.zeros((len(data), R.EPI_COLS)), np.zeros((len(data), R.EPI_COLS))
    tab[:, 0] = succ
    for i, vec in enumerate(VECTORS):
        tab[:, 1 + i] = rew[vec]
        for e, (_, steps) in enumerate(data):
            x = np.abs(np.asarray(steps[vec], np.float64))
            if vec == "nodeDeg":
                delta[e, 1 + i] = 2.0 ** -23 * abs(tab[e, 1 + i]) + R.sum_bound(len(x), x.sum()) / len(x)
            elif vec not in ("step_cnt", "capture_cnt", "penalty_cnt", "vars2"):      # PP: these are whole numbers
                delta[e, 1 + i] = R.sum_bound(len(x), x.sum())
    want = R.episode_means(tab[None])[0]
    got = [summary["success"]] + [summary[v] for v in VECTORS]
    ok = all(abs(got[c] - want[c]) <= R.mean_bound(tab[:, c], delta[:, c]) for c in range(R.EPI_COLS))
    ok = ok and abs(summary["return_std"] - want[9]) <= R.std_bound(tab[:, 1], delta[:, 1])
    ok = ok and abs(summary["return_min"] - want[10]) <= delta[:, 1].max() and abs(summary["return_max"] - want[11]) <= delta[:, 1].max()
    return ok and summary["bound_return"] == bound


def timed(fn, wrapper, pols, n_epi, **kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(wrapper, pols, 0, n_eval_episodes=n_epi, max_env_steps=T, eval_greedy=True, **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def run(name):
    w = WORKLOADS[name]
    B, K, params = w["envs"], w["K"], w["params"]
    n_epi, N = B // K, params["n_agents"]
    wrap = lambda: E.PredatorPreyWrapper(True, params=params, n_envs=B, device="cuda:0", seed=3)   # noqa: E731
    first = wrap()
    pols = []
    for k in range(K):
        torch.manual_seed(k)
        p = nets.CommCategoricalMLPPolicy(first.spec, n_agents=N, device="cuda:0")
        p.set_rng(3)
        pols.append(p)
    # warm-up of both paths, and the comparison of their scores
    _, got = timed(eval_summary, first, pols, n_epi, episodes=True)
    _, ref = timed(eval_models, wrap(), pols, n_epi)
    same = all(compare(got[k], ref[k]) for k in range(K))
    n = torch.stack([g["episodes"][:, 3] for g in got]).cpu().numpy()                   # episode lengths [K, n_epi]
    slots = np.where(n > 1, n - 1, 1)
    adj_bytes = 0.0 if first.batch.adj_const else float(slots.sum()) * N * N * 4
    print(f"{name}: scores of the two paths agree within the bounds: {same}; episode lengths {int(n.min())} .. {int(n.max())} "
          f"(mean {n.mean():.1f}); cm_episode_stats reads {adj_bytes / 1e6:.1f} MB of adjacency and {n.sum() * 40 / 1e6:.1f} MB of "
          f"per-step columns", flush=True)
    del got, ref
    rounds = {"eval_summary": [], "eval_models": []}
    for r in range(ROUNDS):
        for label, fn in (("eval_summary", eval_summary), ("eval_models", eval_models)):
            dt, out = timed(fn, wrap(), pols, n_epi)
            del out
            rounds[label].append(dt)
            print(f"[{r}] {name} {label:12s} K={K} x {n_epi} episodes ({T} steps, {B} envs): {dt * 1e3:9.2f} ms", flush=True)
    ahead = max(rounds["eval_summary"]) < min(rounds["eval_models"])
    print(json.dumps({"workload": name, "envs": B, "policies": K, "episodes_each": n_epi, "steps": T, "scores_agree": bool(same),
                      "eval_summary_ms": [round(x * 1e3, 3) for x in rounds["eval_summary"]],
                      "eval_models_ms": [round(x * 1e3, 3) for x in rounds["eval_models"]],
                      "summary_ahead_in_every_round_against_every_round": bool(ahead),
                      "adjacency_bytes_required": adj_bytes, "column_bytes_required": float(n.sum() * 40)}), flush=True)
    return same


if __name__ == "__main__":
    names = sys.argv[1:] or list(WORKLOADS)
    ok = [run(name) for name in names]
    sys.exit(0 if all(ok) else 1)
