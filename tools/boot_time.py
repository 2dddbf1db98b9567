"""What the bootstrap intervals and paired contrasts cost on one MI355X (DESIGN.md §7 "Bootstrap intervals").
    python tools/boot_time.py sweep     comm_stats_time.py's eval_sweep (K = 8 x C = 8 on 4096 envs of PP map 10, fused wrapper, 200
                                        steps, one round of 64 episodes a cell) three ways: with ci=None - plain, no statistics family
                                        on, and with all four families on -, with ci=0.95, n_boot=2000 on all four families, and with
                                        contrast=dict(condition=0) added.  Whole calls on the host clock, fresh wrappers of one seed
                                        for every call, all warmed, alternating for five rounds; medians.  The keys without ci are
                                        compared (==) with those of the call with it.
    python tools/boot_time.py kernels   cm_boot_means and cm_boot_quantiles alone (device events, five repetitions of 20 launches
                                        each) on tables of the sweep's sizes: 64 cells x 64 and 100 episodes x 4 / 6 / 9 columns,
                                        2000 resamples, staged and from global memory; the quantiles with and without ref_cell."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from com_marl_amd import _lib as L, envs as E, nets  # noqa: E402
from com_marl_amd.evaluate import eval_sweep  # noqa: E402
from comm_stats_time import CONDS, PP, ROUNDS, SEED, T, event_time, sync_time  # noqa: E402  (the same directory)

B, K = 4096, 8
FAMILIES = dict(comm_stats=True, attn_stats=True, listen_stats=True, value_stats=True)


def _wrapper():
    return E.PredatorPreyWrapper(True, params=PP, n_envs=B, device="cuda:0", seed=SEED, channel="IID", conditions=CONDS,
                                 fused_conditions=True)


def _nets(spec):
    pols, critics = [], []
    for k in range(K):
        torch.manual_seed(k)
        p = nets.CommCategoricalMLPPolicy(spec, n_agents=4, device="cuda:0")
        p.set_rng(SEED)
        pols.append(p)
        critics.append(nets.CommBaseCritic(spec, n_agents=4, device="cuda:0"))
    return pols, critics


def sweep():
    C_ = len(CONDS)
    n_epi = B // (K * C_)
    first = _wrapper()
    pols, critics = _nets(first.spec)
    fam = dict(FAMILIES, baselines=critics)
    legs = {
        "plain, ci=None": {},
        "families, ci=None": fam,
        "families, ci=0.95": dict(fam, ci=0.95, n_boot=2000),
        "families, ci=0.95, contrast": dict(fam, ci=0.95, n_boot=2000, contrast=dict(condition=0)),
    }
    call = lambda env, kw: eval_sweep(env, pols, 0, n_eval_episodes=n_epi, max_env_steps=T, eval_greedy=True, paired=True, **kw)   # noqa: E731
    warm = {name: sync_time(lambda: call(first if i == 0 else _wrapper(), kw))[1] for i, (name, kw) in enumerate(legs.items())}
    off, on, con = warm["families, ci=None"], warm["families, ci=0.95"], warm["families, ci=0.95, contrast"]
    same = all(on[k][c][key] == v and con[k][c][key] == v for k in range(K) for c in range(C_) for key, v in off[k][c].items())
    print(f"every key of the sweep without ci is unchanged with it: {same}", flush=True)
    for c in range(C_):
        d = con[0][c]
        print(f"  {CONDS[c]}: reward {d['reward']:.3f} ci ({d['ci']['reward'][0]:.3f}, {d['ci']['reward'][1]:.3f}) se {d['se']['reward']:.3f}; "
              f"delivery {d['delivery']:.3f} ci ({d['ci']['delivery'][0]:.3f}, {d['ci']['delivery'][1]:.3f}); against condition 0: "
              f"reward diff {d['contrast']['reward']['diff']:.3f} ({d['contrast']['reward']['lo']:.3f}, {d['contrast']['reward']['hi']:.3f}) "
              f"p_gt {d['contrast']['reward']['p_gt']:.3f}", flush=True)
    ms = {name: [] for name in legs}
    for r in range(ROUNDS):
        for name, kw in legs.items():
            env = _wrapper()
            dt, _ = sync_time(lambda: call(env, kw))
            ms[name].append(dt * 1e3)
            print(f"[{r}] eval_sweep {K} x {C_} cells x {n_epi} episodes, {B} envs, {name}: {dt * 1e3:9.2f} ms", flush=True)
    print(json.dumps({"workload": "pp_map10 fused", "envs": B, "policies": K, "conditions": C_, "steps": T, "episodes_per_cell": n_epi,
                      "n_boot": 2000, "unchanged_keys_equal": bool(same), "ms": {n: [round(x, 3) for x in v] for n, v in ms.items()},
                      "median_ms": {n: round(statistics.median(v), 3) for n, v in ms.items()}}), flush=True)
    return same


def kernels():
    cells, n_boot, reps = 64, 2000, 20
    lib, st = L.lib(), L.current_stream()
    g = torch.Generator(device="cuda").manual_seed(0)
    ref = torch.zeros(cells, dtype=torch.int32, device="cuda")
    res = {}
    for n in (64, 100):
        for cols, kind in ((4, L.BOOT_COMM), (6, L.BOOT_VALUE), (9, L.BOOT_COLUMNS)):
            table = torch.rand(cells, n, cols, generator=g, dtype=torch.float64, device="cuda") + 0.5
            means = torch.empty(cells, n_boot, cols, dtype=torch.float64, device="cuda")
            keys = E.boot_keys({v: k for k, v in E.BOOT_KINDS.items()}[kind], cols)
            out = torch.empty(cells, keys, L.BOOT_OUT, dtype=torch.float64, device="cuda")
            run_means = lambda r: L.check(lib.cm_boot_means(cells, n, cols, L.ptr(table), n_boot, 1, 0, L.ptr(means), st), "cm_boot_means")   # noqa: E731
            jobs = {"cm_boot_means staged": (run_means, None), "cm_boot_means global": (run_means, "0")}
            for with_ref in (False, True):
                jobs[f"cm_boot_quantiles {keys} keys" + (" ref_cell" if with_ref else "")] = (
                    lambda r, p=L.ptr(ref) if with_ref else None: L.check(
                        lib.cm_boot_quantiles(kind, cells, n_boot, cols, L.ptr(means), p, 50, 1949, L.ptr(out), st), "cm_boot_quantiles"), None)
            for name, (job, budget) in jobs.items():
                if budget is None:
                    os.environ.pop("COMMARL_BOOT_STAGE_BYTES", None)
                else:
                    os.environ["COMMARL_BOOT_STAGE_BYTES"] = budget
                event_time(job, 2)
                us = [round(event_time(job, reps), 1) for _ in range(ROUNDS)]
                res[f"n={n} cols={cols} {name}"] = us
                print(f"n={n} cols={cols} {name}: {us} us, median {statistics.median(us)}", flush=True)
            os.environ.pop("COMMARL_BOOT_STAGE_BYTES", None)
    print(json.dumps({"cells": cells, "n_boot": n_boot, "us": res, "median_us": {k: statistics.median(v) for k, v in res.items()}}), flush=True)


if __name__ == "__main__":
    mode = sys.argv[1:2]
    if mode == ["sweep"]:
        sys.exit(0 if sweep() else 1)
    elif mode == ["kernels"]:
        kernels()
    else:
        sys.exit(__doc__)
