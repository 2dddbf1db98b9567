"""What the per-step evaluation curves cost on one MI355X (DESIGN.md §7 "Per-step evaluation curves").
    python tools/eval_curves_time.py kernel   cm_episode_curves against cm_episode_stats per launch (device events around REPS
                                              launches) on the same trajectory buffers: 4096 envs x 200 steps, PP teams of 4, a
                                              recorded adjacency, groups of 64 envs (the sweep's cells).  Two sets of lengths:
                                              `full` (no episode ends: every slot is read) and `mixed` (a quarter never ends, the
                                              rest end at uniformly random steps).  The buffers exist four times and the launches
                                              cycle through them (4 x 85 MB, past the 256 MB last-level cache); the two kernels
                                              alternate for five rounds after a warm-up.  Prints the bytes each has to read by its
                                              semantics (from the lengths) and the rate that makes.
    python tools/eval_curves_time.py sweep    evaluate.eval_sweep, K = 8 policies x C = 8 conditions on 4096 envs of PP map 10 (teams
                                              of 4, fused_conditions=True, 200 steps, one round), with and without curves, without and
                                              with comm_stats: whole calls on the host clock, each ending in a synchronise, fresh
                                              wrappers of one seed for every call, all warmed, alternating for five rounds; the keys
                                              of the call without curves are compared first."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from com_marl_amd import _lib as L, envs as E, nets  # noqa: E402
from com_marl_amd.evaluate import eval_sweep  # noqa: E402

ROUNDS, REPS, COPIES = 5, 40, 4
T, B, N, GROUP = 200, 4096, 4, 64


def event_time(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for r in range(reps):
        fn(r)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps                           # us per call


def kernel(kind):
    rng = np.random.default_rng(0)
    n = np.full(B, T)
    path_len = np.zeros((T, B), np.int32)
    if kind == "mixed":
        ends = rng.random(B) < 0.75
        n = np.where(ends, rng.integers(1, T + 1, B), T)
        path_len[n[ends] - 1, np.nonzero(ends)[0]] = n[ends]
    g = torch.Generator(device="cuda").manual_seed(0)
    sets = []
    for _ in range(COPIES):
        sets.append(dict(reward=torch.randn(T, B, dtype=torch.float64, device="cuda", generator=g),
                         details=torch.randint(0, 9, (T, B, 6), dtype=torch.int32, device="cuda", generator=g),
                         success=torch.randint(0, 2, (T, B), dtype=torch.int32, device="cuda", generator=g),
                         path_len=torch.from_numpy(path_len).cuda(),
                         adj=(torch.rand(T + 1, B, N, N, device="cuda", generator=g) < 0.5).float()))
    groups = B // GROUP
    table = torch.zeros(groups, GROUP, L.EPI_COLS, dtype=torch.float64, device="cuda")
    sums = torch.zeros(groups, T, L.EPI_COLS, dtype=torch.float64, device="cuda")
    lib, st = L.lib(), L.current_stream()
    # per running (step, env): reward 8 + details 24 + success 4 + path_len 4 bytes and one 64-byte adjacency block (an episode of
    # n steps reads n blocks in both kernels: stats slots 1 .. n-1 and n-1 once, curves one per step)
    stats_bytes = int(n.sum()) * (40 + 4 * N * N)
    # the curves kernel reads path_len a second time: rows 0 .. t0-1 in front of every tile of steps, while a lane still runs
    # (the tile length as csrc/cm_episode_curves.hip chooses it: 16, halved down to 4 while that leaves fewer than 1024 waves)
    tile = 16
    while tile > 4 and groups * -(-T // tile) < 1024:
        tile //= 2
    scan = sum(int(np.minimum(n, t0).sum()) for t0 in range(0, T, tile)) * 4
    curves_bytes = stats_bytes + scan

    def stats(r):
        s = sets[r % COPIES]
        L.check(lib.cm_episode_stats(T, B, N, L.CM_PP, L.ptr(s["reward"]), L.ptr(s["details"]), L.ptr(s["success"]), L.ptr(s["path_len"]),
                                     L.ptr(s["adj"]), GROUP, GROUP, GROUP, 0, L.ptr(table), st), "cm_episode_stats")

    def curves(r):
        s = sets[r % COPIES]
        L.check(lib.cm_episode_curves(T, B, N, L.CM_PP, L.ptr(s["reward"]), L.ptr(s["details"]), L.ptr(s["success"]), L.ptr(s["path_len"]),
                                      L.ptr(s["adj"]), GROUP, GROUP, 0, L.ptr(sums), st), "cm_episode_curves")

    event_time(stats, REPS)
    event_time(curves, REPS)
    s_us, c_us = [], []
    for r in range(ROUNDS):
        s_us.append(event_time(stats, REPS))
        c_us.append(event_time(curves, REPS))
        print(f"[{r}] {kind}: mean length {n.mean():.1f}; cm_episode_stats {s_us[-1]:8.1f} us ({stats_bytes / 1e6:.1f} MB, "
              f"{stats_bytes / s_us[-1] / 1e3:7.1f} GB/s); cm_episode_curves {c_us[-1]:8.1f} us ({curves_bytes / 1e6:.1f} MB, "
              f"{curves_bytes / c_us[-1] / 1e3:7.1f} GB/s)", flush=True)
    # the two reductions of the same buffers agree: a curve summed over the steps is the sum of the episodes' sums
    stats(0)
    curves(0)
    torch.cuda.synchronize()
    a, b = sums.sum(1)[:, 3].cpu().numpy(), table.sum(1)[:, 3].cpu().numpy()
    med = lambda x: sorted(x)[len(x) // 2]                          # noqa: E731
    print(json.dumps({"lengths": kind, "envs": B, "steps": T, "N": N, "group_size": GROUP, "mean_length": float(n.mean()),
                      "stats_bytes": stats_bytes, "curves_bytes": curves_bytes, "cm_episode_stats_us": [round(x, 1) for x in s_us],
                      "cm_episode_curves_us": [round(x, 1) for x in c_us], "curves_over_stats_median": round(med(c_us) / med(s_us), 3),
                      "step_counts_agree": bool((a == b).all())}), flush=True)


SEED = 3
PP = dict(load=2, max_env_steps=T, capture_reward=10, step_cost=0.1, rm=0, penalty=0, grid_size=10, Rsen=1, n_agents=4, n_preys=4,
          n_gcn_layers=2, mode="test", teRcom=9, tepl=0)
CONDS = [dict(Rcom=r, pl=p) for r in (9, 3, 2, 1) for p in (0.0, 0.5)]


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def sweep():
    K, C_ = 8, len(CONDS)
    n_epi = B // (K * C_)
    wrapper = lambda: E.PredatorPreyWrapper(True, params=PP, n_envs=B, device="cuda:0", seed=SEED, channel="IID",   # noqa: E731
                                            conditions=CONDS, fused_conditions=True)
    first = wrapper()
    pols = []
    for k in range(K):
        torch.manual_seed(k)
        p = nets.CommCategoricalMLPPolicy(first.spec, n_agents=4, device="cuda:0")
        p.set_rng(SEED)
        pols.append(p)
    call = lambda env, comm, curves: eval_sweep(env, pols, 0, n_eval_episodes=n_epi, max_env_steps=T, eval_greedy=True,   # noqa: E731
                                                paired=True, comm_stats=comm, curves=curves)
    same = True
    for comm in (False, True):
        _, got = sync_time(lambda: call(wrapper(), comm, True))
        _, ref = sync_time(lambda: call(wrapper(), comm, False))
        same = same and all(got[k][c][key] == v for k in range(K) for c in range(C_) for key, v in ref[k][c].items())
    print(f"every key of the sweep without curves is unchanged with them: {same}", flush=True)
    cv = got[0][5]["curves"]
    print(f"  policy 0 under {CONDS[5]}: running share at steps 0, 50, 100, 199: {cv['step_cnt'][[0, 50, 100, 199]].tolist()}; "
          f"delivery {cv['delivery'][[0, 50, 100, 199]].tolist()}", flush=True)
    variants = [(comm, curves) for comm in (False, True) for curves in (False, True)]
    ms = {v: [] for v in variants}
    for r in range(ROUNDS):
        for v in variants:
            env = wrapper()
            dt, _ = sync_time(lambda: call(env, *v))
            ms[v].append(dt * 1e3)
            print(f"[{r}] eval_sweep {K} x {C_} cells x {n_epi} episodes, {B} envs, comm_stats={v[0]}, curves={v[1]}: {dt * 1e3:9.2f} ms", flush=True)
    print(json.dumps({"workload": "pp_map10 fused", "envs": B, "policies": K, "conditions": C_, "steps": T, "unchanged_keys_equal": bool(same),
                      **{f"comm_stats={v[0]},curves={v[1]}_ms": [round(x, 3) for x in ms[v]] for v in variants}}), flush=True)
    return same


if __name__ == "__main__":
    mode = sys.argv[1:2]
    if mode == ["kernel"]:
        for kind in sys.argv[2:] or ["full", "mixed"]:
            kernel(kind)
    elif mode == ["sweep"]:
        sys.exit(0 if sweep() else 1)
    else:
        sys.exit(__doc__)
