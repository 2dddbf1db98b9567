"""What the communication statistics cost on one MI355X (DESIGN.md §7 "Communication statistics").
    python tools/comm_stats_time.py kernel    cm_comm_stats per launch (device events around REPS launches) at
                                              pp4    N = 4,  L = 2, S = 201 x 4096 graphs (158 MB: a sweep round of 4096 envs)
                                              pp72   N = 72, L = 2, S = 201 x 1024 graphs (12.8 GB: a 200-step round at PP map 30)
                                              against a device-to-device copy of the same arrays timed in the same process (the
                                              copy reads AND writes those bytes), alternating for five rounds after a warm-up.
                                              The pp4 arrays exist four times and the launches cycle through them (632 MB, past the
                                              256 MB last-level cache).
    python tools/comm_stats_time.py sweep     evaluate.eval_sweep, K = 8 policies x C = 8 conditions on 4096 envs of PP map 10 (teams
                                              of 4, fused_conditions=True, 200 steps, one round), with and without comm_stats: whole
                                              calls on the host clock, each ending in a synchronise, fresh wrappers of one seed for
                                              every call, both warmed, alternating for five rounds; prints policy 0's curve."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from com_marl_amd import _lib as L, envs as E, nets  # noqa: E402
from com_marl_amd.evaluate import COMM_KEYS, eval_sweep  # noqa: E402

ROUNDS = 5
SHAPES = {"pp4": dict(N=4, Lh=2, S=201 * 4096, copies=4, reps=50), "pp72": dict(N=72, Lh=2, S=201 * 1024, copies=1, reps=5)}


def event_time(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for r in range(reps):
        fn(r)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps                           # us per call


def kernel(name):
    w = SHAPES[name]
    N, Lh, S, copies, reps = w["N"], w["Lh"], w["S"], w["copies"], w["reps"]
    g = torch.Generator(device="cuda").manual_seed(0)
    sets = []
    for _ in range(copies):
        adj = torch.empty(S, N, N, device="cuda")
        chan = torch.empty(S, Lh, N, N, device="cuda")
        for t in (adj, chan):                                        # 0 / 1 at density 0.5, filled in slices (no S-sized temporaries)
            flat = t.view(-1)
            for lo in range(0, flat.numel(), 1 << 26):
                hi = min(flat.numel(), lo + (1 << 26))
                flat[lo:hi] = (torch.rand(hi - lo, device="cuda", generator=g) < 0.5).float()
        sets.append((adj, chan))
    d_adj, d_chan = torch.empty_like(sets[0][0]), torch.empty_like(sets[0][1])
    out = torch.empty(S, L.COMM_COLS, dtype=torch.int32, device="cuda")
    lib, st = L.lib(), L.current_stream()
    nbytes = (sets[0][0].numel() + sets[0][1].numel()) * 4

    def launch(r):
        adj, chan = sets[r % copies]
        L.check(lib.cm_comm_stats(S, N, Lh, L.ptr(adj), N * N, L.ptr(chan), Lh * N * N, L.ptr(out), st), "cm_comm_stats")

    def copy(r):
        adj, chan = sets[r % copies]
        d_adj.copy_(adj)
        d_chan.copy_(chan)

    event_time(launch, reps)
    event_time(copy, reps)
    k_us, c_us = [], []
    for r in range(ROUNDS):
        k_us.append(event_time(launch, reps))
        c_us.append(event_time(copy, reps))
        print(f"[{r}] {name} N={N} L={Lh} S={S} ({nbytes / 1e6:.0f} MB): cm_comm_stats {k_us[-1]:10.1f} us ({nbytes / k_us[-1] / 1e6:6.2f} TB/s read), "
              f"copy {c_us[-1]:10.1f} us ({nbytes / c_us[-1] / 1e6:6.2f} TB/s read + as much written)", flush=True)
    med = lambda x: sorted(x)[len(x) // 2]                          # noqa: E731
    print(json.dumps({"shape": name, "N": N, "L": Lh, "S": S, "bytes": nbytes, "cm_comm_stats_us": [round(x, 1) for x in k_us],
                      "copy_us": [round(x, 1) for x in c_us], "kernel_over_copy_median": round(med(k_us) / med(c_us), 3),
                      "mean_stats_row": out.double().mean(0).tolist()}), flush=True)


T, SEED = 200, 3
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
    B, K, C_ = 4096, 8, len(CONDS)
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
    call = lambda env, flag: eval_sweep(env, pols, 0, n_eval_episodes=n_epi, max_env_steps=T, eval_greedy=True,   # noqa: E731
                                        paired=True, comm_stats=flag)
    _, got = sync_time(lambda: call(first, True))
    _, ref = sync_time(lambda: call(wrapper(), False))
    same = all(got[k][c][key] == v for k in range(K) for c in range(C_) for key, v in ref[k][c].items())
    print(f"every key of the sweep without comm_stats is unchanged with it: {same}", flush=True)
    for c in range(C_):
        print(f"  {CONDS[c]}: success {got[0][c]['success']:.3f} " + " ".join(f"{key} {got[0][c][key]:.4f}" for key in COMM_KEYS), flush=True)
    ms = {True: [], False: []}
    for r in range(ROUNDS):
        for flag in (True, False):
            env = wrapper()
            dt, _ = sync_time(lambda: call(env, flag))
            ms[flag].append(dt * 1e3)
            print(f"[{r}] eval_sweep {K} x {C_} cells x {n_epi} episodes, {B} envs, comm_stats={flag}: {dt * 1e3:9.2f} ms", flush=True)
    print(json.dumps({"workload": "pp_map10 fused", "envs": B, "policies": K, "conditions": C_, "steps": T, "unchanged_keys_equal": bool(same),
                      "with_comm_stats_ms": [round(x, 3) for x in ms[True]], "without_ms": [round(x, 3) for x in ms[False]]}), flush=True)
    return same


if __name__ == "__main__":
    mode = sys.argv[1:2]
    if mode == ["kernel"]:
        for name in sys.argv[2:] or list(SHAPES):
            kernel(name)
    elif mode == ["sweep"]:
        sys.exit(0 if sweep() else 1)
    else:
        sys.exit(__doc__)
