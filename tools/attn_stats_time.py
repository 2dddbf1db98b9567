"""What the attention statistics cost on one MI355X (DESIGN.md §7 "Attention statistics").
    python tools/attn_stats_time.py kernel    cm_attn_stats per launch (device events around REPS launches) at comm_stats_time.py's
                                              two shapes with the attention array added
                                              pp4    N = 4,  L = 2, S = 201 x 4096 graphs (211 MB)
                                              pp72   N = 72, L = 2, S = 201 x 1024 graphs (17.1 GB)
                                              masks 0 / 1 at density 0.5, attention rows an f32 softmax of random logits, against
                                              a device-to-device copy of the same arrays timed in the same process (the copy reads
                                              AND writes the bytes the kernel only reads), alternating for five rounds after a
                                              warm-up.  The pp4 arrays exist four times and the launches cycle through them.
    python tools/attn_stats_time.py sweep     comm_stats_time.py's eval_sweep (K = 8 x C = 8 on 4096 envs of PP map 10, fused
                                              wrapper, 200 steps, one round) with and without attn_stats: whole calls on the host
                                              clock, fresh wrappers of one seed for every call, both warmed, alternating for five
                                              rounds; prints policy 0's curve."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from com_marl_amd import _lib as L, envs as E, nets  # noqa: E402
from com_marl_amd.evaluate import ATTN_KEYS, eval_sweep  # noqa: E402
from comm_stats_time import CONDS, PP, ROUNDS, SEED, SHAPES, T, event_time, sync_time  # noqa: E402  (the same directory)

SLICE = 1 << 24                                                     # floats filled at a time (no S-sized temporaries)


def kernel(name):
    w = SHAPES[name]
    N, Lh, S, copies, reps = w["N"], w["Lh"], w["S"], w["copies"], w["reps"]
    g = torch.Generator(device="cuda").manual_seed(0)
    sets = []
    for _ in range(copies):
        attn = torch.empty(S, N, N, device="cuda")
        adj = torch.empty(S, N, N, device="cuda")
        chan = torch.empty(S, Lh, N, N, device="cuda")
        rows = attn.view(-1, N)
        step = max(1, SLICE // N)
        for lo in range(0, rows.shape[0], step):
            hi = min(rows.shape[0], lo + step)
            rows[lo:hi] = torch.softmax(torch.randn(hi - lo, N, device="cuda", generator=g), dim=-1)
        for t in (adj, chan):
            flat = t.view(-1)
            for lo in range(0, flat.numel(), SLICE):
                hi = min(flat.numel(), lo + SLICE)
                flat[lo:hi] = (torch.rand(hi - lo, device="cuda", generator=g) < 0.5).float()
        sets.append((attn, adj, chan))
    dst = [torch.empty_like(t) for t in sets[0]]
    out = torch.empty(S, L.ATTN_COLS, dtype=torch.float64, device="cuda")
    lib, st = L.lib(), L.current_stream()
    nbytes = sum(t.numel() for t in sets[0]) * 4

    def launch(r):
        attn, adj, chan = sets[r % copies]
        L.check(lib.cm_attn_stats(S, N, Lh, L.ptr(attn), N * N, L.ptr(adj), N * N, L.ptr(chan), Lh * N * N, L.ptr(out), st),
                "cm_attn_stats")

    def copy(r):
        for d, t in zip(dst, sets[r % copies]):
            d.copy_(t)

    event_time(launch, reps)
    event_time(copy, reps)
    k_us, c_us = [], []
    for r in range(ROUNDS):
        k_us.append(event_time(launch, reps))
        c_us.append(event_time(copy, reps))
        print(f"[{r}] {name} N={N} L={Lh} S={S} ({nbytes / 1e6:.0f} MB): cm_attn_stats {k_us[-1]:10.1f} us ({nbytes / k_us[-1] / 1e6:6.2f} TB/s read), "
              f"copy {c_us[-1]:10.1f} us ({nbytes / c_us[-1] / 1e6:6.2f} TB/s read + as much written)", flush=True)
    med = lambda x: sorted(x)[len(x) // 2]                          # noqa: E731
    print(json.dumps({"shape": name, "N": N, "L": Lh, "S": S, "bytes": nbytes, "cm_attn_stats_us": [round(x, 1) for x in k_us],
                      "copy_us": [round(x, 1) for x in c_us], "kernel_over_copy_median": round(med(k_us) / med(c_us), 3),
                      "mean_stats_row": out.mean(0).tolist()}), flush=True)


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
                                        paired=True, attn_stats=flag)
    _, got = sync_time(lambda: call(first, True))
    _, ref = sync_time(lambda: call(wrapper(), False))
    same = all(got[k][c][key] == v for k in range(K) for c in range(C_) for key, v in ref[k][c].items())
    print(f"every key of the sweep without attn_stats is unchanged with it: {same}", flush=True)
    for c in range(C_):
        print(f"  {CONDS[c]}: success {got[0][c]['success']:.3f} " + " ".join(f"{key[5:]} {got[0][c][key]:.4f}" for key in ATTN_KEYS), flush=True)
    ms = {True: [], False: []}
    for r in range(ROUNDS):
        for flag in (True, False):
            env = wrapper()
            dt, _ = sync_time(lambda: call(env, flag))
            ms[flag].append(dt * 1e3)
            print(f"[{r}] eval_sweep {K} x {C_} cells x {n_epi} episodes, {B} envs, attn_stats={flag}: {dt * 1e3:9.2f} ms", flush=True)
    print(json.dumps({"workload": "pp_map10 fused", "envs": B, "policies": K, "conditions": C_, "steps": T, "unchanged_keys_equal": bool(same),
                      "with_attn_stats_ms": [round(x, 3) for x in ms[True]], "without_ms": [round(x, 3) for x in ms[False]]}), flush=True)
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
