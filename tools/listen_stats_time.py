"""What the listening statistics cost on one MI355X (DESIGN.md §7 "Listening statistics").
    python tools/listen_stats_time.py sweep   comm_stats_time.py's eval_sweep (K = 8 x C = 8 on 4096 envs of PP map 10, fused
                                              wrapper, 200 steps, one round) with and without listen_stats: whole calls on the
                                              host clock, fresh wrappers of one seed for every call, both warmed, alternating for
                                              five rounds; prints policy 0's curve.
    python tools/listen_stats_time.py parts   the same round played once, then its parts timed on their own (device events,
                                              five repetitions each): the mute replay, the lossless replay, cm_listen_stats."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from com_marl_amd import _lib as L, envs as E, nets  # noqa: E402
from com_marl_amd.evaluate import LISTEN_KEYS, eval_sweep, sweep_layout  # noqa: E402
from com_marl_amd.rollout import RolloutEngine  # noqa: E402
from comm_stats_time import CONDS, PP, ROUNDS, SEED, T, event_time, sync_time  # noqa: E402  (the same directory)

B, K = 4096, 8


def _wrapper():
    return E.PredatorPreyWrapper(True, params=PP, n_envs=B, device="cuda:0", seed=SEED, channel="IID", conditions=CONDS,
                                 fused_conditions=True)


def _policies(spec):
    pols = []
    for k in range(K):
        torch.manual_seed(k)
        p = nets.CommCategoricalMLPPolicy(spec, n_agents=4, device="cuda:0")
        p.set_rng(SEED)
        pols.append(p)
    return pols


def sweep():
    C_ = len(CONDS)
    n_epi = B // (K * C_)
    first = _wrapper()
    pols = _policies(first.spec)
    call = lambda env, flag: eval_sweep(env, pols, 0, n_eval_episodes=n_epi, max_env_steps=T, eval_greedy=True,   # noqa: E731
                                        paired=True, listen_stats=flag)
    _, got = sync_time(lambda: call(first, True))
    _, ref = sync_time(lambda: call(_wrapper(), False))
    same = all(got[k][c][key] == v for k in range(K) for c in range(C_) for key, v in ref[k][c].items())
    print(f"every key of the sweep without listen_stats is unchanged with it: {same}", flush=True)
    for c in range(C_):
        print(f"  {CONDS[c]}: success {got[0][c]['success']:.3f} " + " ".join(f"{key} {got[0][c][key]:.3e}" for key in LISTEN_KEYS), flush=True)
    ms = {True: [], False: []}
    for r in range(ROUNDS):
        for flag in (True, False):
            env = _wrapper()
            dt, _ = sync_time(lambda: call(env, flag))
            ms[flag].append(dt * 1e3)
            print(f"[{r}] eval_sweep {K} x {C_} cells x {n_epi} episodes, {B} envs, listen_stats={flag}: {dt * 1e3:9.2f} ms", flush=True)
    print(json.dumps({"workload": "pp_map10 fused", "envs": B, "policies": K, "conditions": C_, "steps": T, "unchanged_keys_equal": bool(same),
                      "with_listen_stats_ms": [round(x, 3) for x in ms[True]], "without_ms": [round(x, 3) for x in ms[False]]}), flush=True)
    return same


def parts():
    C_ = len(CONDS)
    env = _wrapper()
    batch = getattr(env, "env", env).batch
    ps = nets.PolicySet(_policies(env.spec))
    batch.set_conditions(CONDS, *sweep_layout(B, K, C_, batch.cfg.env_id_offset, True))
    ps.sync_weights()
    ps.reset([True] * (B // K))
    eng = RolloutEngine(batch, ps, T, store_attn=False, store_probs=True, groups=[B // K] * K)
    eng.reset()
    eng.play(0, T, greedy=True, chunk=True)
    eng.bump(T)
    N, A = batch.N, 5
    mute, lossless = (torch.empty(T, B, N, A, device="cuda") for _ in range(2))
    stats = torch.empty(T, B, L.LISTEN_COLS, dtype=torch.float64, device="cuda")
    lib, st = L.lib(), L.current_stream()
    jobs = {
        "round (reset + play)": lambda r: (eng.reset(), eng.play(0, T, greedy=True, chunk=True)),
        "mute replay": lambda r: eng.replay_probs(0, T, "identity", mute),
        "lossless replay": lambda r: eng.replay_probs(0, T, "ones", lossless),
        "cm_listen_stats": lambda r: L.check(lib.cm_listen_stats(T * B, N, A, L.ptr(eng.probs), N * A, L.ptr(mute), N * A, L.ptr(lossless),
                                                                 N * A, L.ptr(stats), st), "cm_listen_stats"),
    }
    res = {}
    for name, job in jobs.items():
        event_time(job, 1)
        res[name] = [round(event_time(job, 1), 1) for _ in range(ROUNDS)]
        print(f"{name}: {res[name]} us", flush=True)
    print(json.dumps({"workload": "pp_map10 fused", "envs": B, "policies": K, "steps": T, "us": res,
                      "mean_stats_row": stats.mean((0, 1)).tolist()}), flush=True)


if __name__ == "__main__":
    mode = sys.argv[1:2]
    if mode == ["sweep"]:
        sys.exit(0 if sweep() else 1)
    elif mode == ["parts"]:
        parts()
    else:
        sys.exit(__doc__)
