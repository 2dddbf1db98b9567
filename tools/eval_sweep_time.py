"""Condition sweeps on one MI355X (DESIGN.md §7 "Condition sweeps"): wall time of evaluate.eval_sweep - ONE call over K policies x C
comm conditions - against the same cells scored without per-env conditions: C evaluate.eval_summary calls on uniform wrappers of
B / C envs, the same number of episodes per cell.  Whole calls on the host clock, each ending in a synchronise, on
  pp_map10   PP map 10, teams of 4, 4096 envs, K = 8 policies x C = 8 conditions (IID channel: range x loss), 64 episodes per cell;
  co_map20   CO map 20, teams of 24, 1024 envs, K = 4 x C = 4 (Gilbert-Elliott channel: range x (Pgb, Pbg)), 64 episodes per cell;
  pp_map10_k1  the pp_map10 batch with ONE policy: K = 1 x C = 8, 512 episodes per cell (the single-policy chunk);
max_env_steps = 200, greedy, one round.  Both sides are warmed up first, then alternate for three rounds; every call gets fresh
wrappers of the same seed.  Before anything is timed the sweep's cells of policy 0 are compared (==) with eval_summary of policy 0
on the uniform wrappers (paired ids: those cells play the same episodes).
Teams of 4 get a third leg, alternating with the other two: eval_sweep on a wrapper built with fused_conditions=True (the rollout in
one launch per round, csrc/cm_rollout_wc.hip), whose cells of policy 0 are compared with the unfused sweep's as well.
    python tools/eval_sweep_time.py [pp_map10|pp_map10_k1|co_map20]     one workload, no argument all
    python tools/eval_sweep_time.py rollout_kernels         a 200-step chunk of RolloutEngine on a uniform IID range-3 batch (PP map 10,
                                                            teams of 4, 4096 envs: the non-carried rollout_w_kernel), then on a fused
                                                            conditions batch in which every env has that condition (rollout_wc_kernel),
                                                            three times each: what a `rocprofv3 --kernel-trace --stats` run compares
    python tools/eval_sweep_time.py kernels                 the env step alone, uniform batch then conditions batch of the same
                                                            shape, batch and (single) condition, 300 steps each: the launches a
                                                            `rocprofv3 --kernel-trace --stats` run of this command compares
                                                            (env_kernel* against env_cond_kernel*)
    python tools/eval_sweep_time.py value_stats [off]       the pp_map10 sweep on the fused wrapper with and without value_stats
                                                            (eight CommBaseCritics as baselines): both warmed, the unchanged keys
                                                            compared (==), then five alternating rounds of whole calls.  `off`:
                                                            the five rounds without the switch only, passing no keyword of it - the
                                                            leg a checkout that predates the switch can run, for alternating the two
                                                            trees in one job
    python tools/eval_sweep_time.py value_parts             the same round played once, then its parts on their own (device events,
                                                            five repetitions each): the critics' recorded, mute and lossless replays
                                                            and the cm_value_stats launch (DESIGN.md §7 "Critic statistics")"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from com_marl_amd import envs as E, nets  # noqa: E402
from com_marl_amd.evaluate import eval_summary, eval_sweep  # noqa: E402

T, ROUNDS, SEED = 200, 3, 3
PP = dict(load=2, max_env_steps=T, capture_reward=10, step_cost=0.1, rm=0, penalty=0, grid_size=10, Rsen=1, n_agents=4, n_preys=4,
          n_gcn_layers=2, mode="test", teRcom=9, tepl=0)
CO = dict(load=2, max_env_steps=T, capture_reward=2, step_cost=0, rm=0, penalty=1, revisit_penalty=0.5, lazy_penalty=1, grid_size=20,
          Rsen=2, n_agents=24, n_preys=0, n_gcn_layers=2, mode="test", teRcom=19, tepl=0, obstComplex="Easy", add_clock=0)
WORKLOADS = {
    "pp_map10": dict(cls=E.PredatorPreyWrapper, params=PP, envs=4096, K=8, channel="IID",
                     conditions=[dict(Rcom=r, pl=p) for r in (9, 3, 2, 1) for p in (0.0, 0.5)]),
    "pp_map10_k1": dict(cls=E.PredatorPreyWrapper, params=PP, envs=4096, K=1, channel="IID",
                        conditions=[dict(Rcom=r, pl=p) for r in (9, 3, 2, 1) for p in (0.0, 0.5)]),
    "co_map20": dict(cls=E.CoverageWrapper, params=CO, envs=1024, K=4, channel="GE",
                     conditions=[dict(Rcom=r, Pgb=g, Pbg=b) for r in (19, 4) for g, b in ((0.0196, 0.282), (0.3, 0.1))]),
}
COND_TO_PARAM = dict(Rcom="teRcom", pl="tepl", Pgb="Pgb", Pbg="Pbg")


def with_condition(params, cond):
    p = dict(params)
    p.update({COND_TO_PARAM[k]: v for k, v in cond.items()})
    return p


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def run(name):
    w = WORKLOADS[name]
    cls, params, B, K, channel, conds = w["cls"], w["params"], w["envs"], w["K"], w["channel"], w["conditions"]
    C_ = len(conds)
    n_epi = B // (K * C_)
    kw = dict(n_eval_episodes=n_epi, max_env_steps=T, eval_greedy=True)
    sweep_wrapper = lambda fused=False: cls(True, params=params, n_envs=B, device="cuda:0", seed=SEED, channel=channel,   # noqa: E731
                                            conditions=conds, fused_conditions=fused)
    fused_leg = params["n_agents"] == 4 and cls is E.PredatorPreyWrapper    # the shapes the wave-owned rollout covers
    uniform_wrappers = lambda n: [cls(True, params=with_condition(params, c), n_envs=n, device="cuda:0", seed=SEED,   # noqa: E731
                                      channel=channel) for c in conds]
    first = sweep_wrapper()
    pols = []
    for k in range(K):
        torch.manual_seed(k)
        p = nets.CommCategoricalMLPPolicy(first.spec, n_agents=params["n_agents"], device="cuda:0")
        p.set_rng(SEED)
        pols.append(p)
    who = pols if K > 1 else pols[0]                                        # one policy: the single-policy engine, not a set of one
    as_grid = lambda res: res if K > 1 else [res]                           # noqa: E731
    sweep = lambda env: as_grid(eval_sweep(env, who, 0, paired=True, **kw))                             # noqa: E731
    sequential = lambda envs: [as_grid(eval_summary(env, who, 0, **kw)) for env in envs]                # noqa: E731
    # warm-up of both sides and the comparison
    _, got = sync_time(lambda: sweep(first))
    _, ref = sync_time(lambda: sequential(uniform_wrappers(B // C_)))
    if fused_leg:
        _, got_f = sync_time(lambda: sweep(sweep_wrapper(True)))
        same_f = all(got_f[0][c] == got[0][c] for c in range(C_))
        print(f"{name}: cells of policy 0 on the fused wrapper equal the unfused sweep's: {same_f}", flush=True)
    ref0 = [eval_summary(env, pols[0], 0, **kw) for env in uniform_wrappers(n_epi)]                     # policy 0's cells, paired ids
    same = all({k: v for k, v in got[0][c].items() if k != "condition"} == ref0[c] for c in range(C_))
    print(f"{name}: cells of policy 0 equal eval_summary on the uniform wrappers: {same}", flush=True)
    for c in range(C_):
        print(f"  {conds[c]}: success {[round(got[k][c]['success'], 3) for k in range(K)]} "
              f"(sequential, other episodes: {[round(ref[c][k]['success'], 3) for k in range(K)]})", flush=True)
    rounds = {"eval_sweep_fused": [], "eval_sweep": [], "sequential": []}
    for r in range(ROUNDS):
        if fused_leg:
            env = sweep_wrapper(True)
            dt, _ = sync_time(lambda: sweep(env))
            rounds["eval_sweep_fused"].append(dt)
            print(f"[{r}] {name} eval_sweep, fused wrapper   1 call,  {B} envs, {K} x {C_} cells x {n_epi} episodes: {dt * 1e3:9.2f} ms", flush=True)
        env = sweep_wrapper()
        dt, _ = sync_time(lambda: sweep(env))
        rounds["eval_sweep"].append(dt)
        print(f"[{r}] {name} eval_sweep   1 call,  {B} envs, {K} x {C_} cells x {n_epi} episodes: {dt * 1e3:9.2f} ms", flush=True)
        envs = uniform_wrappers(B // C_)
        dt, _ = sync_time(lambda: sequential(envs))
        rounds["sequential"].append(dt)
        print(f"[{r}] {name} sequential   {C_} calls, {B // C_} envs each, {K} policies x {n_epi} episodes: {dt * 1e3:9.2f} ms", flush=True)
    print(json.dumps({"workload": name, "envs": B, "policies": K, "conditions": C_, "episodes_per_cell": n_epi, "steps": T,
                      "policy0_cells_equal": bool(same),
                      **({"fused_policy0_cells_equal": bool(same_f),
                          "eval_sweep_fused_ms": [round(x * 1e3, 3) for x in rounds["eval_sweep_fused"]],
                          "fused_ahead_of_unfused_in_every_round_against_every_round":
                              bool(max(rounds["eval_sweep_fused"]) < min(rounds["eval_sweep"])),
                          "fused_ahead_of_sequential_in_every_round_against_every_round":
                              bool(max(rounds["eval_sweep_fused"]) < min(rounds["sequential"]))} if fused_leg else {}),
                      "eval_sweep_ms": [round(x * 1e3, 3) for x in rounds["eval_sweep"]],
                      "sequential_ms": [round(x * 1e3, 3) for x in rounds["sequential"]],
                      "sweep_ahead_in_every_round_against_every_round": bool(max(rounds["eval_sweep"]) < min(rounds["sequential"]))}),
          flush=True)
    return same and (not fused_leg or same_f)


def _value_setup():
    """The pp_map10 workload's fused wrapper factory, its 8 policies and 8 critics of seeded weights."""
    w = WORKLOADS["pp_map10"]
    wrapper = lambda: w["cls"](True, params=w["params"], n_envs=w["envs"], device="cuda:0", seed=SEED, channel=w["channel"],   # noqa: E731
                               conditions=w["conditions"], fused_conditions=True)
    first = wrapper()
    pols, critics = [], []
    for k in range(w["K"]):
        torch.manual_seed(k)
        p = nets.CommCategoricalMLPPolicy(first.spec, n_agents=4, device="cuda:0")
        p.set_rng(SEED)
        pols.append(p)
        critics.append(nets.CommBaseCritic(first.spec, n_agents=4, device="cuda:0"))
    return w, wrapper, first, pols, critics


def value_stats(off_only):
    """eval_sweep of the pp_map10 workload on the fused wrapper, with and without value_stats, alternating (off_only: without)."""
    w, wrapper, first, pols, critics = _value_setup()
    B, K, C_, rounds_n = w["envs"], w["K"], len(w["conditions"]), 5
    n_epi = B // (K * C_)
    kw = dict(n_eval_episodes=n_epi, max_env_steps=T, eval_greedy=True, paired=True)
    call = lambda env, flag: eval_sweep(env, pols, 0, **kw, **(dict(value_stats=True, baselines=critics) if flag else {}))   # noqa: E731
    _, ref = sync_time(lambda: call(first, False))
    same = None
    if not off_only:
        from com_marl_amd.evaluate import VALUE_KEYS
        _, got = sync_time(lambda: call(wrapper(), True))
        same = all(got[k][c][key] == v for k in range(K) for c in range(C_) for key, v in ref[k][c].items())
        print(f"every key of the sweep without value_stats is unchanged with it: {same}", flush=True)
        for c in range(C_):
            print(f"  {w['conditions'][c]}: success {got[0][c]['success']:.3f} " + " ".join(f"{key} {got[0][c][key]:.3e}" for key in VALUE_KEYS),
                  flush=True)
    ms = {True: [], False: []}
    for r in range(rounds_n):
        for flag in ((False,) if off_only else (True, False)):
            env = wrapper()
            dt, _ = sync_time(lambda: call(env, flag))
            ms[flag].append(dt * 1e3)
            print(f"[{r}] eval_sweep {K} x {C_} cells x {n_epi} episodes, {B} envs, value_stats={flag}: {dt * 1e3:9.2f} ms", flush=True)
    print(json.dumps({"workload": "pp_map10 fused", "envs": B, "policies": K, "conditions": C_, "steps": T, "unchanged_keys_equal": same,
                      "with_value_stats_ms": [round(x, 3) for x in ms[True]], "without_ms": [round(x, 3) for x in ms[False]]}), flush=True)
    return same is not False


def value_parts():
    """The pp_map10 round played once on the fused wrapper, then the critics' three replays and cm_value_stats, each on its own."""
    from com_marl_amd import _lib as L
    from com_marl_amd.evaluate import sweep_layout
    from com_marl_amd.rollout import RolloutEngine
    w, _, env, pols, critics = _value_setup()
    B, K, C_, reps = w["envs"], w["K"], len(w["conditions"]), 5
    batch = getattr(env, "env", env).batch
    ps = nets.PolicySet(pols)
    batch.set_conditions(w["conditions"], *sweep_layout(B, K, C_, batch.cfg.env_id_offset, True))
    ps.sync_weights()
    for c in critics:
        c.sync_weights()
    ps.reset([True] * (B // K))
    eng = RolloutEngine(batch, ps, T, store_attn=False, store_probs=False, groups=[B // K] * K)
    eng.reset()
    eng.play(0, T, greedy=True, chunk=True)
    eng.bump(T)
    values, mute, lossless = (torch.empty(T, B, device="cuda") for _ in range(3))
    stats = torch.empty(T, B, L.VALUE_COLS, dtype=torch.float64, device="cuda")
    lib, st = L.lib(), L.current_stream()

    def timed(job):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        job()
        b.record()
        torch.cuda.synchronize()
        return round(a.elapsed_time(b) * 1e3, 1)                             # us

    jobs = {
        "round (reset + play)": lambda: (eng.reset(), eng.play(0, T, greedy=True, chunk=True)),
        "recorded replay": lambda: eng.replay_values(0, T, "recorded", critics, values),
        "mute replay": lambda: eng.replay_values(0, T, "identity", critics, mute),
        "lossless replay": lambda: eng.replay_values(0, T, "ones", critics, lossless),
        "cm_value_stats": lambda: L.check(lib.cm_value_stats(T, B, L.ptr(eng.reward64), L.ptr(eng.path_len), L.ptr(values), L.ptr(mute),
                                                             L.ptr(lossless), 0.99, L.ptr(stats), st), "cm_value_stats"),
        "cm_value_stats, no counterfactuals": lambda: L.check(lib.cm_value_stats(T, B, L.ptr(eng.reward64), L.ptr(eng.path_len), L.ptr(values),
                                                                                 None, None, 0.99, L.ptr(stats), st), "cm_value_stats"),
    }
    res = {}
    for name, job in jobs.items():
        timed(job)
        res[name] = [timed(job) for _ in range(reps)]
        print(f"{name}: {res[name]} us", flush=True)
    print(json.dumps({"workload": "pp_map10 fused", "envs": B, "policies": K, "steps": T, "us": res,
                      "mean_stats_row": stats.mean((0, 1)).tolist()}), flush=True)


def kernels():
    """300 cm_env_step launches of a uniform batch, then 300 of a conditions batch in which every env has that same condition:
    the same work per launch, env_kernel* against env_cond_kernel*."""
    shapes = [("pp_map10 N=4 x 4096 (16 lanes per env)", "pp", PP, 4096, "IID", dict(Rcom=3, pl=0.3)),
              ("pp_map10 N=9 x 8192 (32 lanes per env)", "pp", dict(PP, n_agents=9), 8192, "IID", dict(Rcom=3, pl=0.3)),
              ("pp_map10 N=9 x 2048 (64 lanes per env)", "pp", dict(PP, n_agents=9), 2048, "IID", dict(Rcom=3, pl=0.3)),
              ("co_map20 N=24 x 1024 (wide)", "co", CO, 1024, "GE", dict(Rcom=4, Pgb=0.3, Pbg=0.1))]
    steps = 300
    for label, scen, params, B, channel, cond in shapes:
        N = params["n_agents"]
        g = torch.Generator().manual_seed(0)
        acts = torch.randint(0, 5, (steps, B, N), generator=g, dtype=torch.int32).to("cuda:0")
        for kind in ("uniform", "conditions", "uniform", "conditions"):
            kw = dict(conditions=[cond]) if kind == "conditions" else {}
            env = E.GridEnvBatch(scen, with_condition(params, cond), B, device="cuda:0", seed=SEED, channel=channel, **kw)
            env.reset_all()
            dt, _ = sync_time(lambda: [env.step_device(a) for a in acts])
            env.check_status()
            print(f"{label}: {kind:10s} {steps} steps, host clock {dt / steps * 1e6:7.2f} us per step (launch-bound where small)", flush=True)


def rollout_kernels():
    """A 200-step chunk, three times, on a uniform IID range-3 batch - adjacency and channels change every step: the non-carried
    rollout_w_kernel - and on a fused conditions batch of the same shape whose every env has that condition (rollout_wc_kernel)."""
    from com_marl_amd.rollout import RolloutEngine
    cond, B = dict(Rcom=3, pl=0.3), 4096
    for kind in ("uniform", "conditions", "uniform", "conditions"):
        kw = dict(conditions=[cond], fused_conditions=True) if kind == "conditions" else {}
        env = E.GridEnvBatch("pp", with_condition(PP, cond), B, device="cuda:0", seed=SEED, channel="IID", **kw)
        spec = E.EnvSpec(E._Box([0.0] * (env.d * env.N), [1.0] * (env.d * env.N)), E._Discrete(5))
        torch.manual_seed(0)
        pol = nets.CommCategoricalMLPPolicy(spec, n_agents=4, device="cuda:0")
        pol.set_rng(SEED)
        eng = RolloutEngine(env, pol, T)
        pol.sync_weights()
        for r in range(3):
            eng.reset()
            dt, ok = sync_time(lambda: eng.steps_fused(0, T))
            assert ok, "the chunk was not one launch"
            eng.bump(T)
            env.check_status()
            print(f"rollout chunk, {kind:10s} [{r}] {T} steps x {B} envs in one launch: {dt / T * 1e6:7.2f} us per step (host clock)", flush=True)


if __name__ == "__main__":
    if sys.argv[1:] == ["kernels"]:
        kernels()
        sys.exit(0)
    if sys.argv[1:] == ["rollout_kernels"]:
        rollout_kernels()
        sys.exit(0)
    if sys.argv[1:2] == ["value_stats"] and sys.argv[2:] in ([], ["off"]):
        sys.exit(0 if value_stats(sys.argv[2:] == ["off"]) else 1)
    if sys.argv[1:] == ["value_parts"]:
        value_parts()
        sys.exit(0)
    names = sys.argv[1:] or list(WORKLOADS)
    ok = [run(name) for name in names]
    sys.exit(0 if all(ok) else 1)
