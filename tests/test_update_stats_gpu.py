"""Per-step PPO update statistics and the device-side KL early stop on the GPU: cm_ppo_update_stats against float64 torch, the
gated Adam against the ungated one, and whole train_once runs in the deterministic update mode, where "the policy stopped after
exactly j steps" is bit equality with a run scheduled for j steps (DESIGN.md "Update statistics and the KL early stop")."""
import copy
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_TIMING = ("EpochTime", "TrainOnceTime", "GPUMemoryMax")
_NEW_STATS = ("PolicySteps", "ApproxKL", "ClipFraction")
CLIP = 0.1
EPS32 = 1.1920928955078125e-07


@pytest.fixture
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need the MI355X")
    return torch


@pytest.fixture
def det_on(gpu):
    import com_marl_amd
    com_marl_amd.set_deterministic(True)
    yield gpu
    com_marl_amd.set_deterministic(None)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the kernel against float64 torch
# ---------------------------------------------------------------------------------------------------------------------------
def _categorical64(torch, logits):
    """The loss's Categorical in f64: softmax renormalised twice, log(clamp(p, eps32, 1 - eps32)) -> (log-probs, probs)."""
    p = torch.softmax(logits.double(), -1)
    p = p / p.sum(-1, keepdim=True)
    p = p / p.sum(-1, keepdim=True)
    return torch.log(p.clamp(EPS32, 1.0 - EPS32)), p


def _case(torch, P, T, N, A, lens):
    """Inputs as the issue states them and the f64 reference row, computed once per case."""
    g = torch.Generator().manual_seed(1000 * P + 10 * T + N + A)
    logits = torch.randn(P, T, N, A, generator=g).cuda()
    actions = torch.randint(0, A, (P, T, N), generator=g, dtype=torch.int32).cuda()
    lens_t = (torch.randint(1, T + 1, (P,), generator=g, dtype=torch.int32) if lens is None
              else torch.tensor(lens, dtype=torch.int32)).cuda()
    lg, p = _categorical64(torch, logits)
    new_ll = lg.gather(-1, actions.long().unsqueeze(-1)).squeeze(-1).sum(-1)          # [P,T] f64
    ent = -(lg * p).sum(-1).mean(-1)
    r = (0.7 + 0.6 * torch.rand(P, T, generator=g, dtype=torch.float64)).cuda()
    for _ in range(50):                        # no row within 1e-3 of the clip boundary, judged on the inputs the kernel gets
        old_ll = (new_ll - torch.log(r)).float()
        lr = new_ll - old_ll.double()
        near = ((torch.exp(lr) - 1).abs() - CLIP).abs() < 1e-3
        if not bool(near.any()):
            break
        r = torch.where(near, (0.7 + 0.6 * torch.rand(P, T, generator=g, dtype=torch.float64)).cuda(), r)
    valid = torch.arange(T, device="cuda")[None, :] < lens_t[:, None]
    ratio = torch.exp(lr)
    assert float((((ratio - 1).abs() - CLIP).abs())[valid].min()) >= 1e-3 if bool(valid.any()) else True
    n = int(valid.sum())
    if n:
        mean = lambda x: float(x[valid].sum() / n)                                          # noqa: E731
        ref = dict(n_valid=float(n), approx_kl=mean(torch.expm1(lr) - lr), kl=mean(-lr),
                   clip_frac=float(((ratio - 1).abs() > CLIP)[valid].sum()) / n, ratio_min=float(ratio[valid].min()),
                   ratio_max=float(ratio[valid].max()), entropy=mean(ent), stopped=0.0)
    else:
        ref = dict.fromkeys(("n_valid", "approx_kl", "kl", "clip_frac", "ratio_min", "ratio_max", "entropy", "stopped"), 0.0)
    return logits, actions, old_ll, lens_t, ref


def _launch(torch, L, shape, tensors, kl_stop, rows, cursor, gate, ws, nb):
    P, T, N, A = shape
    logits, actions, old_ll, lens_t = tensors
    L.check(L.lib().cm_ppo_update_stats(P, T, N, A, L.ptr(logits), L.ptr(actions), L.ptr(old_ll), L.ptr(lens_t), CLIP, float(kl_stop),
                                        L.ptr(rows), rows.shape[0], L.ptr(cursor), L.ptr(gate), L.ptr(ws), nb, L.current_stream()),
            "cm_ppo_update_stats")


@pytest.mark.parametrize("P,T,N,A,lens", [(1, 1, 1, 2, None), (3, 7, 4, 5, [7, 0, 4]), (5, 300, 24, 5, None), (4, 9, 3, 8, None),
                                          (300, 250, 4, 5, None), (2, 3, 4, 5, [0, 0])])
def test_row_against_float64(P, T, N, A, lens, gpu):
    torch = gpu
    from com_marl_amd import _lib as L
    *tensors, ref = _case(torch, P, T, N, A, lens)
    shape = (P, T, N, A)
    nb = L.lib().cm_ppo_update_stats_ws_bytes(P, T)
    ws = torch.full((nb // 8,), float("nan"), dtype=torch.float64, device="cuda")          # a missed partial shows
    rows = torch.full((4, L.UPD_COLS), -7.0, dtype=torch.float64, device="cuda")
    cursor = torch.zeros(1, dtype=torch.int32, device="cuda")
    _launch(torch, L, shape, tensors, 0.0, rows, cursor, None, ws, nb)                     # gate = NULL works
    _launch(torch, L, shape, tensors, 0.0, rows, cursor, None, ws, nb)                     # the same buffers again
    got = rows.cpu().numpy()
    assert int(cursor.item()) == 2
    assert got[0].tobytes() == got[1].tobytes(), (got[0], got[1])                          # the workspace resets itself
    assert (got[2:] == -7.0).all()
    row = dict(zip(L.UPD_COLUMNS, got[0]))
    dev = {k: abs(row[k] - ref[k]) for k in ref}
    print(f"\n{shape}: n_valid {ref['n_valid']:.0f}, deviations from f64: " + ", ".join(f"{k} {v:.3g}" for k, v in dev.items()))
    assert row["n_valid"] == ref["n_valid"] and row["clip_frac"] == ref["clip_frac"] and row["stopped"] == ref["stopped"] == 0.0
    assert dev["kl"] <= 1e-5 and dev["entropy"] <= 1e-5
    assert dev["approx_kl"] <= 1e-6
    assert dev["ratio_min"] <= 5e-5 * abs(ref["ratio_min"]) and dev["ratio_max"] <= 5e-5 * abs(ref["ratio_max"])
    if ref["n_valid"] == 0:
        assert not got[0].any()                                                            # a row of zeros

    # the decision: a threshold just below / just above the f64 approx_kl (5e-6 away: the row's bound is 1e-6)
    for kl_stop in (ref["approx_kl"] - 5e-6, ref["approx_kl"] + 5e-6, float("nan"), -1.0):
        expect = int(kl_stop > 0 and ref["n_valid"] > 0 and ref["approx_kl"] > kl_stop)
        gate = torch.zeros(1, dtype=torch.int32, device="cuda")
        cursor.zero_()
        _launch(torch, L, shape, tensors, kl_stop, rows, cursor, gate, ws, nb)
        assert int(gate.item()) == expect and float(rows[0, L.UPD_COLUMNS.index("stopped")]) == expect, kl_stop
        if expect:                                                                         # sticky: a later row below the threshold
            _launch(torch, L, shape, tensors, 0.0, rows, cursor, gate, ws, nb)
            assert int(gate.item()) == 1 and float(rows[1, L.UPD_COLUMNS.index("stopped")]) == 1.0
            assert rows[0, :7].cpu().numpy().tobytes() == rows[1, :7].cpu().numpy().tobytes()
    gate = torch.ones(1, dtype=torch.int32, device="cuda")                                 # already set: stays set whatever the row
    cursor.fill_(3)
    _launch(torch, L, shape, tensors, 0.0, rows, cursor, gate, ws, nb)
    assert int(gate.item()) == 1 and float(rows[3, L.UPD_COLUMNS.index("stopped")]) == 1.0 and int(cursor.item()) == 4
    _launch(torch, L, shape, tensors, 0.0, rows, cursor, gate, ws, nb)                     # a cursor past the table: the last row
    assert int(cursor.item()) == 5 and float(rows[3, 0]) == ref["n_valid"]


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the gated Adam
# ---------------------------------------------------------------------------------------------------------------------------
def test_gated_adam(gpu):
    torch = gpu
    from com_marl_amd import _lib as L
    g = torch.Generator().manual_seed(3)
    sizes = [1, 255, 257, 70000]
    n = len(sizes)
    base = {k: [torch.randn(s, generator=g).cuda() * sc for s in sizes] for k, sc in (("p", 1.0), ("g", 1.0), ("m", 0.1))}
    base["v"] = [torch.rand(s, generator=g).cuda() * 0.01 for s in sizes]
    pre_norm = float(torch.cat(base["g"]).double().norm())
    max_norm = 1.0
    assert max_norm < pre_norm                                                             # the clip is active
    host = torch.zeros(256, 2, dtype=torch.float32)
    L.lib().cm_adam_bias_corrections(0.9, 0.999, 5, 10, host.data_ptr())
    table, cursor = host.cuda(), torch.full((1,), 2, dtype=torch.int32, device="cuda")

    def run(name, gate):
        t = {k: [x.clone() for x in v] for k, v in base.items()}
        norm = torch.full((65,), float("nan"), device="cuda")
        arr = lambda ts: (C.c_void_p * n)(*[x.data_ptr() for x in ts])                    # noqa: E731
        args = (n, arr(t["p"]), arr(t["g"]), arr(t["m"]), arr(t["v"]), (C.c_int64 * n)(*sizes), norm.data_ptr(), max_norm, 3e-4, 0.9,
                0.999, 1e-5, table.data_ptr(), cursor.data_ptr(), 256)
        if gate is not None:
            gt = torch.full((1,), gate, dtype=torch.int32, device="cuda")
            args += (gt.data_ptr(),)
        L.check(getattr(L.lib(), name)(*args, L.current_stream()), name)
        torch.cuda.synchronize()
        if gate is not None:
            assert int(gt.item()) == gate                                                  # read, never written
        return t, float(norm[0])

    ref, ref_norm = run("cm_multi_adam_step_dev", None)
    assert ref_norm == pytest.approx(pre_norm ** 2, rel=1e-4)
    assert not torch.equal(ref["p"][3], base["p"][3]) and not torch.equal(ref["g"][3], base["g"][3])   # it stepped and clipped
    open_, open_norm = run("cm_multi_adam_step_gated", 0)
    shut, shut_norm = run("cm_multi_adam_step_gated", 1)
    assert open_norm == ref_norm and shut_norm == ref_norm
    for k in "pgmv":
        for i in range(n):
            assert torch.equal(open_[k][i], ref[k][i]), (k, i)
            assert torch.equal(shut[k][i], base[k][i]), (k, i)


# ---------------------------------------------------------------------------------------------------------------------------
# whole train_once runs
# ---------------------------------------------------------------------------------------------------------------------------
def _make(torch, kind="comm", B=16, mpl=10, seed=5, **algo_kw):
    from com_marl_amd import envs as E, nets
    from com_marl_amd.algos import CentralizedMAPPO
    from com_marl_amd.sampler import CentralizedMAOnPolicyVectorizedSampler
    params = dict(load=2, max_env_steps=mpl, capture_reward=10, step_cost=0.1, rm=0, penalty=0, grid_size=10, Rsen=1, n_agents=4,
                  n_preys=4, n_gcn_layers=2, mode="train", trRcom=9, trpl=0, seed=seed)
    env = E.PredatorPreyWrapper(centralized=True, params=params, n_envs=B, device="cuda:0")
    torch.manual_seed(seed)
    N = env.n_agents
    if kind == "obsdp":
        pol = nets.DecCategoricalMLPPolicy(env.spec, N, hidden_sizes=[128, 64, 32], device="cuda:0")
    else:
        pol = nets.CommCategoricalMLPPolicy(env.spec, n_agents=N, device="cuda:0")
    crit = nets.CommBaseCritic(env.spec, n_agents=N, device="cuda:0")
    pol.set_rng(seed)
    kw = dict(max_path_length=mpl, discount=0.99, positive_adv=False, gae_lambda=0.97, policy_ent_coeff=0.1, clip_grad_norm=7,
              optimization_n_minibatches=1, optimization_mini_epochs=6, device="cuda:0", entropy_method="regularized", center_adv=True,
              stop_entropy_gradient=False)
    kw.update(algo_kw)
    algo = CentralizedMAPPO(env_spec=env.spec, policy=pol, baseline=crit, **kw)
    smp = CentralizedMAOnPolicyVectorizedSampler(algo, env, n_envs=B)
    smp.start_worker()
    return env, pol, crit, algo, smp, B * N * mpl


def _opt_state(opt):
    out = {}
    for i, st in opt.state_dict()["state"].items():
        for k, v in st.items():
            out[f"{i}.{k}"] = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
    return out


def _run(torch, epochs=1, repeat_last_paths=False, **algo_kw):
    """A fresh sampler + `epochs` train_once (the last one on the paths of the one before when asked) -> what it left behind."""
    env, pol, crit, algo, smp, batch = _make(torch, **algo_kw)
    per_epoch, paths = [], None
    for itr in range(epochs):
        if not (repeat_last_paths and itr == epochs - 1):
            paths = smp.obtain_samples(itr, batch_size=batch)
        np.random.seed(100 + itr)
        algo.train_once(itr=itr, paths=paths)
        per_epoch.append(dict(stats={k: v for k, v in algo.stats.items() if k not in _TIMING},
                              rows=None if algo.update_rows is None else {k: v.copy() for k, v in algo.update_rows.items()}))
    env.batch.check_status()
    return dict(pol={k: v.detach().cpu().numpy() for k, v in pol.state_dict().items()},
                crit={k: v.detach().cpu().numpy() for k, v in crit.state_dict().items()},
                opt=_opt_state(algo._optimizer), bopt=_opt_state(algo._baseline_optimizer), epochs=per_epoch, algo=algo)


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    bad = [k for k in a if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True)]
    assert not bad, (what, bad[:10])


def _steps(opt_state):
    return {int(v) for k, v in opt_state.items() if k.endswith(".step")}


def _rows_bytes(rows, k):
    from com_marl_amd import _lib as L
    return b"".join(np.float64(rows[c][k]).tobytes() for c in L.UPD_COLUMNS)


def _pick_stop(k, j_max):
    """The largest j <= j_max with k_j above every earlier row's approx_kl (j = 1 always qualifies: k_0 is ~0) and the target_kl
    whose threshold 1.5 * target_kl lies midway between that row and the largest before it."""
    j = max(j for j in range(1, j_max + 1) if k[j] > k[:j].max())
    return j, (k[:j].max() + k[j]) / 2 / 1.5


_STOP_RUNS = []


@pytest.fixture
def stop_runs(det_on, monkeypatch):
    """Runs A (stats only), B (target_kl stopping in front of step j), C (scheduled for j steps) and D (everything off), on the same
    seeds: PP map10, teams of 4, 16 envs x 10 steps, one minibatch x 6 mini-epochs, graphs forced.  Run once, shared, left unchanged."""
    torch = det_on
    monkeypatch.setenv("COMMARL_UPDATE_GRAPH", "1")
    if _STOP_RUNS:
        return (torch,) + _STOP_RUNS[0]
    A = _run(torch, update_stats=True, target_kl=None)
    k = A["epochs"][0]["rows"]["approx_kl"]
    assert len(k) == 6 and k[1] > k[0]
    j, target = _pick_stop(k, 4)
    B = _run(torch, target_kl=target)
    Cr = _run(torch, update_stats=True, target_kl=None, optimization_mini_epochs=j)
    D = _run(torch, update_stats=False, target_kl=None)
    print(f"\napprox_kl per step {k}, stop in front of step {j} (target_kl {target:.3g})")
    _STOP_RUNS.append((A, B, Cr, D, j, target))
    return torch, A, B, Cr, D, j, target


def test_the_stop_is_exact(stop_runs):
    torch, A, B, Cr, D, j, target = stop_runs
    ra, rb = A["epochs"][0]["rows"], B["epochs"][0]["rows"]
    assert rb["stopped"].tolist() == [0.0] * j + [1.0] * (6 - j)
    assert ra["stopped"].tolist() == [0.0] * 6
    assert rb["mini_epoch"].tolist() == list(range(6)) and rb["minibatch"].tolist() == [0] * 6
    for c in ra:
        if c not in ("stopped", "mini_epoch", "minibatch"):
            assert ra[c][:j + 1].tobytes() == rb[c][:j + 1].tobytes(), c                   # rows 0..j: the same weights judged
            assert all(rb[c][i].tobytes() == rb[c][j].tobytes() for i in range(j, 6)), c    # rows j..5: the weights are frozen
    st = B["epochs"][0]["stats"]
    assert st["PolicySteps"] == j and st["ApproxKL"] == rb["approx_kl"].max() and st["ApproxKL"] > 1.5 * target
    assert st["ClipFraction"] == rb["clip_frac"][:j].mean()
    assert B["algo"]._update_graphs.captured > 0 and not B["algo"]._update_graphs.broken
    # the policy is the one a j-step schedule leaves, bit for bit; the critic took all six steps
    _same(B["pol"], Cr["pol"], "policy parameters")
    _same(B["opt"], Cr["opt"], "policy moments and step")
    assert _steps(B["opt"]) == {j}
    assert B["epochs"][0]["stats"]["GradNorm"] == Cr["epochs"][0]["stats"]["GradNorm"]      # over the applied steps only
    _same(B["crit"], A["crit"], "critic parameters")
    _same(B["bopt"], A["bopt"], "critic moments and step")
    assert _steps(B["bopt"]) == {6}
    # the statistics change no bit
    for what in ("pol", "crit", "opt", "bopt"):
        _same(A[what], D[what], what)
    sa, sd = A["epochs"][0]["stats"], D["epochs"][0]["stats"]
    assert set(sa) - set(sd) == set(_NEW_STATS) and D["epochs"][0]["rows"] is None
    _same({k: sa[k] for k in sd}, sd, "stats")
    assert sa["PolicySteps"] == 6


def test_eager_steps_equal_replayed_ones_under_the_gate(stop_runs, monkeypatch):
    torch, A, B, Cr, D, j, target = stop_runs
    monkeypatch.setenv("COMMARL_UPDATE_GRAPH", "0")
    E = _run(torch, target_kl=target)
    assert getattr(E["algo"], "_update_graphs", None) is None
    for what in ("pol", "crit", "opt", "bopt"):
        _same(B[what], E[what], what)
    _same(B["epochs"][0]["stats"], E["epochs"][0]["stats"], "stats")
    _same(B["epochs"][0]["rows"], E["epochs"][0]["rows"], "rows")


def test_epoch_boundaries(det_on, monkeypatch):
    """Three minibatches x 10 mini-epochs, graphs on, three epochs, the third on the second's paths (so its steps replay the second's
    graphs): cursor and gate start every epoch afresh, the optimisers' host-side step counts follow the device."""
    torch = det_on
    monkeypatch.setenv("COMMARL_UPDATE_GRAPH", "1")
    kw = dict(optimization_n_minibatches=3, optimization_mini_epochs=10)
    S = _run(torch, update_stats=True, **kw)
    k = S["epochs"][0]["rows"]["approx_kl"]
    assert len(k) == 30
    j, target = _pick_stop(k, 15)
    G = _run(torch, epochs=3, repeat_last_paths=True, target_kl=target, **kw)
    applied = [e["stats"]["PolicySteps"] for e in G["epochs"]]
    print(f"\nstop in front of step {j} of epoch 0 (target_kl {target:.3g}); applied per epoch {applied}")
    assert applied[0] == j and G["epochs"][0]["rows"]["stopped"].tolist() == [0.0] * j + [1.0] * (30 - j)
    for e in G["epochs"]:
        r = e["rows"]
        assert len(r["stopped"]) == 30 and r["stopped"][0] == 0.0 and r["approx_kl"][0] < 1e-9
        assert r["minibatch"].tolist() == [0, 1, 2] * 10 and r["mini_epoch"].tolist() == [m for m in range(10) for _ in range(3)]
        n = int((r["stopped"] == 0).sum())
        assert e["stats"]["PolicySteps"] == n and r["stopped"].tolist() == [0.0] * n + [1.0] * (30 - n)     # sticky
        for i in range(n, 27):                                                              # frozen weights: the same minibatch again
            assert _rows_bytes(r, i) == _rows_bytes(r, i + 3), i
    assert _steps(G["opt"]) == {sum(applied)}
    assert _steps(G["bopt"]) == {90}
    ug = G["algo"]._update_graphs
    assert ug.reused >= 3 and not ug.broken


# ---------------------------------------------------------------------------------------------------------------------------
# 6. row 0 against an independent computation
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["comm", "obsdp"])
def test_row_zero_against_an_independent_computation(kind, gpu):
    torch = gpu
    env, pol, crit, algo, smp, batch = _make(torch, kind=kind, B=8, optimization_mini_epochs=2, update_stats=True)
    paths = smp.obtain_samples(0, batch_size=batch)
    before = copy.deepcopy(pol)
    obs, _, actions, rewards, valids, baselines, returns, dist_adjs, channels = algo.process_samples(0, paths)
    with torch.no_grad():
        logits = before._logits(obs, dist_adjs, channels)
    lg, p = _categorical64(torch, logits)
    valid = torch.arange(obs.shape[1], device=obs.device)[None, :] < valids[:, None]
    n_valid = int(valid.sum())
    entropy = float((-(lg * p).sum(-1).mean(-1))[valid].sum() / n_valid)
    np.random.seed(1)
    algo.train_once(itr=0, paths=paths)
    r = algo.update_rows
    print(f"\n{kind}: n_valid {r['n_valid'][0]:.0f}, entropy {r['entropy'][0]:.9f} vs {entropy:.9f}, approx_kl[0] {r['approx_kl'][0]:.3g}")
    assert len(r["n_valid"]) == 2 and r["n_valid"][0] == n_valid
    assert abs(r["entropy"][0] - entropy) <= 1e-5
    assert r["approx_kl"][0] < 1e-9 and r["clip_frac"][0] == 0.0                           # the policy IS the old policy
    assert r["stopped"].tolist() == [0.0, 0.0] and algo.stats["PolicySteps"] == 2


# ---------------------------------------------------------------------------------------------------------------------------
# 7. off means off   8. refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_off_means_off(gpu, monkeypatch):
    from tests.lib_spy import _Spy
    from com_marl_amd import _lib as L
    torch = gpu
    monkeypatch.delenv("COMMARL_UPDATE_STATS", raising=False)
    monkeypatch.delenv("COMMARL_TARGET_KL", raising=False)
    monkeypatch.setenv("COMMARL_UPDATE_GRAPH", "1")
    env, pol, crit, algo, smp, batch = _make(torch, optimization_mini_epochs=4)
    paths = smp.obtain_samples(0, batch_size=batch)
    spy = _Spy(L.lib())
    monkeypatch.setattr(L, "lib", lambda: spy)
    np.random.seed(1)
    algo.train_once(itr=0, paths=paths)
    names = spy.names()
    assert "cm_ppo_surrogate" in names and "cm_multi_adam_step" in names and "cm_multi_adam_step_dev" in names
    assert not names & {"cm_ppo_update_stats", "cm_ppo_update_stats_ws_bytes", "cm_multi_adam_step_gated"}
    assert algo.update_rows is None and not set(algo.stats) & set(_NEW_STATS)
    assert getattr(algo, "_upd_state", None) is None


# ---------------------------------------------------------------------------------------------------------------------------
# 9. one owner of the device-step bookkeeping: the launches stay, an error leaves no optimiser armed
# ---------------------------------------------------------------------------------------------------------------------------
_SWITCHES = {"off": dict(update_stats=False, target_kl=None), "on": dict(update_stats=True, target_kl=None), "gated": dict(target_kl=1e9)}
_STEP_CALLS = ("cm_multi_adam_step", "cm_multi_adam_step_dev", "cm_multi_adam_step_gated", "cm_ppo_update_stats", "cm_ppo_surrogate",
               "cm_adam_bias_corrections")
_S, _A, _D, _G, _U, _B = "cm_ppo_surrogate", "cm_multi_adam_step", "cm_multi_adam_step_dev", "cm_multi_adam_step_gated", \
    "cm_ppo_update_stats", "cm_adam_bias_corrections"
# What the commit BEFORE the bookkeeping was folded into one owner printed for this test body on the MI355X, pasted: these
# sequences do not come from the code under test.  (First and last: the full-batch loss before / after the update.  With the
# graphs, mini-epoch 0 is eager, the first replayed step arms the optimisers not yet armed and is captured, a replay calls nothing.)
_PARENT_SEQUENCES = {
    ("off", "0"): [_S, _S, _A, _A, _S, _A, _A, _S, _A, _A, _S],
    ("off", "1"): [_S, _S, _A, _A, _B, _B, _S, _D, _D, _S],
    ("on", "0"): [_S, _S, _U, _A, _A, _S, _U, _A, _A, _S, _U, _A, _A, _S],
    ("on", "1"): [_S, _S, _U, _A, _A, _B, _B, _S, _U, _D, _D, _S],
    ("gated", "0"): [_S, _B, _S, _U, _G, _A, _S, _U, _G, _A, _S, _U, _G, _A, _S],
    ("gated", "1"): [_S, _B, _S, _U, _G, _A, _B, _S, _U, _G, _D, _S],
}


@pytest.mark.parametrize("graph", ["0", "1"])
@pytest.mark.parametrize("switch", ["off", "on", "gated"])
def test_launch_sequence_is_the_parents(switch, graph, gpu, monkeypatch):
    """PP map10, teams of 4, 8 envs x 10 steps, 1 minibatch x 3 mini-epochs, a fresh algo: the ordered optimiser / statistics /
    loss entry points of one train_once, and the optimisers' host state after it."""
    from tests.lib_spy import _Spy
    from com_marl_amd import _lib as L
    torch = gpu
    monkeypatch.delenv("COMMARL_UPDATE_STATS", raising=False)
    monkeypatch.delenv("COMMARL_TARGET_KL", raising=False)
    monkeypatch.setenv("COMMARL_UPDATE_GRAPH", graph)
    env, pol, crit, algo, smp, batch = _make(torch, B=8, optimization_mini_epochs=3, **_SWITCHES[switch])
    paths = smp.obtain_samples(0, batch_size=batch)
    spy = _Spy(L.lib())
    monkeypatch.setattr(L, "lib", lambda: spy)
    np.random.seed(1)
    algo.train_once(itr=0, paths=paths)
    seq = [str(c) for c in spy.calls if c in _STEP_CALLS]
    print(f"\n({switch!r}, {graph!r}): {seq}")
    assert seq == _PARENT_SEQUENCES[switch, graph]
    assert algo._optimizer._dev_steps is None and algo._baseline_optimizer._dev_steps is None
    assert _steps(_opt_state(algo._baseline_optimizer)) == {3}
    assert _steps(_opt_state(algo._optimizer)) == {3}


def test_an_error_after_arming_leaves_no_optimiser_armed(gpu, monkeypatch):
    """target_kl arms the policy's optimiser before the update graphs are looked up: an error from there (plain Python, nothing
    faults) must leave both optimisers out of the device-step mode with nothing booked, and the next train_once must work."""
    from com_marl_amd import algos
    torch = gpu
    monkeypatch.setenv("COMMARL_UPDATE_GRAPH", "1")
    env, pol, crit, algo, smp, batch = _make(torch, B=8, optimization_mini_epochs=3, target_kl=1e9)
    paths = smp.obtain_samples(0, batch_size=batch)
    before = {k: v.clone() for k, v in pol.state_dict().items()}

    def boom(*a, **k):
        raise RuntimeError("no update graphs today")
    with monkeypatch.context() as m:
        m.setattr(algos._UpdateGraphs, "maybe", boom)
        np.random.seed(1)
        with pytest.raises(RuntimeError, match="no update graphs today"):
            algo.train_once(itr=0, paths=paths)
    assert algo._optimizer._dev_steps is None
    assert algo._baseline_optimizer._dev_steps is None
    assert all(torch.equal(v, before[k]) for k, v in pol.state_dict().items())
    assert _steps(_opt_state(algo._optimizer)) <= {0} and _steps(_opt_state(algo._baseline_optimizer)) <= {0}   # (never stepped: no
    np.random.seed(1)                                                                      # state, or the zero state of the arming)
    algo.train_once(itr=0, paths=paths)
    assert algo.stats["PolicySteps"] == 3
    assert algo._optimizer._dev_steps is None and algo._baseline_optimizer._dev_steps is None
    assert _steps(_opt_state(algo._optimizer)) == {3} and _steps(_opt_state(algo._baseline_optimizer)) == {3}


def test_refusals(gpu, monkeypatch):
    from com_marl_amd import _lib as L
    torch = gpu

    def attempt(match, exc=L.CommarlError, **kw):
        env, pol, crit, algo, smp, batch = _make(torch, B=8, **kw)
        paths = smp.obtain_samples(0, batch_size=batch)
        before = {k: v.clone() for k, v in pol.state_dict().items()}
        with pytest.raises(exc, match=match):
            algo.train_once(itr=0, paths=paths)
        assert all(torch.equal(v, before[k]) for k, v in pol.state_dict().items())         # refused before any step
    attempt("optim.Adam", target_kl=0.01, optimizer=torch.optim.Adam)
    attempt("optim.Adam", update_stats=True, optimizer=torch.optim.Adam)
    attempt("DEV_STEP_CAPACITY", target_kl=0.01, optimization_mini_epochs=257)
    attempt("DEV_STEP_CAPACITY", update_stats=True, optimization_mini_epochs=129, optimization_n_minibatches=2)
    monkeypatch.setenv("COMMARL_FUSED_LOSS", "0")
    attempt("fused PPO loss", target_kl=0.01)
