"""Deterministic update mode (com_marl_amd.set_deterministic): every cross-workgroup sum of the PPO update is
merged in a fixed order (slab twins of the atomic-merging kernels, include/commarl.h), so a whole training run - sampler plus
train_once - repeats bit for bit.  CPU part: the switch and the C ABI's refusals.  GPU part: the twins against float64 torch,
the reference's optimiser steps, whole runs compared with np.array_equal, and the switches that must not change a bit."""
import ctypes as C

import numpy as np
import pytest

# stats that measure the machine, not the training
_TIMING = ("EpochTime", "TrainOnceTime", "GPUMemoryMax")


@pytest.fixture
def det_off():
    import com_marl_amd
    yield com_marl_amd
    com_marl_amd.set_deterministic(None)


def test_switch_resolves(det_off, monkeypatch):
    import torch
    cm = det_off
    monkeypatch.delenv("COMMARL_DETERMINISTIC", raising=False)
    was = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(False)
        cm.set_deterministic(None)
        assert cm.deterministic() is False
        monkeypatch.setenv("COMMARL_DETERMINISTIC", "1")             # read on every call
        assert cm.deterministic() is True
        monkeypatch.setenv("COMMARL_DETERMINISTIC", "0")
        assert cm.deterministic() is False
        torch.use_deterministic_algorithms(True)
        assert cm.deterministic() is True
        cm.set_deterministic(False)                                    # explicit wins over both
        monkeypatch.setenv("COMMARL_DETERMINISTIC", "1")
        assert cm.deterministic() is False
        torch.use_deterministic_algorithms(False)
        monkeypatch.delenv("COMMARL_DETERMINISTIC")
        cm.set_deterministic(True)
        assert cm.deterministic() is True
        with pytest.raises(TypeError):
            cm.set_deterministic(1)
    finally:
        torch.use_deterministic_algorithms(was)


_TWINS = ("cm_linear_act_backward_det", "cm_encoder_backward_det", "cm_masked_agg_backward_det", "cm_linear_wgrad_det",
          "cm_ppo_surrogate_det", "cm_gauss_nll_forward_det")


def test_twins_are_exported():
    from com_marl_amd import _lib
    lib = _lib.lib()
    for n in _TWINS:
        assert n in _lib.EXPORTED and n + "_ws_bytes" in _lib.EXPORTED
        assert hasattr(lib, n) and hasattr(lib, n + "_ws_bytes")
    assert lib.cm_abi_version() == 3
    # _lib.launch's table: every twin reached, each with the default's leading arguments, then (slab, slab bytes, stream)
    assert {twin for twin, _ in _lib.TWINS.values()} == {n for n in _lib.EXPORTED if n.endswith("_det")} >= set(_TWINS)
    for name, (twin, ws_bytes) in _lib.TWINS.items():
        assert {name, twin, ws_bytes} <= set(_lib.EXPORTED), name
        args, twin_args = _lib._SIGNATURES[name][1], _lib._SIGNATURES[twin][1]
        n = len(twin_args) - 3
        assert twin_args[:n] == args[:n] and twin_args[n:] == [C.c_void_p, C.c_size_t, C.c_void_p], name


def _calls(ws, nb):
    """Each twin with plausible (never dereferenced) pointers and the given workspace: the check precedes every launch."""
    p = C.c_void_p(16)
    return {
        "cm_linear_act_backward_det": lambda L: L.cm_linear_act_backward_det(1000, 64, 64, p, p, 0, p, None, None, p, p, p, ws, nb, None),
        "cm_encoder_backward_det": lambda L: L.cm_encoder_backward_det(1000, 21, p, p, p, p, p, None, p, p, p, p, ws, nb, None),
        "cm_masked_agg_backward_det": lambda L: L.cm_masked_agg_backward_det(100, 4, 64, p, None, None, 0, p, p, None, p, p, p, p, ws, nb, None),
        "cm_linear_wgrad_det": lambda L: L.cm_linear_wgrad_det(1000, 64, 32, p, p, p, p, ws, nb, None),
        "cm_ppo_surrogate_det": lambda L: L.cm_ppo_surrogate_det(10, 15, 4, 5, p, p, p, p, p, 0.2, 0.1, 1, p, p, p, ws, nb, None),
        "cm_gauss_nll_forward_det": lambda L: L.cm_gauss_nll_forward_det(1000, 4, p, p, p, 0.0, 0, p, ws, nb, None),
    }


def test_twins_reject_missing_or_small_workspace():
    from com_marl_amd import _lib
    lib = _lib.lib()
    for name, call in _calls(None, 1 << 30).items():
        assert call(lib) == -1, name
        assert b"null slab workspace" in lib.cm_last_error(), name
    need = {"cm_linear_act_backward_det": lib.cm_linear_act_backward_det_ws_bytes(1000, 64, 64),
            "cm_encoder_backward_det": lib.cm_encoder_backward_det_ws_bytes(1000, 21),
            "cm_masked_agg_backward_det": lib.cm_masked_agg_backward_det_ws_bytes(100, 4, 64),
            "cm_linear_wgrad_det": lib.cm_linear_wgrad_det_ws_bytes(1000, 64, 32),
            "cm_ppo_surrogate_det": lib.cm_ppo_surrogate_det_ws_bytes(10, 15),
            "cm_gauss_nll_forward_det": lib.cm_gauss_nll_forward_det_ws_bytes(1000)}
    for name, call in _calls(C.c_void_p(4096), 0).items():
        assert need[name] > 0, name
        small = _calls(C.c_void_p(4096), need[name] - 1)[name]
        assert small(lib) == -1, name
        assert b"required" in lib.cm_last_error(), name


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def det_on(monkeypatch):
    import torch
    import com_marl_amd
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need the MI355X")
    com_marl_amd.set_deterministic(True)
    yield torch
    com_marl_amd.set_deterministic(None)


def _nan_slab(L, nb, dev):
    import torch
    return torch.full((max(1, (nb + 3) // 4),), float("nan"), dtype=torch.float32, device=dev)


def _twice(fn):
    """fn() -> tuple of tensors, run twice: bit-identical."""
    a = [t.cpu().numpy().copy() for t in fn()]
    b = [t.cpu().numpy().copy() for t in fn()]
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    return a


def _close64(got, ref, what, rel=2e-5):
    ref = ref.detach().double().cpu().numpy()
    scale = max(1e-6, float(np.abs(ref).max()))
    err = float(np.abs(got.astype(np.float64) - ref).max()) / scale
    assert err < rel, (what, err)


@pytest.mark.gpu
@pytest.mark.parametrize("R", [1000, 4099, 70001])
@pytest.mark.parametrize("K,O,layout,act", [(32, 32, 0, 1), (64, 64, 0, 1), (128, 64, 0, 0), (64, 128, 0, 1), (64, 64, 1, 0),
                                            (21, 128, 0, 1), (53, 64, 0, 1), (64, 5, 0, 0)])
def test_linear_backward_twin(R, K, O, layout, act, det_on):
    """cm_linear_act_backward_det (both the streaming kernel and the ragged-width one) against float64 torch; the slab starts as
    NaN, so a partial any workgroup failed to store shows up."""
    torch = det_on
    from com_marl_amd import _lib as L
    g = torch.Generator().manual_seed(R + K + O)
    x = torch.randn(R, K, generator=g).cuda()
    w = (torch.randn(O, K, generator=g) if layout == 0 else torch.randn(K, O, generator=g)).cuda() * 0.2
    y = torch.tanh(torch.randn(R, O, generator=g)).cuda() if act else None
    dy = torch.randn(R, O, generator=g).cuda()
    nb = L.lib().cm_linear_act_backward_det_ws_bytes(R, K, O)

    def run():
        dx = torch.empty(R, K, device="cuda") if K % 16 == 0 else None
        dw, db = torch.zeros_like(w), torch.zeros(O, device="cuda")
        L.check(L.lib().cm_linear_act_backward_det(R, K, O, L.ptr(x), L.ptr(w), layout, L.ptr(dy), None, L.ptr(y), L.ptr(dx), L.ptr(dw),
                                                   L.ptr(db), L.ptr(_nan_slab(L, nb, "cuda")), nb, L.current_stream()), "det")
        return (dw, db) + ((dx,) if dx is not None else ())
    got = _twice(run)
    dz = dy.double() * (1 - y.double() ** 2) if act else dy.double()
    wd = w.double() if layout == 0 else w.double().t()
    _close64(got[0], dz.t() @ x.double() if layout == 0 else x.double().t() @ dz, "dw")
    _close64(got[1], dz.sum(0), "db")
    if len(got) > 2:
        _close64(got[2], dz @ wd, "dx")


@pytest.mark.gpu
@pytest.mark.parametrize("R,d", [(999, 21), (65537, 29), (4096, 53)])
def test_encoder_backward_twin(R, d, det_on):
    torch = det_on
    from com_marl_amd import _lib as L
    g = torch.Generator().manual_seed(R + d)
    obs = torch.randn(R, d, generator=g).cuda()
    a1 = torch.tanh(torch.randn(R, 128, generator=g)).cuda()
    e = torch.tanh(torch.randn(R, 64, generator=g)).cuda()
    w2 = (torch.randn(64, 128, generator=g) * 0.1).cuda()
    dy, dy2 = torch.randn(R, 64, generator=g).cuda(), torch.randn(R, 64, generator=g).cuda()
    nb = L.lib().cm_encoder_backward_det_ws_bytes(R, d)

    def run():
        dw2, db2 = torch.zeros(64, 128, device="cuda"), torch.zeros(64, device="cuda")
        dw1, db1 = torch.zeros(128, d, device="cuda"), torch.zeros(128, device="cuda")
        rc = L.lib().cm_encoder_backward_det(R, d, L.ptr(obs), L.ptr(a1), L.ptr(e), L.ptr(w2), L.ptr(dy), L.ptr(dy2), L.ptr(dw2), L.ptr(db2),
                                             L.ptr(dw1), L.ptr(db1), L.ptr(_nan_slab(L, nb, "cuda")), nb, L.current_stream())
        if rc == 1:
            pytest.skip("shape not covered by the chained kernel")
        L.check(rc, "cm_encoder_backward_det")
        return dw2, db2, dw1, db1
    got = _twice(run)
    dz2 = (dy.double() + dy2.double()) * (1 - e.double() ** 2)
    dz1 = (dz2 @ w2.double()) * (1 - a1.double() ** 2)
    for v, r, n in zip(got, (dz2.t() @ a1.double(), dz2.sum(0), dz1.t() @ obs.double(), dz1.sum(0)), ("dw2", "db2", "dw1", "db1")):
        _close64(v, r, n)


@pytest.mark.gpu
@pytest.mark.parametrize("S,N", [(1001, 4), (37, 4), (77, 24), (9, 80), (3, 5)])
def test_masked_agg_backward_twin(S, N, det_on):
    """Teams of 4 (agg_bwd4), 24 and 80 (matrix cores) and 5 (first-generation kernel) against float64 autograd."""
    torch = det_on
    from com_marl_amd import _lib as L
    g = torch.Generator().manual_seed(S * N)
    attn = torch.softmax(torch.randn(S, N, N, generator=g), -1).cuda()
    adj = (torch.rand(S, N, N, generator=g) > 0.3).float().cuda()
    hw = torch.randn(S, N, 64, generator=g).cuda()
    bias = torch.randn(64, generator=g).cuda()
    A = attn.double() * adj.double()
    A = A / (A.sum(-1, keepdim=True) + 1e-12)
    out = torch.tanh(A @ hw.double() + bias.double()).float()
    d_out = torch.randn(S, N, 64, generator=g).cuda()
    nb = L.lib().cm_masked_agg_backward_det_ws_bytes(S, N, 64)

    def run():
        d_attn, d_hw, d_b = torch.empty_like(attn), torch.empty_like(hw), torch.zeros(64, device="cuda")
        L.check(L.lib().cm_masked_agg_backward_det(S, N, 64, L.ptr(attn), L.ptr(adj), None, 0, L.ptr(hw), L.ptr(out), None, L.ptr(d_out),
                                                   L.ptr(d_attn), L.ptr(d_hw), L.ptr(d_b), L.ptr(_nan_slab(L, nb, "cuda")), nb,
                                                   L.current_stream()), "cm_masked_agg_backward_det")
        return d_b, d_hw
    got = _twice(run)
    dp = d_out.double() * (1 - out.double() ** 2)
    _close64(got[0], dp.sum((0, 1)), "d_bias")
    _close64(got[1], A.transpose(1, 2) @ dp, "d_hw", rel=1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("R,P,Q", [(1000, 64, 53), (70001, 128, 64), (333, 5, 32)])
def test_wgrad_twin(R, P, Q, det_on):
    torch = det_on
    from com_marl_amd import _lib as L
    g = torch.Generator().manual_seed(R + P + Q)
    a, b = torch.randn(R, P, generator=g).cuda(), torch.randn(R, Q, generator=g).cuda()
    nb = L.lib().cm_linear_wgrad_det_ws_bytes(R, P, Q)

    def run():
        c, cs = torch.zeros(P, Q, device="cuda"), torch.zeros(P, device="cuda")
        L.check(L.lib().cm_linear_wgrad_det(R, P, Q, L.ptr(a), L.ptr(b), L.ptr(c), L.ptr(cs), L.ptr(_nan_slab(L, nb, "cuda")), nb,
                                            L.current_stream()), "cm_linear_wgrad_det")
        return c, cs
    got = _twice(run)
    _close64(got[0], a.double().t() @ b.double(), "c")
    _close64(got[1], a.double().sum(0), "colsum")


@pytest.mark.gpu
@pytest.mark.parametrize("P,T,N", [(7, 13, 4), (40, 200, 4), (5, 9, 24)])
def test_surrogate_and_gauss_nll_twins(P, T, N, det_on):
    """The f64 loss totals: block sums summed in a fixed order; equal to the atomic-merged default up to f64 rounding."""
    torch = det_on
    import com_marl_amd
    from com_marl_amd.algos import _SurrogateFn
    from com_marl_amd.nets import _GaussNLLFn
    g = torch.Generator().manual_seed(P * T)
    logits = torch.randn(P, T, N, 5, generator=g).cuda()
    actions = torch.randint(0, 5, (P, T, N), generator=g, dtype=torch.int32).cuda()
    old_ll = (torch.randn(P, T, generator=g) * 0.1 - 6).cuda()
    adv = torch.randn(P, T, generator=g).cuda()
    valids = torch.randint(1, T + 1, (P,), generator=g, dtype=torch.int32).cuda()
    S = P * T
    pa, ret = torch.randn(S, N, generator=g).cuda(), torch.randn(S, generator=g).cuda()
    ls = torch.tensor([-0.3], device="cuda")
    ws = torch.zeros(2, dtype=torch.float64, device="cuda")

    def run():
        tot, cnt = _SurrogateFn.apply(logits, actions, old_ll, adv, valids, 0.2, 0.1, 1)
        nll = _GaussNLLFn.apply(pa, ret, ls, None, ws)
        return tot, cnt, nll
    det = _twice(run)
    com_marl_amd.set_deterministic(False)
    ref = [t.cpu().numpy() for t in run()]
    np.testing.assert_allclose(det[0], ref[0], rtol=1e-6)
    assert det[1] == ref[1]
    np.testing.assert_allclose(det[2], ref[2], rtol=1e-6)


# ---- the reference's optimiser steps, in this mode -------------------------------------------------------------------------
@pytest.mark.gpu
def test_reference_steps_comm(det_on):
    from tests import test_hip_ppo_parity as T
    T.test_two_ppo_steps_match_reference(det_on)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["obsdp", "cent"])
def test_reference_steps_variants(kind, det_on):
    from tests import test_variants_parity as T
    T.test_two_ppo_steps_match_reference_variants(kind, det_on)


# ---- whole runs ------------------------------------------------------------------------------------------------------------
def _make(torch, case, seed=5):
    from com_marl_amd import envs as E, nets
    from com_marl_amd.algos import CentralizedMAPPO
    from com_marl_amd.sampler import CentralizedMAOnPolicyVectorizedSampler
    mpl = 15
    if case == "co24":
        B = 8
        params = dict(load=2, max_env_steps=mpl, capture_reward=2, step_cost=0, rm=0, penalty=1, revisit_penalty=0.5,
                      lazy_penalty=1, grid_size=20, Rsen=2, n_agents=24, n_preys=0, n_gcn_layers=2, mode="train",
                      trRcom=9, trpl=0.3, obstComplex="Easy", add_clock=0, seed=seed)
        env = E.CoverageWrapper(centralized=True, params=params, n_envs=B, device="cuda:0")
    elif case == "pp128":
        B, mpl = 6, 5
        params = dict(load=4, max_env_steps=mpl, capture_reward=10, step_cost=0.1, rm=0, penalty=0, grid_size=40, Rsen=2, n_agents=128,
                      n_preys=128, n_gcn_layers=2, mode="train", trRcom=9, trpl=0, seed=seed)
        env = E.PredatorPreyWrapper(centralized=True, params=params, n_envs=B, device="cuda:0")
    else:
        B = 64
        params = dict(load=2, max_env_steps=mpl, capture_reward=10, step_cost=0.1, rm=0, penalty=0, grid_size=10,
                      Rsen=1, n_agents=4, n_preys=4, n_gcn_layers=2, mode="train", trRcom=9, trpl=0, seed=seed)
        env = E.PredatorPreyWrapper(centralized=True, params=params, n_envs=B, device="cuda:0")
    torch.manual_seed(seed)
    N = env.n_agents
    if case == "obsdp":
        pol = nets.DecCategoricalMLPPolicy(env.spec, N, hidden_sizes=[128, 64, 32], device="cuda:0")
        crit = nets.CommBaseCritic(env.spec, n_agents=N, device="cuda:0")
    elif case == "cent":
        pol = nets.CentralizedCategoricalMLPPolicy(env.spec, n_agents=N, hidden_sizes=[128, 64, 32], device="cuda:0")
        crit = nets.GaussianMLPBaseline(env_spec=env.spec, hidden_sizes=(64, 64, 64), device="cuda:0")
    else:
        pol = nets.CommCategoricalMLPPolicy(env.spec, n_agents=N, device="cuda:0")
        crit = nets.CommBaseCritic(env.spec, n_agents=N, device="cuda:0")
    pol.set_rng(seed)
    ent = dict(entropy_method="max", center_adv=False, stop_entropy_gradient=True) if case == "max" else \
        dict(entropy_method="regularized", center_adv=True, stop_entropy_gradient=False)
    algo = CentralizedMAPPO(env_spec=env.spec, policy=pol, baseline=crit, max_path_length=mpl, discount=0.99, positive_adv=False,
                            gae_lambda=0.97, policy_ent_coeff=0.1, clip_grad_norm=7, optimization_n_minibatches=3,
                            optimization_mini_epochs=10, device="cuda:0", **ent)
    smp = CentralizedMAOnPolicyVectorizedSampler(algo, env, n_envs=B)
    smp.start_worker()
    return env, pol, crit, algo, smp, B * N * mpl


def _whole_run(torch, case, epochs=3):
    import com_marl_amd
    assert com_marl_amd.deterministic()
    env, pol, crit, algo, smp, batch = _make(torch, case)
    stats = []
    for itr in range(epochs):
        paths = smp.obtain_samples(itr, batch_size=batch)
        np.random.seed(100 + itr)
        algo.train_once(itr=itr, paths=paths)
        stats.append({k: v for k, v in algo.stats.items() if k not in _TIMING})
    env.batch.check_status()
    out = {"pol." + k: v.detach().cpu().numpy() for k, v in pol.state_dict().items()}
    out.update({"crit." + k: v.detach().cpu().numpy() for k, v in crit.state_dict().items()})
    for tag, opt in (("opt", algo._optimizer), ("bopt", algo._baseline_optimizer)):
        for i, st in opt.state_dict()["state"].items():
            for k, v in st.items():
                out[f"{tag}.{i}.{k}"] = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
    for e, st in enumerate(stats):
        for k, v in st.items():
            out[f"stats{e}.{k}"] = np.asarray(v)
    for i in range(min(8, len(paths))):                                # the trajectories of the last epoch
        for k in ("observations", "actions", "rewards"):
            v = paths[i][k]
            out[f"path{i}.{k}"] = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
    return out, algo


def _assert_identical(a, b):
    assert a.keys() == b.keys()
    bad = [k for k in a if not np.array_equal(a[k], b[k], equal_nan=True)]
    assert not bad, bad[:10]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["pp4", "co24", "obsdp", "cent", "max"])
def test_whole_runs_are_bit_identical(case, det_on, monkeypatch):
    """Two fresh runs of sampler + three train_once epochs: every parameter, both Adam moments and `step`, every stat and the last
    epoch's trajectories are equal bit for bit.  pp4 takes the wave-owned training forward (threshold lowered to the test's
    minibatch) and the teams-of-4 aggregation backward; co24 the matrix-core one."""
    torch = det_on
    if case == "pp4":
        monkeypatch.setenv("COMMARL_TRAIN_FWD_WAVE_MIN", "64")
    a, _ = _whole_run(torch, case)
    b, _ = _whole_run(torch, case)
    _assert_identical(a, b)


@pytest.mark.gpu
def test_whole_run_large_team_layer_by_layer(det_on):
    """PP map40 N=128 (the per-layer training path above 80 agents), one epoch."""
    a, _ = _whole_run(det_on, "pp128", epochs=1)
    b, _ = _whole_run(det_on, "pp128", epochs=1)
    _assert_identical(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("var,values", [("COMMARL_UPDATE_GRAPH", ("0", "1")), ("COMMARL_CRITIC_STREAM", ("0", "1"))])
def test_switches_are_bitwise_neutral(var, values, det_on, monkeypatch):
    """Graph replay against eager steps, and the critic on its own stream against one stream: no bit changes."""
    runs = []
    for v in values:
        monkeypatch.setenv(var, v)
        out, algo = _whole_run(det_on, "pp4")
        if var == "COMMARL_UPDATE_GRAPH" and v == "1":
            ug = algo._update_graphs
            assert ug is not None and ug.captured > 0 and not ug.broken
        runs.append(out)
    _assert_identical(*runs)


@pytest.mark.gpu
def test_switching_the_mode_captures_a_new_graph(det_on, monkeypatch):
    import com_marl_amd
    monkeypatch.setenv("COMMARL_UPDATE_GRAPH", "1")
    torch = det_on
    env, pol, crit, algo, smp, batch = _make(torch, "pp4")
    paths = smp.obtain_samples(0, batch_size=batch)
    np.random.seed(1)
    algo.train_once(itr=0, paths=paths)
    np.random.seed(1)
    algo.train_once(itr=1, paths=paths)                            # same shapes, same mode: replays
    ug = algo._update_graphs
    captured = ug.captured
    assert ug.reused > 0
    com_marl_amd.set_deterministic(False)
    np.random.seed(1)
    algo.train_once(itr=2, paths=paths)
    assert ug.captured > captured and not ug.broken
