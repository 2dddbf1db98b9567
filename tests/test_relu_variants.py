"""ReLU hidden layers of the Obs-DP and CENT policies (``hidden_nonlinearity=F.relu``, the reference runners'
``--hidden_nonlinearity relu``).

CPU part: the constructor switch and its refusals, the state_dict / pickle contract, the cm_mlp_weights field, and a
float64 restatement of both nets against the reference recordings of tools/gen_golden_relu.py (which shows the recordings
are ReLU nets, far from the tanh ones).
GPU part: the fused rollout forward, the autograd path and two PPO steps against those recordings; the ReLU forms of the
dense-layer kernels against float64 through the C ABI; bit-identical deterministic runs; end-to-end training and greedy eval."""
import ctypes as C
import os
import pickle
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from tests.test_oracle_golden import GOLDEN
from tests.test_variants_parity import _state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = [("variants_relu_pp_map10", 4), ("variants_relu_co_map20", 24), ("variants_relu_pp_map30", 72)]
TANH, RELU, NONE = 1, 2, 0


def _spec(d_total):
    from com_marl_amd.envs import EnvSpec, _Box, _Discrete
    return EnvSpec(_Box(np.zeros(d_total), np.ones(d_total)), _Discrete(5))


def _net(kind, N=4, d=21, **kw):
    from com_marl_amd import nets
    spec = _spec(N * d)
    if kind == "dec":
        return nets.DecCategoricalMLPPolicy(spec, N, hidden_sizes=[128, 64, 32], **kw)
    return nets.CentralizedCategoricalMLPPolicy(spec, n_agents=N, hidden_sizes=[128, 64, 32], **kw)


# ---- float64 restatement of the two reference nets ----------------------------------------------------------------------
def _mlp64(x, layers, acts):
    x = np.asarray(x, np.float64)
    for (w, b), a in zip(layers, acts):
        x = x @ np.asarray(w, np.float64).T + np.asarray(b, np.float64)
        if a == TANH:
            x = np.tanh(x)
        elif a == RELU:
            x = np.where(x < 0, 0.0, x)
    return x


def logits64(kind, sd, obs, N, act=RELU):
    """obs [..., N*d] -> logits [..., N, 5] of DecCategoricalMLPPolicy (encoder tanh, head hidden `act`) or
    CentralizedCategoricalMLPPolicy (every hidden layer `act`)."""
    def L(p):
        return sd[p + ".weight"], sd[p + ".bias"]
    obs = np.asarray(obs)
    if kind == "dec":
        x = obs.reshape(obs.shape[:-1] + (N, -1))
        return _mlp64(x, [L("encoder._layers.0.linear"), L("encoder._output_layers.0.linear"), L("_layers.0.linear"),
                          L("_output_layers.0.linear")], [TANH, TANH, act, NONE])
    lg = _mlp64(obs, [L("_layers.0.linear"), L("_layers.1.linear"), L("_layers.2.linear"), L("_output_layers.0.linear")],
                [act, act, act, NONE])
    return lg.reshape(obs.shape[:-1] + (N, -1))


def probs64(kind, sd, obs, avail, N, act=RELU):
    lg = logits64(kind, sd, obs, N, act)
    p = np.exp(lg - lg.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    if avail is not None:
        p = p * np.asarray(avail, np.float64).reshape(p.shape)
        p /= p.sum(-1, keepdims=True)
    return p


# ----------------------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------------------
SPELLINGS = [("torch.tanh", torch.tanh, TANH), ("F.tanh", F.tanh, TANH), ("nn.Tanh()", nn.Tanh(), TANH),
             ("torch.relu", torch.relu, RELU), ("F.relu", F.relu, RELU), ("nn.ReLU()", nn.ReLU(), RELU)]


@pytest.mark.parametrize("label,fn,code", SPELLINGS, ids=[s[0] for s in SPELLINGS])
def test_constructor_sets_the_per_layer_codes(label, fn, code):
    dec = _net("dec", hidden_nonlinearity=fn)
    assert [int(a) for _, a in dec._chain()] == [TANH, TANH, code, NONE]          # the encoder stays tanh
    cent = _net("cent", hidden_nonlinearity=fn)
    assert [int(a) for _, a in cent._chain()] == [code, code, code, NONE]


def test_default_is_tanh_and_unsupported_activations_raise():
    assert [int(a) for _, a in _net("dec")._chain()] == [TANH, TANH, TANH, NONE]
    assert [int(a) for _, a in _net("cent")._chain()] == [TANH, TANH, TANH, NONE]
    for bad in (torch.sigmoid, nn.ELU()):
        for kind in ("dec", "cent"):
            with pytest.raises(NotImplementedError, match="relu"):
                _net(kind, hidden_nonlinearity=bad)
    with pytest.raises(TypeError):                                                 # no catch-all keyword any more
        _net("dec", hidden_nonlinearity_typo=F.relu)


@pytest.mark.parametrize("kind", ["dec", "cent"])
def test_state_dict_and_pickle(kind):
    t, r = _net(kind), _net(kind, hidden_nonlinearity=F.relu)
    assert [(k, tuple(v.shape)) for k, v in t.state_dict().items()] == [(k, tuple(v.shape)) for k, v in r.state_dict().items()]
    r.load_state_dict(t.state_dict())                                             # checkpoints load both ways
    t.load_state_dict(r.state_dict())
    back = pickle.loads(pickle.dumps(r))
    assert back.hidden_nonlinearity == "relu" and [int(a) for _, a in back._chain()] == [int(a) for _, a in r._chain()]


def test_mlp_weights_relu_mask_field():
    from com_marl_amd import _lib as L
    src = open(os.path.join(ROOT, "include", "commarl.h")).read()
    body = re.search(r"typedef struct cm_mlp_weights \{(.*?)\} cm_mlp_weights;", src, re.S).group(1)
    assert re.search(r"int32_t tanh_mask, relu_mask;", body)
    # in_dim, n_layers, out_dim[6], tanh_mask, then relu_mask: byte 36; the struct size is unchanged
    assert L.MlpWeights.relu_mask.offset == 4 * (2 + L.MLP_MAX_LAYERS + 1) == 36
    assert C.sizeof(L.MlpWeights) == 2 * 4 + 6 * 4 + 2 * 4 + 13 * 8
    w = _net("cent", hidden_nonlinearity=F.relu)._struct_from({f"{p}{i}{s}": 0 for i in range(4) for p, s in (("w", "t"), ("b", ""))})
    assert (w.tanh_mask, w.relu_mask) == (0, 0b0111)
    w = _net("dec", hidden_nonlinearity=F.relu)._struct_from({f"{p}{i}{s}": 0 for i in range(4) for p, s in (("w", "t"), ("b", ""))})
    assert (w.tanh_mask, w.relu_mask) == (0b0011, 0b0100)


@pytest.mark.parametrize("name,N", FIX)
def test_f64_restatement_reproduces_relu_recordings(name, N):
    """The recordings are ReLU nets: the float64 restatement reproduces them, and the tanh one is far off."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    obs = z["obs"]
    for tag in ("dec", "cent"):
        sd = _state_dict(z, tag)
        for suffix, av in (("", None), ("_masked", z["avail_masked"])):
            p = probs64(tag, sd, obs, av, N)
            np.testing.assert_allclose(p, z[f"{tag}.probs{suffix}"], rtol=1e-5, atol=1e-6, err_msg=f"{tag}{suffix}")
            gap = float(np.abs(probs64(tag, sd, obs, av, N, act=TANH) - z[f"{tag}.probs{suffix}"]).max())
            assert gap > 1e-2, (tag, suffix, gap)                                 # >> the GPU tests' 1e-5
        p = probs64(tag, sd, obs, z["avail_masked"], N)
        s = np.sort(p, -1)
        ok = s[..., -1] - s[..., -2] > 1e-6
        np.testing.assert_array_equal(p.argmax(-1)[ok], z[f"{tag}.greedy_masked"][ok])
        p = probs64(tag, sd, obs, None, N)
        np.testing.assert_allclose(-(p * np.log(p)).sum(-1).mean(-1), z[f"{tag}.entropy"], rtol=1e-5, atol=1e-6)
        ll = np.log(np.take_along_axis(p, z["actions"][..., None], -1))[..., 0].sum(-1)
        np.testing.assert_allclose(ll, z[f"{tag}.loglik"], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("kind", ["obsdp", "cent"])
def test_f64_restatement_reproduces_relu_ppo_steps(kind):
    """ppo_step_<kind>_relu.npz: at the first step the ratio is 1 and the centred advantages average to 0, so the reference's
    loss is -0.1 x the valid steps' mean policy entropy, which the float64 ReLU restatement reproduces from pol0 and obs."""
    z = np.load(os.path.join(GOLDEN, f"ppo_step_{kind}_relu.npz"))
    sd = {k[5:]: z[k] for k in z.files if k.startswith("pol0.")}
    obs = z["obs"]
    P, T = obs.shape[:2]
    valid = np.arange(T)[None, :] < np.asarray(z["valids"])[:, None]
    tag = "dec" if kind == "obsdp" else "cent"
    ents = {}
    for act in (RELU, TANH):
        p = probs64(tag, sd, obs, None, 4, act=act)
        ents[act] = -0.1 * float((-(p * np.log(p)).sum(-1).mean(-1))[valid].mean())
    np.testing.assert_allclose(ents[RELU], float(z["loss1"]), rtol=1e-6)
    assert abs(ents[TANH] - float(z["loss1"])) > 1e-3


# ----------------------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def torch_cuda():
    from oracle import oracle as O
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need the MI355X")
    O.build()
    return torch


@pytest.fixture
def relu_nets(monkeypatch):
    """The two policy classes of com_marl_amd.nets with F.relu as the default hidden nonlinearity (as the reference
    runners build them), so that the tanh parity tests of tests/test_variants_parity.py run unchanged on ReLU nets."""
    from com_marl_amd import nets
    for name in ("DecCategoricalMLPPolicy", "CentralizedCategoricalMLPPolicy"):
        base = getattr(nets, name)

        def init(self, *a, _base=base, **k):
            k.setdefault("hidden_nonlinearity", F.relu)
            _base.__init__(self, *a, **k)
        monkeypatch.setattr(nets, name, type(name, (base,), {"__init__": init}))
    return nets


@pytest.mark.gpu
@pytest.mark.parametrize("name,N", FIX)
def test_hip_relu_forward_matches_reference(name, N, torch_cuda, relu_nets):
    """cm_mlp_policy_forward with relu_mask: probabilities (1e-5), greedy actions, and the Philox samples on the kernel's own
    probabilities, for both policies at N = 4, 24, 72."""
    from tests import test_variants_parity as T
    T.test_hip_row_mlp_forward_matches_reference_and_oracle(name, N, torch_cuda)
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    for tag in ("dec", "cent"):
        assert [int(a) for _, a in T._make(torch, z, tag, N, z["obs"].shape[1])._chain()][-2] == RELU


@pytest.mark.gpu
@pytest.mark.parametrize("name,N", FIX)
def test_hip_relu_autograd_matches_reference(name, N, torch_cuda, relu_nets):
    from tests import test_variants_parity as T
    T.test_variant_autograd_matches_reference(name, N, torch_cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["obsdp", "cent"])
@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
def test_two_relu_ppo_steps_match_reference(kind, det, torch_cuda, relu_nets, monkeypatch, tmp_path):
    """Two optimiser steps of the reference's CentralizedMAPPO with ReLU nets (ppo_step_<kind>_relu.npz), in both update modes."""
    import com_marl_amd
    from tests import test_variants_parity as T
    os.symlink(os.path.join(GOLDEN, f"ppo_step_{kind}_relu.npz"), tmp_path / f"ppo_step_{kind}.npz")
    monkeypatch.setattr(T, "GOLDEN", str(tmp_path))
    com_marl_amd.set_deterministic(det)
    try:
        T.test_two_ppo_steps_match_reference_variants(kind, torch_cuda)
    finally:
        com_marl_amd.set_deterministic(None)


# ---- the dense-layer kernels through the C ABI, against float64 --------------------------------------------------------------
# (K, O, layout, dx): lin2 streaming 64 -> 32 and 128 -> 64; the ragged lin2 first layer 84 -> 128 (no dx); lin::bwd_kernel at
# widths it alone serves, and for the [in,out] layout
ABI_SHAPES = [(64, 32, 0, True), (128, 64, 0, True), (84, 128, 0, False), (48, 40, 0, True), (100, 20, 0, True),
              (48, 40, 1, True), (64, 64, 1, True), (64, 32, 0, False)]
TOL = 2e-5
_WORST = {}


def _ratio(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max()) / max(1e-12, float(np.abs(ref).max())) / TOL


@pytest.mark.gpu
@pytest.mark.parametrize("R", [1000, 100003])
@pytest.mark.parametrize("K,O,layout,want_dx", ABI_SHAPES)
@pytest.mark.parametrize("dy2", [False, True], ids=["dy", "dy+dy2"])
@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
def test_relu_linear_kernels_against_f64(R, K, O, layout, want_dx, dy2, det, torch_cuda):
    """cm_linear_act_forward(act=2) then cm_linear_act_backward_ex(_det)(act=2) against float64.  Where the pre-activation is
    within 1e-6 of its own magnitude scale (|b| + sum|x w|) of 0, float32 and float64 may disagree on its sign: those
    elements take the kernel's own mask in the reference; they are counted and must be a tiny fraction."""
    from com_marl_amd import _lib as L
    lib = L.lib()
    g = torch.Generator().manual_seed(R + 7 * K + O + layout)
    x = torch.randn(R, K, generator=g)
    w = (torch.randn(O, K, generator=g) if layout == 0 else torch.randn(K, O, generator=g)) * 0.2
    b = torch.randn(O, generator=g) * 0.3
    dy = torch.randn(R, O, generator=g)
    d2 = torch.randn(R, O, generator=g) if dy2 else None
    xc, wc, bc, dyc = x.cuda(), w.cuda(), b.cuda(), dy.cuda()
    d2c = d2.cuda() if dy2 else None
    y = torch.empty(R, O, device="cuda")
    L.check(lib.cm_linear_act_forward(R, K, O, L.ptr(xc), L.ptr(wc), layout, L.ptr(bc), 2, L.ptr(y), L.current_stream()), "fwd")
    dx = torch.empty(R, K, device="cuda") if want_dx else None
    dw, db = torch.zeros_like(wc), torch.zeros(O, device="cuda")
    if det:
        nb = lib.cm_linear_act_backward_det_ws_bytes(R, K, O)
        ws = torch.full((max(1, (nb + 3) // 4),), float("nan"), device="cuda")
        L.check(lib.cm_linear_act_backward_ex_det(R, K, O, L.ptr(xc), L.ptr(wc), layout, L.ptr(dyc), L.ptr(d2c), L.ptr(y), 2, L.ptr(dx),
                                                  L.ptr(dw), L.ptr(db), L.ptr(ws), nb, L.current_stream()), "bwd det")
    else:
        L.check(lib.cm_linear_act_backward_ex(R, K, O, L.ptr(xc), L.ptr(wc), layout, L.ptr(dyc), L.ptr(d2c), L.ptr(y), 2, L.ptr(dx),
                                              L.ptr(dw), L.ptr(db), L.current_stream()), "bwd")
    torch.cuda.synchronize()
    x64, b64 = x.double(), b.double()
    w64 = w.double() if layout == 0 else w.double().t()                          # [O, K]
    z64 = x64 @ w64.t() + b64
    scale = x64.abs() @ w64.abs().t() + b64.abs()
    kink = (z64.abs() <= 1e-6 * scale).numpy()
    yk = y.cpu().numpy()
    mask = np.where(kink, yk > 0, (z64 > 0).numpy())
    n_kink = int(kink.sum())
    assert n_kink <= 1e-4 * R * O, n_kink
    g64 = (dy.double() + (d2.double() if dy2 else 0.0)).numpy()
    dz = np.where(mask, g64, 0.0)
    refs = dict(y=np.where(z64.numpy() < 0, 0.0, z64.numpy()), db=dz.sum(0))
    dw_ref = dz.T @ x64.numpy()                                                   # [O, K]
    refs["dw"] = dw_ref if layout == 0 else dw_ref.T
    if want_dx:
        refs["dx"] = dz @ w64.numpy()
    got = dict(y=yk, dw=dw.cpu().numpy(), db=db.cpu().numpy(), dx=None if dx is None else dx.cpu().numpy())
    ratios = {k: _ratio(got[k], v) for k, v in refs.items()}
    key = f"K{K} O{O} layout{layout}{' dx' if want_dx else ''}"
    _WORST[key] = max(_WORST.get(key, 0.0), *ratios.values())
    print(f"[relu abi] R={R} {key} dy2={dy2} det={det}: worst ratio {max(ratios.values()):.3f} {ratios} kinks {n_kink}")
    assert max(ratios.values()) < 1.0, ratios
    # negative control: the tanh derivative applied to the ReLU outputs fails the same metric
    bad = g64 * (1.0 - yk.astype(np.float64) ** 2)
    assert _ratio(got["db"], bad.sum(0)) > 10.0


@pytest.mark.gpu
def test_relu_abi_refusals(torch_cuda):
    from com_marl_amd import _lib as L
    lib = L.lib()
    R, K, O = 64, 32, 32
    x, w, y = (torch.zeros(R, K, device="cuda"), torch.zeros(O, K, device="cuda"), torch.zeros(R, O, device="cuda"))
    dy, dw = torch.zeros(R, O, device="cuda"), torch.zeros(O, K, device="cuda")
    s = L.current_stream()
    assert lib.cm_linear_act_forward(R, K, O, L.ptr(x), L.ptr(w), 0, None, 3, L.ptr(y), s) == -1
    assert b"act" in lib.cm_last_error()
    assert lib.cm_linear_act_backward_ex(R, K, O, L.ptr(x), L.ptr(w), 0, L.ptr(dy), None, L.ptr(y), 3, None, L.ptr(dw), None, s) == -1
    assert lib.cm_linear_act_backward_ex(R, K, O, L.ptr(x), L.ptr(w), 0, L.ptr(dy), None, None, 2, None, L.ptr(dw), None, s) == -1
    nb = lib.cm_linear_act_backward_det_ws_bytes(R, K, O)
    ws = torch.zeros((nb + 3) // 4, device="cuda")
    assert lib.cm_linear_act_backward_ex_det(R, K, O, L.ptr(x), L.ptr(w), 0, L.ptr(dy), None, L.ptr(y), 3, None, L.ptr(dw), None,
                                             L.ptr(ws), nb, s) == -1
    assert lib.cm_linear_act_backward_ex_det(R, K, O, L.ptr(x), L.ptr(w), 0, L.ptr(dy), None, L.ptr(y), 2, None, L.ptr(dw), None,
                                             None, 0, s) == -1
    assert lib.cm_linear_act_backward_ex_det(R, K, O, L.ptr(x), L.ptr(w), 0, L.ptr(dy), None, L.ptr(y), 2, None, L.ptr(dw), None,
                                             L.ptr(ws), nb - 4, s) == -1
    torch.cuda.synchronize()
    # both mask bits on one layer
    wt = torch.zeros(8, 10, device="cuda")
    mw = L.MlpWeights()
    mw.in_dim, mw.n_layers = 8, 1
    mw.out_dim[0] = 10
    mw.wt[0] = wt.data_ptr()
    mw.tanh_mask, mw.relu_mask = 1, 1
    obs, probs = torch.zeros(4, 8, device="cuda"), torch.zeros(4, 2, 5, device="cuda")
    assert lib.cm_mlp_policy_forward(C.byref(mw), 4, 2, 5, 2, obs.data_ptr(), None, 1, 0, 0, None, 0, None, probs.data_ptr(), None) == -1
    assert b"relu_mask" in lib.cm_last_error()
    mw.tanh_mask = 0
    assert lib.cm_mlp_policy_forward(C.byref(mw), 4, 2, 5, 2, obs.data_ptr(), None, 1, 0, 0, None, 0, None, probs.data_ptr(), None) == 0
    torch.cuda.synchronize()


# ---- whole runs --------------------------------------------------------------------------------------------------------------
def _run_setup(kind, case, act=F.relu, seed=5, B=None, mpl=10):
    from com_marl_amd import envs as E, nets
    from com_marl_amd.algos import CentralizedMAPPO
    from com_marl_amd.sampler import CentralizedMAOnPolicyVectorizedSampler
    if case == "co24":
        params = dict(load=2, max_env_steps=mpl, capture_reward=2, step_cost=0, rm=0, penalty=1, revisit_penalty=0.5,
                      lazy_penalty=1, grid_size=20, Rsen=2, n_agents=24, n_preys=0, n_gcn_layers=2, mode="train",
                      trRcom=9, trpl=0.3, obstComplex="Easy", add_clock=0, seed=seed)
        env = E.CoverageWrapper(centralized=True, params=params, n_envs=B or 8, device="cuda:0")
    else:
        params = dict(load=2, max_env_steps=mpl, capture_reward=10, step_cost=0.1, rm=0, penalty=0, grid_size=10,
                      Rsen=1, n_agents=4, n_preys=4, n_gcn_layers=2, mode="train", trRcom=9, trpl=0, seed=seed)
        env = E.PredatorPreyWrapper(centralized=True, params=params, n_envs=B or 64, device="cuda:0")
    torch.manual_seed(seed)
    N = env.n_agents
    if kind == "obsdp":
        pol = nets.DecCategoricalMLPPolicy(env.spec, N, hidden_sizes=[128, 64, 32], hidden_nonlinearity=act, device="cuda:0")
        crit = nets.CommBaseCritic(env.spec, n_agents=N, device="cuda:0")
    else:
        pol = nets.CentralizedCategoricalMLPPolicy(env.spec, n_agents=N, hidden_sizes=[128, 64, 32], hidden_nonlinearity=act,
                                                   device="cuda:0")
        crit = nets.GaussianMLPBaseline(env_spec=env.spec, hidden_sizes=(64, 64, 64), device="cuda:0")
    pol.set_rng(seed)
    algo = CentralizedMAPPO(env_spec=env.spec, policy=pol, baseline=crit, max_path_length=mpl, discount=0.99, positive_adv=False,
                            center_adv=True, gae_lambda=0.97, policy_ent_coeff=0.1, entropy_method="regularized",
                            stop_entropy_gradient=False, clip_grad_norm=7, optimization_n_minibatches=3,
                            optimization_mini_epochs=10, device="cuda:0")
    smp = CentralizedMAOnPolicyVectorizedSampler(algo, env, n_envs=env.batch.B)
    smp.start_worker()
    return env, pol, crit, algo, smp, env.batch.B * N * mpl


def _epochs(kind, case, epochs, **kw):
    env, pol, crit, algo, smp, batch = _run_setup(kind, case, **kw)
    stats = []
    for itr in range(epochs):
        paths = smp.obtain_samples(itr, batch_size=batch)
        np.random.seed(100 + itr)
        algo.train_once(itr=itr, paths=paths)
        stats.append({k: v for k, v in algo.stats.items() if k not in ("EpochTime", "TrainOnceTime", "GPUMemoryMax")})
    env.batch.check_status()
    return env, pol, crit, algo, stats, paths


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["obsdp", "cent"])
def test_relu_whole_runs_are_bit_identical(kind, torch_cuda):
    import com_marl_amd
    com_marl_amd.set_deterministic(True)
    try:
        outs = []
        for _ in range(2):
            env, pol, crit, algo, stats, paths = _epochs(kind, "pp4", 3)
            out = {"pol." + k: v.detach().cpu().numpy() for k, v in pol.state_dict().items()}
            out.update({"crit." + k: v.detach().cpu().numpy() for k, v in crit.state_dict().items()})
            for e, st in enumerate(stats):
                out.update({f"stats{e}.{k}": np.asarray(v) for k, v in st.items()})
            for i in range(min(8, len(paths))):
                for k in ("observations", "actions", "rewards"):
                    v = paths[i][k]
                    out[f"path{i}.{k}"] = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
            outs.append(out)
        a, b = outs
        assert a.keys() == b.keys()
        bad = [k for k in a if not np.array_equal(a[k], b[k], equal_nan=True)]
        assert not bad, bad[:10]
    finally:
        com_marl_amd.set_deterministic(None)


@pytest.mark.gpu
@pytest.mark.parametrize("case,B", [("pp4", 4096), ("co24", 64)])
@pytest.mark.parametrize("kind", ["obsdp", "cent"])
def test_relu_end_to_end_train_and_greedy_eval(kind, case, B, torch_cuda, monkeypatch):
    """Sampler + train_once, then eval_model(eval_greedy=True); a greedy RolloutEngine span (the path eval_model takes) picks the
    float64 ReLU restatement's argmax on the recorded observations; a tanh run from the same seeds has other losses."""
    from com_marl_amd import evaluate
    from com_marl_amd.rollout import RolloutEngine
    monkeypatch.setenv("COMMARL_UPDATE_GRAPH", "1")
    mpl = 10
    env, pol, crit, algo, stats, _ = _epochs(kind, case, 1, B=B, mpl=mpl)
    for k in ("LossBefore", "LossAfter", "KL", "Entropy"):
        assert np.isfinite(stats[0][k]), (k, stats[0][k])
    data, succ, rews, bound = evaluate.eval_model(env, pol, 0, n_eval_episodes=20, max_env_steps=mpl, eval_greedy=True)
    assert len(data) == 20 and all(np.isfinite(r) for r in rews["reward"])
    # the greedy span eval_model runs, checked against float64
    base = getattr(env, "env", env)
    pol.sync_weights()
    eng = RolloutEngine(base.batch, pol, mpl, store_attn=False, store_probs=False)
    evaluate._first_episodes(eng, base, mpl, True)
    N = base.batch.N
    sd = {k: v.detach().double().cpu().numpy() for k, v in pol.state_dict().items()}
    obs = eng.obs[:mpl].cpu().numpy().reshape(mpl, B, -1)
    acts = eng.actions[:mpl].cpu().numpy()
    p = probs64("dec" if kind == "obsdp" else "cent", sd, obs, None, N)
    s = np.sort(p, -1)
    ok = s[..., -1] - s[..., -2] > 1e-6
    n_tie = int((~ok).sum())
    print(f"[relu e2e] {kind} {case}: {acts.size} greedy actions, {n_tie} near-ties excluded")
    assert n_tie < 1e-3 * acts.size
    np.testing.assert_array_equal(acts[ok], p.argmax(-1)[ok])
    # the switch reaches the training path: same seeds, tanh nets, other first-epoch losses
    _, _, _, _, stats_t, _ = _epochs(kind, case, 1, B=B, mpl=mpl, act=torch.tanh)
    assert abs(stats_t[0]["LossBefore"] - stats[0]["LossBefore"]) > 1e-4 * max(1.0, abs(stats[0]["LossBefore"]))
