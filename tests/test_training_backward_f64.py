"""The whole training path of the Comm-DP nets - forward, loss and backward through whatever kernels a shape reaches -
against the float64 restatement (tests/f64_commnet.py, pinned to the reference by tests/test_f64_commnet.py):

  * CASES: curated shapes, each naming the path it covers and ASSERTING it - the C entry points that ran (and the
    bias_replicas they got) are recorded by a proxy around com_marl_amd._lib.lib(), not inferred from the shape;
  * test_net_grads_fixture: the reference's own recordings of the default net at N = 24 .. 128 (tests/golden/net_grads_*.npz).

pol._logits -> the PPO-shaped scalar of oracle/gen_golden.py::record_net_options on the avail-masked probabilities, and
crit._values_grad -> the Gaussian NLL, each backward to every parameter.  Tolerance: max|got - ref64| <= 1e-5 * max|ref64|
for logits, probabilities, values, the two scalars and every gradient; logits are also held per agent row.  The float64
reference runs in torch float64 on the GPU (no code shared with the kernels)."""
import time

import numpy as np
import pytest
import torch

from tests import f64_commnet as R
from tests.lib_spy import spy  # noqa: F401  (the fixture: a recording proxy around _lib.lib())

pytestmark = pytest.mark.gpu

TAU = 1e-5
DEV = "cuda:0"
F64 = torch.float64


# path -> (entry points that must run, entry points that must not)
FUSED_BWD = {"cm_masked_agg_backward_r", "cm_attention_backward", "cm_encoder_backward"}
PATHS = {
    "fused": ({"cm_policy_forward_saved", "cm_critic_forward_saved"} | FUSED_BWD,
              {"cm_masked_agg_forward", "cm_attention_forward", "cm_policy_forward_saved_wave"}),
    "wave": ({"cm_policy_forward_saved_wave"} | FUSED_BWD, {"cm_masked_agg_forward"}),
    "layers": ({"cm_attention_forward", "cm_masked_agg_forward", "cm_masked_agg_backward", "cm_attention_backward",
                "cm_linear_act_forward", "cm_linear_act_backward"},
               {"cm_policy_forward_saved", "cm_critic_forward_saved", "cm_masked_agg_backward_r"}),
    "torch": ({"cm_linear_act_backward"}, {"cm_attention_forward", "cm_attention_backward", "cm_masked_agg_forward",
                                           "cm_masked_agg_backward", "cm_masked_agg_backward_r", "cm_policy_forward_saved"}),
}
DET_NAMES = {"cm_masked_agg_backward_r": "cm_masked_agg_backward_det", "cm_masked_agg_backward": "cm_masked_agg_backward_det",
             "cm_encoder_backward": "cm_encoder_backward_det", "cm_linear_act_backward": "cm_linear_act_backward_det"}

# name: (N, S, d, hops, residual, attention, aggregator, masks, path, bias_replicas | None, note)
CASES = {
    "n4_s300": (4, 300, 21, 2, True, "general", "sum", "present", "fused", 1, "teams of 4, quad backward kernels"),
    "n4_s70001_wave": (4, 70001, 21, 2, True, "general", "sum", "present", "wave", 32,
                       "wave-owned forward (S >= 16384), 32 bias replicas (S > 8192), agg_bwd4 and attn_bwd4 both looping"),
    "n3": (3, 64, 21, 2, True, "general", "sum", "masked_row", "fused", 1, "first-generation N x N kernels, a fully masked row"),
    "n8": (8, 50, 30, 2, True, "general", "sum", "present", "fused", 1, "matrix core MAXNT 2"),
    "n24": (24, 20, 77, 2, True, "general", "sum", "present", "fused", 1, "matrix core MAXNT 2, config 3 team size"),
    "n54": (54, 8, 77, 2, True, "general", "sum", "masked_row", "fused", 1, "matrix core MAXNT 5, config 5, masked row"),
    "n72": (72, 6, 53, 2, True, "general", "sum", "present", "fused", 1, "matrix core MAXNT 5, config 4"),
    "n72_d84": (72, 6, 84, 2, True, "general", "sum", "present", "layers", None,
                "d > 80: no matrix-core pack, hence no saved forward (MAX_FUSED_OBS): per-layer path"),
    "n80": (80, 5, 40, 2, True, "general", "sum", "present", "fused", 1, "largest fused team (MAX_FUSED_AGENTS)"),
    "n96_layers": (96, 4, 77, 2, True, "general", "sum", "present", "layers", None, "per-layer path, MAXNT 8"),
    "n128_layers": (128, 3, 84, 2, True, "general", "sum", "masked_row", "layers", None, "per-layer path at MAX_KERNEL_AGENTS"),
    "n130_torch": (130, 2, 21, 2, True, "general", "sum", "present", "torch", None, "above MAX_KERNEL_AGENTS: framework GEMMs"),
    "hops1": (24, 12, 40, 1, True, "general", "sum", "present", "fused", 1, "one hop"),
    "hops3_nores": (24, 12, 40, 3, False, "general", "sum", "present", "fused", 1, "three hops, no residual"),
    "hops4": (8, 40, 40, 4, True, "general", "sum", "present", "fused", 1, "four hops (the fused maximum)"),
    "hops0": (8, 40, 40, 0, True, "general", "sum", "present", "layers0", None, "no hop: per-layer, x = 2E"),
    "hops5": (8, 20, 40, 5, True, "general", "sum", "present", "layers", None, "five hops: per-layer"),
    "dot": (24, 12, 40, 2, True, "dot", "sum", "present", "fused", 1, "'dot' attention"),
    "direct": (24, 12, 40, 2, True, "general", "direct", "present", "fused+direct", None, "critic 'direct' aggregator"),
    "d77": (4, 300, 77, 2, True, "general", "sum", "present", "fused", 1, "d > 64: two-layer encoder fallback"),
    "d80": (8, 40, 80, 2, True, "general", "sum", "present", "fused", 1, "d = 80, the largest fused: two-layer encoder fallback"),
    "d96": (4, 300, 96, 2, True, "general", "sum", "none", "layers", None, "d = 96, no masks: per-layer path (MAX_FUSED_OBS)"),
    "nomask": (4, 300, 21, 1, False, "general", "sum", "none", "fused", 1, "masks None"),
}
DET_CASES = ["n4_s300", "n4_s70001_wave", "n24", "n72", "n72_d84", "n96_layers", "d77", "d80", "hops3_nores"]


def _inputs(N, S, d, hops, masks, seed):
    g = torch.Generator().manual_seed(seed)
    obs = (torch.rand(S, N * d, generator=g) < 0.3).float() + 0.05 * torch.randn(S, N * d, generator=g)
    adj = ch = avail = None
    if masks != "none":
        adj = (torch.rand(S, N, N, generator=g) < 0.7).float()
        adj[:, torch.arange(N), torch.arange(N)] = 1.0
        if hops:
            ch = (torch.rand(S, hops, N, N, generator=g) < 0.8).float()
            ch[:, :, torch.arange(N), torch.arange(N)] = 1.0
        avail = torch.ones(S, N, 5)
        avail[torch.rand(S, N, generator=g) < 0.3, 1] = 0.0
        if masks == "masked_row":
            adj[0, 0, :] = 0.0
    acts = torch.randint(0, 5, (S, N), generator=g)
    wts = torch.randn(S, generator=g)
    rets = torch.randn(S, generator=g) * 3
    cuda = lambda t: None if t is None else t.to(DEV).contiguous()           # noqa: E731
    return tuple(map(cuda, (obs, adj, ch, avail, acts, wts, rets)))


def _nets(N, d, hops, residual, att, agg, seed):
    from com_marl_amd import envs as E, nets
    spec = E.EnvSpec(E._Box(np.zeros(d * N), np.ones(d * N)), E._Discrete(5))
    torch.manual_seed(seed)
    pol = nets.CommCategoricalMLPPolicy(spec, n_agents=N, n_gcn_layers=hops, residual=residual, attention_type=att, device=DEV)
    crit = nets.CommBaseCritic(spec, n_agents=N, n_gcn_layers=hops, residual=residual, attention_type=att, aggregator_type=agg,
                               device=DEV)
    with torch.no_grad():
        for net in (pol, crit):
            for name, p in net.named_parameters():
                if name.endswith("bias") and "gcn" not in name:
                    p.uniform_(-0.1, 0.1)
    return pol, crit


CRIT_OUT_BIAS = "gcrit.baseline_aggregator._mean_module._output_layers.0.linear.bias"


def _out_bias_terms(values, std, rets, mult):
    """The critic's last bias gradient is ONE sum, mult * sum_s dNLL/dv_s = mult * sum_s (v_s - r_s) / (S std^2), whose terms
    have random signs: at a few envs it cancels to far below them, and the float32 values it is formed from (each a sum over the
    team's agents) carry ~1e-7 of their own size.  Measured STRICT ratios of that one tensor: 0.9e-5 .. 1.01e-5 (N = 24, 96) -
    rounding of the values, not a kernel error.  Its applied scale is the root-sum-square of the terms (independent roundings
    of S values add as such): max(|ref|, mult * sqrt(sum_s ((v_s - r_s) / (S std^2))^2))."""
    v, r, sd = (torch.as_tensor(np.asarray(t.detach().cpu()) if torch.is_tensor(t) else np.asarray(t)).to(F64)
                for t in (values, rets, std))
    return float(mult * (((v - r) / (v.numel() * sd.reshape(-1)[0] ** 2)) ** 2).sum().sqrt())


def _as64(t):
    return torch.as_tensor(np.asarray(t.detach().cpu()) if torch.is_tensor(t) else np.asarray(t)).to(F64)


def _check(case, name, got, ref, worst, rows=None, terms=None):
    """worst[name] = (strict, applied): strict = max|got - ref| / max|ref| (and per row with `rows`); applied = the same with
    the tensor scale max(max|ref|, terms) where `terms` is given (the critic's last bias only, see _out_bias_terms)."""
    g, r = _as64(got), _as64(ref)
    err, scale = float((g - r).abs().max()), max(float(r.abs().max()), 1e-6)
    strict = err / scale
    if rows is not None:
        strict = max(strict, R.row_ratio(got, ref, rows))
    applied = strict if terms is None else max(err / max(scale, terms), R.row_ratio(got, ref, rows) if rows is not None else 0.0)
    worst[name] = (strict, applied)
    assert applied <= TAU, f"{case}: {name} off by {applied:.3g} of its scale (strict {strict:.3g}; tolerance {TAU})"


def _summary(worst):
    ks = max(worst, key=lambda k: worst[k][0])
    ka = max(worst, key=lambda k: worst[k][1])
    return f"worst strict ratio {worst[ks][0]:.2e} ({ks}); worst applied {worst[ka][1]:.2e} ({ka})"


def _run_and_compare(case, pol, crit, N, residual, obs, adj, ch, avail, acts, wts, rets):
    """-> {tensor: ratio}; asserts every ratio <= TAU."""
    worst = {}
    # HIP training path
    logits = pol._logits(obs, adj, ch)
    probs = R.masked_probs(logits, avail)
    scalar = R.ppo_scalar(probs, acts, wts)
    pol.zero_grad()
    scalar.backward()
    values, std = crit._values_grad(obs, adj, ch)
    loss = R.critic_nll(values, std, rets)
    crit.zero_grad()
    loss.backward()
    torch.cuda.synchronize()
    # float64 restatement
    p64 = R.params(pol.state_dict(), device=DEV)
    c64 = R.params(crit.state_dict(), device=DEV)
    w = lambda t: None if t is None else t.to(F64)                            # noqa: E731
    lg64, pr64, _ = R.policy_forward(p64, w(obs), w(avail), w(adj), w(ch), N, residual)
    sc64 = R.ppo_scalar(pr64, acts, w(wts))
    sc64.backward()
    v64 = R.critic_values(c64, w(obs), w(adj), w(ch), N, residual, crit.aggregator_type)
    l64 = R.critic_nll(v64, R.critic_std(c64), w(rets))
    l64.backward()
    S = obs.shape[0]
    _check(case, "logits", logits, lg64, worst, rows=S * N)
    _check(case, "probs", probs, pr64, worst)
    _check(case, "values", values, v64, worst)
    _check(case, "scalar", scalar, sc64, worst)
    _check(case, "critic_loss", loss, l64, worst)
    tb = _out_bias_terms(v64, R.critic_std(c64), rets, N if crit.aggregator_type == "sum" else 1)
    for pre, net, ref in (("pol", pol, p64), ("crit", crit, c64)):
        for name, p in net.named_parameters():
            got = torch.zeros_like(p) if p.grad is None else p.grad
            want = ref[name].grad if ref[name].grad is not None else torch.zeros_like(ref[name])   # (no hop: linear_in unused)
            _check(case, f"g{pre}.{name}", got, want, worst, terms=tb if f"g{pre}.{name}" == CRIT_OUT_BIAS else None)
    return worst


def _assert_path(case, spy, path, reps, det, d):
    names = spy.names()
    kind = path.split("+")[0]
    if kind == "layers0":                                                    # no hop: no aggregation kernel at all
        must, must_not = {"cm_attention_forward", "cm_linear_act_backward"}, {"cm_masked_agg_forward",
                                                                                                       "cm_policy_forward_saved"}
    else:
        must, must_not = PATHS[kind]
    if path == "fused+direct":                                               # the critic's 'direct' head: per-layer critic
        must = (must - {"cm_critic_forward_saved"}) | {"cm_masked_agg_forward"}
        must_not = must_not - {"cm_masked_agg_forward", "cm_attention_forward"}
    if det:
        must = {DET_NAMES.get(n, n) for n in must}
    if d > 64 and kind in ("fused", "wave"):                                 # the one-pass encoder chain declines: two layers
        must = must | {"cm_linear_act_backward_det" if det else "cm_linear_act_backward"}
    missing, unexpected = must - names, must_not & names
    assert not missing and not unexpected, f"{case}: path '{path}' not taken: missing {sorted(missing)}, unexpected {sorted(unexpected)}"
    if reps is not None and not det:
        assert spy.replicas() == {reps}, f"{case}: bias_replicas {sorted(spy.replicas())}, expected {reps}"


def _run_case(name, det, spy):
    import com_marl_amd
    N, S, d, hops, residual, att, agg, masks, path, reps, note = CASES[name]
    t0 = time.time()
    pol, crit = _nets(N, d, hops, residual, att, agg, seed=N * 7 + hops)
    obs, adj, ch, avail, acts, wts, rets = _inputs(N, S, d, hops, masks, seed=N * 11 + S)
    com_marl_amd.set_deterministic(det)
    try:
        spy.calls.clear()
        worst = _run_and_compare(name, pol, crit, N, residual, obs, adj, ch, avail, acts, wts, rets)
    finally:
        com_marl_amd.set_deterministic(None)
    _assert_path(name, spy, path, reps, det, d)
    if path == "layers" and N <= 80:
        # teams the one-launch forward serves, with observations it does not: the no-grad evaluation of the PPO epoch
        # (algos.py: evaluate_nograd) must take a kernel that exists too
        with torch.no_grad():
            _, p_ng = pol.evaluate_nograd(obs, adj, ch)
            p64 = R.params(pol.state_dict(), device=DEV, requires_grad=False)
            w = lambda t: None if t is None else t.to(F64)                    # noqa: E731
            _, pr64, _ = R.policy_forward(p64, w(obs), None, w(adj), w(ch), N, residual)
        _check(name, "evaluate_nograd probs", p_ng, pr64, worst)
    print(f"{name}{' det' if det else ''} [{note}]: {_summary(worst)}, {time.time() - t0:.1f}s")


@pytest.mark.parametrize("name", sorted(CASES))
def test_training_backward_matches_f64(name, spy):
    _run_case(name, False, spy)


@pytest.mark.parametrize("name", DET_CASES)
def test_training_backward_matches_f64_deterministic(name, spy):
    _run_case(name, True, spy)


NET_GRADS = {"net_grads_co_map20": (24, "fused"), "net_grads_co_map30_iid": (54, "fused"), "net_grads_pp_map30": (72, "fused"),
             "net_grads_co_map40": (96, "layers"), "net_grads_pp_map40": (128, "layers")}


@pytest.mark.parametrize("fixture", sorted(NET_GRADS))
def test_net_grads_fixture(fixture, spy):
    """The reference's recorded scalar, critic loss and gradients of the default net, through the HIP training path."""
    import os
    from com_marl_amd import envs as E, nets
    from tests.test_oracle_golden import GOLDEN
    N, path = NET_GRADS[fixture]
    z = np.load(os.path.join(GOLDEN, fixture + ".npz"))
    obs, adj, ch, avail, acts, wts, rets = (torch.as_tensor(z[k]).to(DEV) for k in ("obs", "adj", "channels", "avail", "actions",
                                                                                   "weights", "returns"))
    d = obs.shape[1] // N
    spec = E.EnvSpec(E._Box(np.zeros(d * N), np.ones(d * N)), E._Discrete(5))
    pol = nets.CommCategoricalMLPPolicy(spec, n_agents=N, device=DEV)
    crit = nets.CommBaseCritic(spec, n_agents=N, device=DEV)
    pol.load_state_dict({k[4:]: torch.as_tensor(z[k]) for k in z.files if k.startswith("pol.")})
    crit.load_state_dict({k[5:]: torch.as_tensor(z[k]) for k in z.files if k.startswith("crit.")})
    spy.calls.clear()
    logits = pol._logits(obs, adj, ch)
    probs = R.masked_probs(logits, avail)
    scalar = R.ppo_scalar(probs, acts, wts)
    pol.zero_grad()
    scalar.backward()
    values, std = crit._values_grad(obs, adj, ch)
    loss = R.critic_nll(values, std, rets)
    crit.zero_grad()
    loss.backward()
    torch.cuda.synchronize()
    _assert_path(fixture, spy, path, 1 if path == "fused" else None, False, d)
    worst = {}
    _check(fixture, "probs", probs, z["probs"], worst)
    _check(fixture, "values", values, z["values"], worst)
    _check(fixture, "scalar", scalar, z["scalar"], worst)
    _check(fixture, "critic_loss", loss, z["critic_loss"], worst)
    tb = _out_bias_terms(z["values"], np.exp(float(z["crit.baseline_aggregator._init_std"].reshape(-1)[0])), z["returns"], N)
    for pre, net in (("gpol", pol), ("gcrit", crit)):
        for name, p in net.named_parameters():
            _check(fixture, f"{pre}.{name}", p.grad, z[f"{pre}.{name}"], worst, terms=tb if f"{pre}.{name}" == CRIT_OUT_BIAS else None)
    print(f"{fixture}: {_summary(worst)}")
