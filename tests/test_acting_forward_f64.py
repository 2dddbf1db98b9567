"""The acting forward - act_device (and get_actions on top of it), evaluate_nograd, values_device, through whatever kernel a
shape reaches - and its action sampler against the float64 restatement (tests/f64_commnet.py, pinned to the reference by
tests/test_f64_commnet.py) where a TRAINED policy sits: logits in the tens, probabilities exactly 0 after the `avail` mask or
within 1e-7 of 1, saturated tanh units, one-hot attention rows (tests/acting_regimes.py; tests/test_acting_regimes_cpu.py shows
on the CPU that each input is what its name says, that the kernels' split-f16 scheme alone stays within half the bar on it, and
that next to none of the sampler's draws is undecided at that bar).  The rollout kernels are tied to these bit for bit
(tests/test_hip_fused_parity.py, in the same regimes), so what is judged here carries over.

CASES names each route with the rule that selects it.  The C entry points that ran are recorded by a proxy around
com_marl_amd._lib.lib() and asserted; INSIDE cm_policy_forward the kernel is chosen by shape, and the note cites that rule
(csrc: mw::shape_ok_w, policy_shape_ok, nets.MAX_FUSED_AGENTS) instead of pretending to observe it.  One choice in there IS
observed: the split-f16 launcher answers "not for this shape" where its LDS need exceeds 160 KB and cm_policy_forward then runs the
all-f32 matrix-core kernel without a word, so the 'split' rows also ask cm_policy_forward_saved - which has the split-f16 kernel and
nothing behind it - for the same probabilities and require them bit for bit (as test_evaluate_nograd_shares_one_forward does at
N = 6): a silent fall to the f32 kernel would differ in the last bits and fail.  (evaluate_nograd takes no `avail`, so in the 'avail'
setting the kernel is inferred from the other two settings of the same shape: the choice depends on the shape alone.)  The wave-owned acting kernel
takes `avail` itself (policy_forward_w declines only a saved forward; its training twin policy_forward_w_train is the one that
refuses `avail`), so the 'avail' runs of the N = 4 rows judge that kernel's own mask-and-renormalise, not the split-f16 kernel's.

Per case, regime and mask setting (none / range and channel masks / those plus `avail`), TAU = 1e-5:
  * probabilities, attention, values: max|got - ref64| <= TAU * max|ref64|; evaluate_nograd's logits also per agent row;
  * log-probabilities, which is what judges a peaked row: where p64 >= 1e-30, |log p - log p64| <= 2 TAU max|logits64| (log-softmax
    is 2-Lipschitz in the sup norm of the logits; the `avail` renormalisation is a log-softmax over the available logits); where
    p64 < 1e-30, 0 <= p <= 1e-29;
  * every probability row finite, non-negative, summing to 1 within 1e-6; a masked action has probability exactly 0;
  * sampled actions (fixed seed, env_id_offset, policy_step) == the oracle's inverse-CDF draw on the kernel's own probabilities,
    exactly; == the float64 rule on the float64 probabilities except where the uniform lies within 5e-5 of a float64 CDF boundary
    (at most 1 % of the draws); never an unavailable action, no exclusion; greedy likewise against the float64 argmax except where
    the float64 top two are within 2e-5.  (The sampler's fallback for a uniform beyond the end of the float32 CDF - the last action
    with p > 0 - is not reached at the fixed seed, about 1e-7 per draw: on the GPU it is judged only through the oracle's draw
    agreeing wherever it would be; the rule itself is pinned by the hand-made table of tests/test_acting_regimes_cpu.py.)
  * the PEAKED regimes reached the kernel on every route, the seeded nets included: max|logit64| >= 20 and a row above 0.99 under
    head40, max|logit64| >= 7 under enc14_head12.
Each case prints its ratios next to those of the restatement run in float32: how far above float32 noise a kernel sits."""
import ctypes as C
import os
import time

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import acting_regimes as G
from tests import any_shapes as AS
from tests import f64_commnet as R
from tests.lib_spy import spy  # noqa: F401  (the fixture: a recording proxy around _lib.lib())
from tests.test_oracle_golden import GOLDEN

pytestmark = pytest.mark.gpu

TAU = 1e-5
DEV = "cuda:0"
F64 = torch.float64


LAYER_OPS = {"cm_attention_forward", "cm_masked_agg_forward", "cm_mlp_policy_forward"}
# route -> (entry points that must run, entry points that must not)
ROUTES = {
    "act": ({"cm_policy_forward"}, LAYER_OPS | {"cm_policy_forward_any", "cm_policy_forward_saved"}),
    "split": ({"cm_policy_forward"}, LAYER_OPS | {"cm_policy_forward_any", "cm_policy_forward_saved"}),
    "plain": ({"cm_policy_forward"}, LAYER_OPS | {"cm_policy_forward_any", "cm_policy_forward_saved"}),
    "saved": ({"cm_policy_forward_saved"}, LAYER_OPS | {"cm_policy_forward", "cm_policy_forward_saved_wave", "cm_policy_forward_any"}),
    "layers": (LAYER_OPS, {"cm_policy_forward", "cm_policy_forward_any", "cm_policy_forward_saved"}),
    "any": ({"cm_policy_forward_any"}, LAYER_OPS | {"cm_policy_forward"}),
    "critic": ({"cm_critic_forward"}, {"cm_critic_forward_any", "cm_masked_agg_forward", "cm_critic_forward_saved"}),
}
ALL, PEAKED = tuple(sorted(G.REGIMES)), G.PEAKED
# the recorded one-hop net without the skip connection: its head sees H_1 alone and HO x12 / HO x40 leave its logits at 3 / 10
# (tests/test_acting_regimes_cpu.py: DROPPED), so the two head-only regimes are not claimed for it; enc14_head12 peaks it
NO_HEAD_ONLY = tuple(r for r in ALL if r not in ("head12", "head40"))

# name: (route, N, S, d, hops, residual, weights (a fixture | None: a seeded net | an any_shapes shape), masked_row, regimes, note)
CASES = {
    "wave_n4": ("act", 4, 37, 21, 2, True, "policy_pp_map10", False, ALL,
                "act_device, mw::shape_ok_w (N == 4, d <= 32, 1-2 hops): wave-owned kernel, `avail` included; 5 workgroups, the last ragged"),
    "wave_n4_hop1_nores": ("act", 4, 37, 21, 1, False, "policy_pp_map10_hops1_nores", False, NO_HEAD_ONLY,
                           "wave-owned kernel, one hop, no skip connection (head12 / head40 do not take hold on this net: not run)"),
    "saved_n4": ("saved", 4, 37, 21, 2, True, "policy_pp_map10", False, ALL,
                 "evaluate_nograd below COMMARL_TRAIN_FWD_WAVE_MIN envs: split-f16 kernel at N = 4 (cm_policy_forward_saved), logits + probabilities"),
    "split_n3": ("split", 3, 9, 21, 2, True, None, False, PEAKED, "policy_shape_ok, not shape_ok_w: split-f16 kernel, first-generation N x N"),
    "split_n8": ("split", 8, 13, 30, 2, True, None, False, PEAKED, "split-f16 kernel, matrix-core N x N, ragged last workgroup"),
    "split_n24": ("split", 24, 5, 77, 2, True, "policy_co_map20", False, ALL, "split-f16 kernel, d > 64, config 3 team size"),
    "split_n54_masked_row": ("split", 54, 3, 77, 2, True, "policy_co_map30_iid", True, PEAKED,
                             "split-f16 kernel, one env per workgroup, an agent whose range mask is all zero"),
    "split_n80_hops3_nores": ("split", 80, 2, 40, 3, False, None, False, PEAKED, "split-f16 kernel at nets.MAX_FUSED_AGENTS (its LDS need, lds_map(..).total, still within 160 KB), three hops, no skip connection (seeded head output layer x2)"),
    "layers_n96": ("layers", 96, 2, 77, 2, True, None, False, PEAKED,
                   "N > nets.MAX_FUSED_AGENTS: layer by layer, head + sampler on the row-MLP kernel (cm_mlp_policy_forward)"),
    "plain_n5": ("plain", 5, 11, 21, 2, True, None, False, PEAKED,
                 "cm_policy_forward called with mfma_pack = NULL: generic VALU kernel on the plain weights"),
    "plain_d100": ("act", 4, 11, 100, 2, True, None, False, PEAKED,
                   "d = 100: kpad_of(d) == 0, policy_shape_ok fails, no operand pack exists: generic VALU kernel"),
    "any_A": ("any", 4, AS.N_ENVS, 21, 2, True, "A", False, PEAKED,
              "layer sizes (96, 48) | 32 | (48, 24): cm_policy_forward_any, _last_forward == 'one_launch'"),
    "critic_n4": ("critic", 4, 37, 21, 2, True, "policy_pp_map10", False, G.CRITIC_REGIMES, "values_device, split-f16 critic kernel"),
    "critic_n24": ("critic", 24, 5, 77, 2, True, "policy_co_map20", False, G.CRITIC_REGIMES, "values_device"),
    "critic_n54_masked_row": ("critic", 54, 3, 77, 2, True, "policy_co_map30_iid", True, G.CRITIC_REGIMES, "values_device, a fully masked agent"),
}
PARAMS = [(name, regime) for name in CASES for regime in CASES[name][8]]


def _sd_of(z, pre):
    return {k[len(pre) + 1:]: z[k] for k in z.files if k.startswith(pre + ".")}


def _net(name):
    """-> (net with its UNSCALED weights, pool of recorded per-agent observations | None)."""
    from com_marl_amd import envs as E, nets
    route, N, S, d, hops, residual, weights, _, _, _ = CASES[name]
    critic = route == "critic"
    if route == "any":
        pol, _ = AS.build(weights, device=DEV, critic=False)
        return pol, AS.fixture(AS.SHAPES[weights]["fixture"])["obs"]
    spec = E.EnvSpec(E._Box(np.zeros(d * N), np.ones(d * N)), E._Discrete(5))
    torch.manual_seed(N * 7 + hops)
    cls = nets.CommBaseCritic if critic else nets.CommCategoricalMLPPolicy
    net = cls(spec, n_agents=N, n_gcn_layers=hops, residual=residual, device=DEV)
    if weights is None:
        with torch.no_grad():
            for pname, p in net.named_parameters():
                if pname.endswith("bias") and "gcn" not in pname:
                    p.uniform_(-0.1, 0.1)
            if not residual:       # the head sees H_L alone, a third of E + H_L's scale: an output layer twice as large keeps the
                net.state_dict()[G.HO].mul_(2.0)     # seeded net's logits where the head regimes' names promise them
        return net, None
    z = np.load(os.path.join(GOLDEN, weights + ".npz"))
    net.load_state_dict({k: torch.as_tensor(v) for k, v in _sd_of(z, "crit" if critic else "pol").items()}, strict=True)
    return net, z["obs"]


def _setup(name, regime, masks):
    """The case's net in the regime (float32 values through apply(), strict load, sync_weights) and its inputs (numpy)."""
    route, N, S, d, hops, residual, _, masked_row, _, _ = CASES[name]
    net, pool = _net(name)
    sd32 = G.apply(net.state_dict(), regime)
    net.load_state_dict({k: torch.as_tensor(v) for k, v in sd32.items()}, strict=True)
    net.sync_weights()
    obs, avail, adj, ch = G.inputs(N, S, d, hops, masks, seed=N * 11 + S, obs_pool=pool, masked_row=masked_row)
    return net, sd32, (obs, avail, adj, ch)


def _dev(a):
    return None if a is None else torch.as_tensor(a).to(DEV).contiguous()


def _t64(a):
    return None if a is None else torch.as_tensor(np.asarray(a), dtype=F64)


def _act(route, pol, obs, avail, adj, ch, greedy):
    """-> (actions, probs, attn) numpy, sampler stream (G.SEED, G.ENV_ID_OFFSET, G.POLICY_STEP)."""
    from com_marl_amd import _lib as L
    pol.set_rng(G.SEED, G.ENV_ID_OFFSET)
    if route != "plain":
        a, p, m = pol.act_device(obs, avail, adj, ch, greedy=greedy, policy_step=G.POLICY_STEP)
    else:                                          # as test_operand_pack_path_equals_plain_weight_path: no operand pack handed over
        N, S = pol._n_agents, obs.shape[0]
        w = pol._weights_struct()
        assert w.mfma_pack
        w.mfma_pack = None
        a = torch.empty(S, N, dtype=torch.int32, device=DEV)
        p = torch.empty(S, N, 5, device=DEV)
        m = torch.empty(S, N, N, device=DEV)
        L.check(L.lib().cm_policy_forward(C.byref(w), S, L.ptr(obs), L.ptr(avail), L.ptr(adj), L.ptr(ch), G.SEED, G.ENV_ID_OFFSET,
                                          G.POLICY_STEP, None, int(greedy), L.ptr(a), L.ptr(p), L.ptr(m), L.current_stream()),
                "cm_policy_forward (plain weights)")
    torch.cuda.synchronize()
    return a.cpu().numpy().astype(np.int64), p.cpu().numpy(), m.cpu().numpy()


def _ratio(tag, name, got, ref, f32, worst, rows=None):
    r = R.ratio(got, ref)
    if rows is not None:
        r = max(r, R.row_ratio(got, ref, rows))
    b = R.ratio(f32, ref) if rows is None else max(R.ratio(f32, ref), R.row_ratio(f32, ref, rows))
    worst[name] = (r, b)
    assert r <= TAU, f"{tag}: {name} off by {r:.3g} of its scale (float32 restatement {b:.3g}; tolerance {TAU})"


def _check_rows(tag, probs, avail):
    p = np.asarray(probs, np.float64)
    assert np.isfinite(p).all() and (p >= 0).all(), f"{tag}: a probability is negative or not finite"
    s = np.abs(p.sum(-1) - 1).max()
    assert s <= 1e-6, f"{tag}: a probability row sums to 1 -+ {s:.3g}"
    if avail is not None:
        assert (p[np.asarray(avail).reshape(p.shape) == 0] == 0).all(), f"{tag}: a masked action has a non-zero probability"


def _check_logp(tag, probs, pr64, lg64, worst):
    p, p64 = np.asarray(probs, np.float64), pr64.numpy()
    big = p64 >= 1e-30
    bound = 2 * TAU * float(lg64.abs().max())
    with np.errstate(divide="ignore"):
        err = float(np.abs(np.log(p[big]) - np.log(p64[big])).max())
    worst["logp"] = (err / bound * TAU, 0.0)                      # in units of the bound, scaled so that TAU is the limit
    assert err <= bound, f"{tag}: log-probabilities off by {err:.3g} (bound 2 TAU max|logits64| = {bound:.3g})"
    assert (p[~big] <= 1e-29).all(), f"{tag}: a probability whose float64 value is below 1e-30 came out as {p[~big].max():.3g}"


def _check_sampler(tag, route, pol, dev_in, avail, probs, acts, pr64, worst):
    S, N = acts.shape
    want = O.sample_actions(np.ascontiguousarray(probs, np.float32), G.SEED, G.ENV_ID_OFFSET, G.POLICY_STEP)
    np.testing.assert_array_equal(acts, want, err_msg=f"{tag}: sampled actions != the oracle's draw on the kernel's own probabilities")
    g_acts, g_probs, _ = _act(route, pol, *dev_in, greedy=True)
    np.testing.assert_array_equal(g_probs, probs, err_msg=f"{tag}: greedy and sampled calls returned other probabilities")
    if avail is not None:
        av = np.asarray(avail).reshape(S, N, 5)
        for what, a in (("sampled", acts), ("greedy", g_acts)):
            assert (np.take_along_axis(av, a[..., None], -1) == 1).all(), f"{tag}: a {what} action is not available"
    u = G.uniforms(G.SEED, G.ENV_ID_OFFSET, G.POLICY_STEP, S, N)
    near = G.near_boundary(pr64, u, G.DELTA)
    assert near.mean() <= G.MAX_EXCLUDED, f"{tag}: {near.mean():.4f} of the draws within {G.DELTA} of a float64 CDF boundary"
    a64 = G.cdf_actions64(pr64, u)
    assert (acts[~near] == a64[~near]).all(), \
        f"{tag}: {int((acts[~near] != a64[~near]).sum())} sampled actions differ from the float64 rule away from every CDF boundary"
    und = G.greedy_undecided(pr64)
    assert und.mean() <= G.MAX_EXCLUDED, f"{tag}: {und.mean():.4f} of the rows with a float64 top-two gap below {G.GREEDY_GAP}"
    g64 = pr64.numpy().argmax(-1)
    assert (g_acts[~und] == g64[~und]).all(), f"{tag}: {int((g_acts[~und] != g64[~und]).sum())} greedy actions differ from the float64 argmax"
    worst["excluded"] = (float(near.mean()), float(und.mean()))


def _assert_route(tag, spy, route):
    must, must_not = ROUTES[route]
    names = set(spy.calls)
    missing, unexpected = must - names, must_not & names
    assert not missing and not unexpected, f"{tag}: route '{route}' not taken: missing {sorted(missing)}, unexpected {sorted(unexpected)}"


def _line(worst):
    out = [f"{k} {v[0]:.1e} (f32 {v[1]:.1e})" for k, v in worst.items() if k not in ("logp", "excluded")]
    if "logp" in worst:
        out.append(f"logp {worst['logp'][0] / TAU:.2f} of its bound")
    if "excluded" in worst:
        out.append(f"excluded draws {worst['excluded'][0]:.4f}, greedy rows {worst['excluded'][1]:.4f}")
    return ", ".join(out)


def _run_policy(name, regime, masks, spy):
    route, N, S, d, hops, residual, weights, _, _, note = CASES[name]
    tag = f"{name} {regime} {masks}"
    pol, sd32, (obs, avail, adj, ch) = _setup(name, regime, masks)
    if name == "plain_d100":
        assert pol._mfma is None, "d = 100 got an operand pack: the case no longer reaches the generic kernel"
    dev_in = tuple(map(_dev, (obs, avail, adj, ch)))
    p64 = R.params(sd32, requires_grad=False)
    with torch.no_grad():
        lg64, pr64, at64 = R.policy_forward(p64, _t64(obs), _t64(avail), _t64(adj), _t64(ch), N, residual)
    lg32, pr32, at32 = G.f32_forward(sd32, obs, avail, adj, ch, N, residual)
    worst = {}
    spy.calls.clear()
    if route == "saved":
        logits, probs = pol.evaluate_nograd(dev_in[0], dev_in[2], dev_in[3])
        torch.cuda.synchronize()
        _assert_route(tag, spy, route)
        logits, probs = logits.cpu().numpy(), probs.cpu().numpy()
        _ratio(tag, "logits", logits, lg64, lg32, worst, rows=S * N)
    else:
        acts, probs, attn = _act(route, pol, *dev_in, greedy=False)
        _assert_route(tag, spy, route)
        if route == "split" and avail is None:                   # the kernel inside cm_policy_forward, observed (module docstring)
            _, p_saved = pol.evaluate_nograd(dev_in[0], dev_in[2], dev_in[3])
            assert "cm_policy_forward_saved" in spy.calls
            np.testing.assert_array_equal(p_saved.cpu().numpy(), probs, err_msg=f"{tag}: act_device did not run the split-f16 kernel")
        if route == "any":
            assert pol._last_forward == "one_launch", pol._last_forward
        _ratio(tag, "attn", attn, at64, at32, worst)
    _ratio(tag, "probs", probs, pr64, pr32, worst)
    _check_rows(tag, probs, avail)
    _check_logp(tag, probs, pr64, lg64, worst)
    if route != "saved":
        _check_sampler(tag, route, pol, dev_in, avail, probs, acts, pr64, worst)
    max_logit, peaked = float(lg64.abs().max()), float((pr64.amax(-1) > 0.99).double().mean())
    if regime == "head40":
        assert max_logit >= 20 and peaked > 0, f"{tag}: the regime did not reach the kernel (max|logit64| {max_logit:.1f}, rows p > .99 {peaked:.2f})"
    if regime == "enc14_head12":
        assert max_logit >= 7, f"{tag}: the regime did not reach the kernel (max|logit64| {max_logit:.1f})"
    return worst, max_logit, peaked


@pytest.mark.parametrize("name,regime", [p for p in PARAMS if CASES[p[0]][0] != "critic"])
def test_acting_forward_matches_f64(name, regime, spy):
    route, note = CASES[name][0], CASES[name][9]
    t0 = time.time()
    for masks in (G.MASKS[:2] if route == "saved" else G.MASKS):     # (evaluate_nograd takes no `avail`)
        worst, max_logit, peaked = _run_policy(name, regime, masks, spy)
        print(f"{name} {regime} {masks}: max|logit64| {max_logit:.1f}, rows p > .99 {peaked:.2f}; {_line(worst)}")
    print(f"{name} {regime} [{note}]: {time.time() - t0:.1f}s")


@pytest.mark.parametrize("name,regime", [p for p in PARAMS if CASES[p[0]][0] == "critic"])
def test_critic_values_match_f64(name, regime, spy):
    route, N, S, d, hops, residual, weights, _, _, note = CASES[name]
    t0 = time.time()
    for masks in G.MASKS[:2]:
        tag = f"{name} {regime} {masks}"
        crit, sd32, (obs, _, adj, ch) = _setup(name, regime, masks)
        spy.calls.clear()
        values = crit.values_device(_dev(obs), _dev(adj), _dev(ch))
        torch.cuda.synchronize()
        _assert_route(tag, spy, route)
        with torch.no_grad():
            v64 = R.critic_values(R.params(sd32, requires_grad=False), _t64(obs), _t64(adj), _t64(ch), N, residual, "sum")
            c32 = {k: torch.as_tensor(v) for k, v in sd32.items()}
            f = lambda a: None if a is None else torch.as_tensor(a)                              # noqa: E731
            v32 = R.critic_values(c32, f(obs), f(adj), f(ch), N, residual, "sum")
        worst = {}
        _ratio(tag, "values", values.cpu().numpy(), v64, v32, worst)
        print(f"{tag}: {_line(worst)}")
    print(f"{name} {regime} [{note}]: {time.time() - t0:.1f}s")


def test_get_actions_is_act_device(spy):
    """The numpy-in / numpy-out call of the reference's sampler: same kernel, same stream, same answers as act_device."""
    pol, sd32, (obs, avail, adj, ch) = _setup("wave_n4", "head40", "avail")
    pol.set_rng(G.SEED, G.ENV_ID_OFFSET)
    pol._policy_step = G.POLICY_STEP
    acts, infos = pol.get_actions(obs, avail.reshape(obs.shape[0], -1), adj, ch)
    a, p, m = _act("act", pol, *map(_dev, (obs, avail, adj, ch)), greedy=False)
    np.testing.assert_array_equal(acts, a)
    np.testing.assert_array_equal(np.stack(infos["action_probs"]), p)
    np.testing.assert_array_equal(np.stack(infos["attention_weights"]), m)
