"""entropy_method='max' and the entropy switches (use_softplus_entropy, stop_entropy_gradient) of CentralizedMAPPO:
cm_entropy_gae and the CM_ENT_* bits of cm_ppo_surrogate against float64 torch compositions of the reference formulas
(centralized_ma_ppo.py:415-438, :499-538), reference train_once recordings (tests/golden/ppo_epoch_max_*.npz,
ppo_step_entropy_switches.npz, written by tools/gen_golden_entropy.py), the update graphs and the drop-in runner script."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from tests.test_oracle_golden import GOLDEN

EPS = float(np.finfo(np.float32).eps)
KINDS = ("obsdp", "cent", "comm")


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def _cpu_algo(**kw):
    import torch
    from com_marl_amd.algos import CentralizedMAPPO
    pol, crit = torch.nn.Linear(2, 2), torch.nn.Linear(2, 1)                 # stub nets: the ctor only needs parameters
    return CentralizedMAPPO(env_spec=None, policy=pol, baseline=crit, **kw)


def test_ctor_accepts_the_entropy_settings():
    a = _cpu_algo(entropy_method="max", center_adv=False, stop_entropy_gradient=True, policy_ent_coeff=0.1)
    assert a._maximum_entropy and not a._entropy_regularzied and a._entropy_flags() == 0
    a = _cpu_algo(entropy_method="max", center_adv=False, stop_entropy_gradient=True, use_softplus_entropy=True,
                  positive_adv=True, policy_ent_coeff=0.1)
    assert a._use_softplus_entropy and a._positive_adv
    for sp in (False, True):
        for stop in (False, True):
            a = _cpu_algo(entropy_method="regularized", use_softplus_entropy=sp, stop_entropy_gradient=stop,
                          policy_ent_coeff=0.1)
            assert a._entropy_flags() == 1 | (2 if sp else 0) | (4 if stop else 0)
    a = _cpu_algo(entropy_method="no_entropy", use_softplus_entropy=True, stop_entropy_gradient=True)
    assert a._entropy_flags() == 0


@pytest.mark.parametrize("kw,msg", [
    (dict(entropy_method="max", center_adv=True, stop_entropy_gradient=True), "center_adv should be False"),
    (dict(entropy_method="max", center_adv=False, stop_entropy_gradient=False), "stop_gradient should be True"),
    (dict(entropy_method="no_entropy", policy_ent_coeff=0.1), "policy_ent_coeff should be zero"),
    (dict(entropy_method="maximum"), "Invalid entropy_method")])
def test_ctor_keeps_the_reference_refusals(kw, msg):
    with pytest.raises(ValueError, match=msg):
        _cpu_algo(**kw)


def test_entropy_fixtures_have_what_the_gpu_tests_read():
    for kind in KINDS:
        z = np.load(os.path.join(GOLDEN, f"ppo_epoch_max_{kind}.npz"))
        P, T = z["rewards"].shape
        assert str(z["kind"]) == kind and T == 12 and P == 9 and sorted(z["perm"]) == list(range(P))
        assert int(z["n_calls"]) == 11 and z["valids"].min() < T                       # 1 + 3 x 3 + 1 calls; ragged
        for k in ("obs", "actions", "rewards64", "baselines", "returns", "dist_adjs", "channels", "LossBefore", "LossAfter",
                  "Entropy", "loss_before_full", "loss_after_full", "ent_coeff", "positive_adv"):
            assert k in z.files, (kind, k)
        for i in range(11):
            n = P if i in (0, 10) else 3
            assert z[f"call{i}.rewards"].shape == z[f"call{i}.adv"].shape == (n, T)
        assert any(k.startswith("pol0.") for k in z.files) and any(k.startswith("pol1.") for k in z.files)
        assert any(k.startswith("crit1.") for k in z.files)
        # the in-place quirk as recorded: a minibatch step's GAE sees the loss_before rewards (r + c H_before) again
        ids = z["perm"][:3]
        assert np.all(z["call0.rewards"][ids] - z["rewards"][ids] > 0)
        assert float((z["call1.rewards"] - z["rewards"][ids]).mean()) > 1.8 * float((z["call0.rewards"] - z["rewards"])[ids].mean())
    assert int(np.load(os.path.join(GOLDEN, "ppo_epoch_max_cent.npz"))["positive_adv"]) == 1
    z = np.load(os.path.join(GOLDEN, "ppo_step_entropy_switches.npz"))
    for tag in ("sp", "spstop"):
        for step in (1, 2):
            assert z[f"{tag}.loss{step}"].shape == ()
            assert any(k.startswith(f"{tag}.gpol{step}.") for k in z.files)


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need the MI355X")
    return torch


def _entropy64(torch, logits):
    """Per-step mean-over-agents entropy of Categorical(probs=softmax(logits) / sum) in float64, with the reference's
    log(clamp(p, eps, 1 - eps))."""
    p = torch.softmax(logits.double(), -1)
    p = p / p.sum(-1, keepdim=True)
    p = p / p.sum(-1, keepdim=True)
    return -(p * torch.log(p.clamp(EPS, 1 - EPS))).sum(-1).mean(-1)


def _gae64(torch, r, v, gamma, lam):
    P, T = r.shape
    adv = torch.zeros_like(r)
    acc = torch.zeros(P, dtype=r.dtype, device=r.device)
    vnext = torch.zeros_like(acc)
    for t in range(T - 1, -1, -1):
        acc = r[:, t] + gamma * vnext - v[:, t] + gamma * lam * acc
        adv[:, t] = acc
        vnext = v[:, t]
    return adv


@pytest.mark.gpu
@pytest.mark.parametrize("N", [4, 24, 72])
@pytest.mark.parametrize("T", [12, 500])
@pytest.mark.parametrize("softplus", [0, 1])
def test_entropy_gae_kernel_matches_float64(N, T, softplus, torch_cuda):
    """cm_entropy_gae: H (mean over agents, softplus after the mean), r + c H, GAE over the padded length, against float64
    torch; rewards_out aliased to rewards (the full-batch in-place add) and null (rewards untouched)."""
    torch = torch_cuda
    from com_marl_amd import _lib as L
    g = torch.Generator().manual_seed(N * 1000 + T + softplus)
    P, A, c, gamma, lam = 7, 5, 0.1, 0.99, 0.97
    lens = torch.randint(1, T + 1, (P,), generator=g)
    lens[0] = T
    logits = (torch.randn(P * T, N, A, generator=g) * 3).cuda()
    valid = torch.arange(T)[None, :] < lens[:, None]
    rew = (torch.randn(P, T, generator=g) * valid).cuda()                  # zero padding, as process_samples pads
    base = torch.randn(P, T, generator=g).cuda()
    h = _entropy64(torch, logits).reshape(P, T)
    if softplus:
        h = torch.nn.functional.softplus(h)
    r2 = rew.double() + c * h
    want = _gae64(torch, r2, base.double(), gamma, lam)
    scale = float(want.abs().max())
    for alias in (False, True):
        r_in = rew.clone()
        adv = torch.empty(P, T, device="cuda:0")
        ent = torch.empty(P, T, device="cuda:0")
        L.check(L.lib().cm_entropy_gae(P, T, N, A, L.ptr(logits), L.ptr(r_in), L.ptr(base), gamma, lam, c, softplus,
                                       L.ptr(r_in) if alias else None, L.ptr(ent), L.ptr(adv), L.current_stream()),
                "cm_entropy_gae")
        torch.cuda.synchronize()
        np.testing.assert_allclose(adv.cpu().numpy(), want.cpu().numpy(), rtol=0, atol=1e-5 * scale)
        np.testing.assert_allclose(ent.cpu().numpy(), h.cpu().numpy(), rtol=0, atol=1e-5 * float(h.abs().max()))
        if alias:
            np.testing.assert_allclose(r_in.cpu().numpy(), r2.cpu().numpy(), rtol=0, atol=1e-5 * float(r2.abs().max()))
        else:
            assert torch.equal(r_in, rew)
    # argument errors come back as CM_ERR_ARG with a message
    assert L.lib().cm_entropy_gae(P, T, N, 9, L.ptr(logits), L.ptr(rew), L.ptr(base), gamma, lam, c, 0, None, None,
                                  L.ptr(adv), L.current_stream()) != 0
    assert b"n_actions" in L.lib().cm_last_error()
    assert L.lib().cm_entropy_gae(P, T, N, A, None, L.ptr(rew), L.ptr(base), gamma, lam, c, 0, None, None, L.ptr(adv),
                                  L.current_stream()) != 0
    assert b"null" in L.lib().cm_last_error()


def _surrogate(torch, logits, actions, old_ll, adv, lens, c, flags):
    from com_marl_amd.algos import _SurrogateFn
    lg = logits.clone().requires_grad_(True)
    total, count = _SurrogateFn.apply(lg, actions, old_ll, adv, lens, 0.1, c, flags)
    total.backward()
    return total.detach(), count, lg.grad


@pytest.mark.gpu
@pytest.mark.parametrize("softplus,stop", [(True, False), (False, True), (True, True)])
def test_surrogate_entropy_bits_match_autograd(softplus, stop, torch_cuda):
    """cm_ppo_surrogate with CM_ENT_SOFTPLUS / CM_ENT_STOP_GRAD against torch autograd (float64) of the reference objective
    (:434-435): min(r adv, clip(r) adv) + c * f(H), f = softplus or identity, H detached under stop-gradient.  The values 0 and
    1 of add_entropy are the original ones: the stop-gradient gradient is bit-identical to the no-entropy one and its loss
    bit-identical to the plain entropy bonus's when softplus is off."""
    torch = torch_cuda
    g = torch.Generator().manual_seed(7 + 2 * softplus + stop)
    P, T, N, A, c = 6, 40, 4, 5, 0.3
    lens = torch.randint(1, T + 1, (P,), generator=g).to(torch.int32).cuda()
    logits = (torch.randn(P, T, N, A, generator=g) * 2).cuda()
    actions = torch.randint(0, A, (P, T, N), generator=g).to(torch.int32).cuda()
    old_ll = (torch.randn(P, T, generator=g) * 0.2 - 6).cuda()
    adv = torch.randn(P, T, generator=g).cuda()
    flags = 1 | (2 if softplus else 0) | (4 if stop else 0)
    total, count, dl = _surrogate(torch, logits, actions, old_ll, adv, lens, c, flags)
    # float64 autograd of the reference objective
    lg = logits.double().clone().requires_grad_(True)
    p = torch.softmax(lg, -1)
    p = p / p.sum(-1, keepdim=True)
    p = p / p.sum(-1, keepdim=True)
    logp = torch.log(p.clamp(EPS, 1 - EPS))
    H = -(p * logp).sum(-1).mean(-1)
    if stop:
        H = H.detach()
    if softplus:
        H = torch.nn.functional.softplus(H)
    new_ll = logp.gather(-1, actions.long().unsqueeze(-1)).squeeze(-1).sum(-1)
    r = (new_ll - old_ll.double()).exp()
    obj = torch.min(r * adv.double(), r.clamp(0.9, 1.1) * adv.double()) + c * H
    mask = torch.arange(T, device="cuda:0")[None, :] < lens[:, None]
    want = -(obj * mask).sum()
    want.backward()
    assert int(count) == int(mask.sum())
    np.testing.assert_allclose(float(total), float(want.detach()), rtol=1e-5, atol=1e-5)
    gs = float(lg.grad.abs().max())
    np.testing.assert_allclose(dl.cpu().numpy(), lg.grad.cpu().numpy(), rtol=0, atol=1e-5 * gs)
    if stop:                                                                 # the term is in the loss, not in the gradient
        t0, _, d0 = _surrogate(torch, logits, actions, old_ll, adv, lens, c, 0)
        assert torch.equal(dl, d0)
        if not softplus:
            t1, _, _ = _surrogate(torch, logits, actions, old_ll, adv, lens, c, 1)
            assert torch.equal(total, t1)


def _fixture_paths(z):
    lens = z["valids"]
    return [dict(observations=z["obs"][i, :n], actions=z["actions"][i, :n], rewards=z["rewards64"][i, :n],
                 dist_adjs=z["dist_adjs"][i, :n], channels=z["channels"][i, :n]) for i, n in enumerate(lens)]


def _nets(torch, kind, z):
    from com_marl_amd import nets
    from com_marl_amd.envs import EnvSpec, _Box, _Discrete
    d_total = z["obs"].shape[-1]
    spec = EnvSpec(_Box(np.zeros(d_total), np.ones(d_total)), _Discrete(5))
    if kind == "comm":
        pol = nets.CommCategoricalMLPPolicy(spec, n_agents=4, device="cuda:0")
        crit = nets.CommBaseCritic(spec, n_agents=4, device="cuda:0")
    elif kind == "obsdp":
        pol = nets.DecCategoricalMLPPolicy(spec, 4, hidden_sizes=[128, 64, 32], name="dec_categorical_mlp_policy",
                                           device="cuda:0")
        crit = nets.CommBaseCritic(spec, n_agents=4, device="cuda:0")
    else:
        pol = nets.CentralizedCategoricalMLPPolicy(spec, n_agents=4, hidden_sizes=[128, 64, 32], name="centralized",
                                                   device="cuda:0")
        crit = nets.GaussianMLPBaseline(env_spec=spec, hidden_sizes=(64, 64, 64), device="cuda:0")
    pol.load_state_dict({k[5:]: torch.as_tensor(z[k]) for k in z.files if k.startswith("pol0.")})
    crit.load_state_dict({k[6:]: torch.as_tensor(z[k]) for k in z.files if k.startswith("crit0.")})
    return spec, pol, crit


def _max_algo(spec, pol, crit, positive_adv=False):
    from com_marl_amd.algos import CentralizedMAPPO
    return CentralizedMAPPO(env_spec=spec, policy=pol, baseline=crit, max_path_length=12, discount=0.99, center_adv=False,
                            positive_adv=positive_adv, gae_lambda=0.97, policy_ent_coeff=0.1, entropy_method="max",
                            stop_entropy_gradient=True, clip_grad_norm=7, optimization_n_minibatches=3,
                            optimization_mini_epochs=3, device="cuda:0")


def _epoch(torch, algo, z, monkeypatch, record=None, epochs=1, ref_baselines=True):
    """train_once on the fixture's paths with the recorded permutation and (ref_baselines) the recorded baselines (our
    critic's agree to 4e-5; the advantages are compared at 1e-5 of their scale).  record: list receiving (rewards in,
    in_place, adv) per _max_entropy_advantages call.  -> the full-batch rewards tensor of the last epoch."""
    perm = z["perm"].copy()
    monkeypatch.setattr(np.random, "permutation", lambda n: perm.copy())
    monkeypatch.setattr(algo, "_log_performance", lambda *a: {"AverageReturn": 0.0})
    orig_ps, seen = algo.process_samples, {}

    def process_samples(itr, paths):
        out = list(orig_ps(itr, paths))
        if ref_baselines:
            np.testing.assert_allclose(out[5].cpu().numpy(), z["baselines"], rtol=1e-5, atol=4e-5)
            out[5] = torch.as_tensor(z["baselines"]).cuda()
        seen["rewards"] = out[3]
        return tuple(out)
    monkeypatch.setattr(algo, "process_samples", process_samples)
    if record is not None:
        orig_adv = algo._max_entropy_advantages

        def adv_fn(logits, rewards, baselines, in_place):
            r_in = rewards.detach().clone()
            adv = orig_adv(logits, rewards, baselines, in_place)
            record.append((r_in, in_place, adv.detach().clone()))
            return adv
        monkeypatch.setattr(algo, "_max_entropy_advantages", adv_fn)
    for itr in range(epochs):
        algo.train_once(itr=itr, paths=_fixture_paths(z))
    return seen["rewards"]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_max_entropy_epoch_matches_reference(kind, torch_cuda, monkeypatch):
    """One eager train_once in entropy_method='max' against the reference's (tests/golden/ppo_epoch_max_<kind>.npz): the
    advantages of all 11 loss evaluations (loss before, 3 x 3 optimiser steps, loss after) and the rewards each one starts
    from, LossBefore / LossAfter (the full-batch losses) and Entropy at 1e-5 of scale, the weights after nine Adam steps.
    The minibatch steps must start from r + c H_before (the reference's in-place add on the full batch) and add their own
    entropy on top: with the entropy counted once the rewards check of calls 1..9 fails by ~c log 5."""
    torch = torch_cuda
    monkeypatch.setenv("COMMARL_UPDATE_GRAPH", "0")
    z = np.load(os.path.join(GOLDEN, f"ppo_epoch_max_{kind}.npz"))
    spec, pol, crit = _nets(torch, kind, z)
    positive = bool(int(z["positive_adv"]))
    algo = _max_algo(spec, pol, crit, positive_adv=positive)
    rec = []
    full_rewards = _epoch(torch, algo, z, monkeypatch, record=rec)
    assert len(rec) == int(z["n_calls"]) == 11
    assert [ip for _, ip, _ in rec] == [True] + [False] * 9 + [True]
    steps = [z["perm"][s:s + 3] for s in (0, 3, 6)] * 3

    def close(a, b, what):
        b = np.asarray(b, np.float64)
        np.testing.assert_allclose(np.asarray(a, np.float64), b, rtol=0, atol=1e-5 * max(float(np.abs(b).max()), 1e-6),
                                   err_msg=what)
    for i, (r_in, _, adv) in enumerate(rec):
        ref_adv = z[f"call{i}.adv"]
        if positive:
            ref_adv = ref_adv - ref_adv.min()                               # :428-429 on that call's advantages
        close(adv.cpu().numpy(), ref_adv, f"{kind} advantages of call {i}")
        if 1 <= i <= 9:         # the minibatch's rewards = the loss_before rewards r + c H_before, sliced
            close(r_in.cpu().numpy(), z["call0.rewards"][steps[i - 1]], f"{kind} rewards into call {i}")
    close(full_rewards.cpu().numpy(), z["call10.rewards"], f"{kind} rewards after loss_after (r + c H_before + c H_after)")
    s = algo.stats
    close(s["LossBefore"], z["loss_before_full"], "LossBefore")
    close(s["LossAfter"], z["LossAfter"], "LossAfter")
    close(s["Entropy"], z["Entropy"], "Entropy")
    # weights after nine Adam steps: Adam divides by sqrt(v) ~ |g|, so a gradient entry near zero whose sign flips between the
    # two arithmetic orders would move its weight by up to ~lr = 3e-4 per step.  Measured on the MI355X: 3.4e-7 (Obs-DP),
    # 5.2e-7 (CENT), 2.2e-7 (Comm-DP), no flip; the bound 5e-5 is ~100x that and a sixth of one flipped step.
    worst = 0.0
    for pre, net in (("pol1.", pol), ("crit1.", crit)):
        for name, p in net.state_dict().items():
            want = z[pre + name]
            d = float(np.abs(p.cpu().numpy() - want).max())
            worst = max(worst, d)
            np.testing.assert_allclose(p.cpu().numpy(), want, rtol=0, atol=5e-5, err_msg=f"{kind} {pre}{name}")
    print(f"{kind}: max |weights - reference| after the epoch = {worst:.2e}")


@pytest.mark.gpu
def test_entropy_switch_steps_match_reference(torch_cuda):
    """regularized + use_softplus_entropy, with and without stop_entropy_gradient: two full-batch optimiser steps of the
    Obs-DP nets against the reference (tests/golden/ppo_step_entropy_switches.npz): loss and every policy gradient at 1e-5 of
    the tensor's scale, on the fused surrogate (CM_ENT_* bits) and on the per-layer loss (COMMARL_FUSED_LOSS=0)."""
    torch = torch_cuda
    from com_marl_amd.algos import CentralizedMAPPO
    z = np.load(os.path.join(GOLDEN, "ppo_step_entropy_switches.npz"))
    worst = 0.0
    for fused in ("1", "0"):
        os.environ["COMMARL_FUSED_LOSS"] = fused
        try:
            for tag, stop in (("sp", False), ("spstop", True)):
                spec, pol, crit = _nets(torch, "obsdp", z)
                algo = CentralizedMAPPO(env_spec=spec, policy=pol, baseline=crit, max_path_length=12, discount=0.99,
                                        center_adv=True, positive_adv=False, gae_lambda=0.97, policy_ent_coeff=0.1,
                                        entropy_method="regularized", use_softplus_entropy=True,
                                        stop_entropy_gradient=stop, clip_grad_norm=7, optimization_n_minibatches=3,
                                        optimization_mini_epochs=10, device="cuda:0")
                obs, avail, actions, rewards, valids, baselines, returns, da, ch = algo.process_samples(0, _fixture_paths(z))
                baselines = torch.as_tensor(z["baselines"]).cuda()
                for step in (1, 2):
                    loss = algo._compute_loss(0, obs, avail, actions, rewards, valids, baselines, da, ch)
                    bl = algo._baseline_loss(obs, returns, da, ch)
                    np.testing.assert_allclose(loss.item(), z[f"{tag}.loss{step}"], rtol=1e-5, atol=1e-6,
                                               err_msg=f"{tag} fused={fused}")
                    algo._baseline_optimizer.zero_grad()
                    bl.backward()
                    algo._optimizer.zero_grad()
                    loss.backward()
                    for name, p in pol.named_parameters():
                        want = z[f"{tag}.gpol{step}.{name}"]
                        scale = max(1e-3, float(np.abs(want).max()))
                        worst = max(worst, float(np.abs(p.grad.cpu().numpy() - want).max()) / scale)
                        np.testing.assert_allclose(p.grad.cpu().numpy(), want, rtol=1e-4, atol=1e-5 * scale,
                                                   err_msg=f"{tag} fused={fused} grad {name} step {step}")
                    torch.nn.utils.clip_grad_norm_(pol.parameters(), 7)
                    algo._optimizer.step()
                    algo._baseline_optimizer.step()
        finally:
            os.environ.pop("COMMARL_FUSED_LOSS", None)
    print(f"worst gradient deviation / tensor scale: {worst:.2e}")


@pytest.mark.gpu
def test_max_entropy_update_graphs_take_the_eager_steps(torch_cuda, monkeypatch):
    """A Comm-DP 'max' epoch with its optimiser steps replayed from hipGraphs (COMMARL_UPDATE_GRAPH=1) against the same epoch
    eager (twice, for the run-to-run noise of the float-atomic gradient merges): parameters within that noise, the minibatch
    rewards buffers bit-unchanged by the replays (a step that wrote them would add c H again every mini-epoch), and a second
    epoch on the same shapes replays the graphs of the first and still matches eager."""
    torch = torch_cuda
    from com_marl_amd.algos import _UpdateGraphs
    z = np.load(os.path.join(GOLDEN, "ppo_epoch_max_comm.npz"))
    runs = {}
    for tag, mode in (("eager", "0"), ("eager2", "0"), ("graph", "1")):
        monkeypatch.setenv("COMMARL_UPDATE_GRAPH", mode)
        spec, pol, crit = _nets(torch, "comm", z)
        algo = _max_algo(spec, pol, crit)
        mb_rewards = {}
        orig_step = _UpdateGraphs.step

        def step(self, i, inputs, fn, _seen=mb_rewards, _orig=orig_step):
            _seen.setdefault(i, (inputs[2], inputs[2].clone()))        # the minibatch's rewards as the epoch built them
            return _orig(self, i, inputs, fn)
        monkeypatch.setattr(_UpdateGraphs, "step", step)
        stats = []
        for ep in range(2):
            mb_rewards.clear()
            _epoch(torch, algo, z, monkeypatch, ref_baselines=False)        # (the critic has trained: its own baselines)
            stats.append(dict(algo.stats))
            if tag == "graph":
                ug = algo._update_graphs
                assert not ug.broken and ug.captured == 3, (ug.captured, ug.reused)
                assert ug.reused == 3 * ep                              # epoch 2: every minibatch takes epoch 1's graph
                assert len(mb_rewards) == 3 and len(ug.cache) == 3
                snaps = [snap for _, snap in mb_rewards.values()]
                for src, snap in mb_rewards.values():
                    assert torch.equal(src, snap)
                for ent in ug.cache.values():                           # the captured step's own rewards buffer after 2-3 replays
                    assert any(torch.equal(ent[2][2], snap) for snap in snaps)
        monkeypatch.setattr(_UpdateGraphs, "step", orig_step)
        runs[tag] = dict(pol={k: v.detach().cpu().numpy() for k, v in pol.state_dict().items()},
                         crit={k: v.detach().cpu().numpy() for k, v in crit.state_dict().items()}, stats=stats)

    def dev(a, b):
        return max(float(np.abs(a[k] - b[k]).max()) for k in a)
    noise = max(dev(runs["eager"]["pol"], runs["eager2"]["pol"]), dev(runs["eager"]["crit"], runs["eager2"]["crit"]))
    got = max(dev(runs["eager"]["pol"], runs["graph"]["pol"]), dev(runs["eager"]["crit"], runs["graph"]["crit"]))
    print(f"max: |graph - eager| = {got:.3e}, |eager - eager| = {noise:.3e}")
    assert got <= max(4 * noise, 1e-4)
    for a, b in zip(runs["eager"]["stats"], runs["graph"]["stats"]):
        for k in ("LossBefore", "LossAfter", "KL", "Entropy"):
            np.testing.assert_allclose(a[k], b[k], rtol=2e-3, atol=2e-5, err_msg=k)


@pytest.mark.gpu
def test_runner_shaped_training_script_max_entropy():
    """The runner_pp_commDP.py body (tests/test_dropin.py) with --entropy_method max --center_adv 0: the runner passes
    stop_entropy_gradient=True exactly then (:133-135); two epochs train and log a finite Entropy."""
    import torch
    assert torch.cuda.is_available()
    import com_marl_amd.dropin as dropin
    from tests.test_dropin import _args
    dropin.install(force=True)
    from envs import PredatorPreyWrapper
    from com_marl.torch.policies import CommCategoricalMLPPolicy
    from com_marl.torch.baselines import CommBaseCritic
    from com_marl.torch.algos import CentralizedMAPPO
    from com_marl.sampler import CentralizedMAOnPolicyVectorizedSampler
    args = SimpleNamespace(**dict(vars(_args()), entropy_method="max", center_adv=0))
    env = PredatorPreyWrapper(centralized=True, grid_shape=(args.grid_size, args.grid_size), n_agents=args.n_agents,
                              n_preys=args.n_preys, max_steps=args.max_env_steps, step_cost=args.step_cost,
                              prey_capture_reward=args.capture_reward, penalty=args.penalty,
                              other_agent_visible=bool(args.agent_visible), params=vars(args),
                              n_envs=args.n_envs, device=args.device)
    policy = CommCategoricalMLPPolicy(env.spec, n_agents=args.n_agents, encoder_hidden_sizes=args.encoder_hidden_sizes,
                                      embedding_dim=args.embedding_dim, attention_type=args.attention_type,
                                      n_gcn_layers=args.n_gcn_layers, residual=bool(args.residual),
                                      gcn_bias=bool(args.gcn_bias),
                                      categorical_mlp_hidden_sizes=args.categorical_mlp_hidden_sizes,
                                      name='comm_categorical_mlp_policy', device=args.device)
    baseline = CommBaseCritic(env.spec, n_agents=args.n_agents, encoder_hidden_sizes=args.encoder_hidden_sizes,
                              embedding_dim=args.embedding_dim, attention_type=args.attention_type,
                              n_gcn_layers=args.n_gcn_layers, residual=bool(args.residual), gcn_bias=bool(args.gcn_bias),
                              aggregator_type=args.aggregator_type, device=args.device)
    algo = CentralizedMAPPO(env_spec=env.spec, policy=policy, baseline=baseline, max_path_length=args.max_env_steps,
                            discount=args.discount, center_adv=bool(args.center_adv),
                            positive_adv=bool(args.positive_adv), gae_lambda=args.gae_lambda,
                            policy_ent_coeff=args.ent, entropy_method=args.entropy_method,
                            stop_entropy_gradient=True if args.entropy_method == 'max' else False,
                            clip_grad_norm=args.clip_grad_norm, optimization_n_minibatches=args.opt_n_minibatches,
                            optimization_mini_epochs=args.opt_mini_epochs, device=args.device)
    runner = dropin.SimpleRunner()
    runner.setup(algo, env, sampler_cls=CentralizedMAOnPolicyVectorizedSampler, sampler_args={'n_envs': args.n_envs})
    ret = runner.train(n_epochs=args.n_epochs, batch_size=args.bs)
    assert np.isfinite(ret) and len(runner.history) == 2
    for h in runner.history:
        assert np.isfinite(h["Entropy"]) and 0 < h["Entropy"] <= np.log(5) + 1e-6
        assert np.isfinite(h["LossBefore"]) and np.isfinite(h["LossAfter"])
