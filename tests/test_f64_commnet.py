"""Pin of the float64 restatement (tests/f64_commnet.py) to the reference's own recordings, before it judges any kernel:
every Comm-DP quantity the fixtures hold - probabilities, attention, entropy, log-likelihood, values and critic loss of
policy_*.npz; scalar, critic loss and every parameter gradient of net_options_*.npz and net_grads_*.npz - to within 1e-5 of
that tensor's own largest entry (no floor at 1).  CPU only: the restatement is plain torch."""
import glob
import os

import numpy as np
import pytest
import torch

from tests import f64_commnet as R
from tests.test_oracle_golden import GOLDEN

TAU = 1e-5


def _sd(z, pre):
    k0 = pre + "."
    return {k[len(k0):]: z[k] for k in z.files if k.startswith(k0)}


def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=R.F64)


def _n_agents(z, pre):
    return z["adj"].shape[-1]


def _check(name, got, want, worst):
    r = R.ratio(got, want)
    worst[name] = r
    assert r <= TAU, f"{name}: max|f64 - reference| = {r:.3g} of the tensor's scale"


def _policy_fixtures():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "policy_*.npz")))


def _grad_fixtures():
    out = []
    for p in sorted(glob.glob(os.path.join(GOLDEN, "net_options_*.npz"))):
        out += [(os.path.basename(p)[:-4], tag) for tag in ("dot", "direct")]
    out += [(os.path.basename(p)[:-4], "") for p in sorted(glob.glob(os.path.join(GOLDEN, "net_grads_*.npz")))]
    return out


def test_fixture_sets_are_present():
    assert len(_policy_fixtures()) == 7
    assert len([n for n, _ in _grad_fixtures() if n.startswith("net_grads_")]) == 5


@pytest.mark.parametrize("name", _policy_fixtures())
def test_restatement_matches_policy_fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    N = _n_agents(z, "pol")
    residual = bool(int(z["residual"])) if "residual" in z.files else True       # (older recordings: the default)
    pol, crit = R.params(_sd(z, "pol"), requires_grad=False), R.params(_sd(z, "crit"), requires_grad=False)
    obs, adj, ch = _t(z["obs"]), _t(z["adj"]), _t(z["channels"])
    S = obs.shape[0]
    acts = torch.as_tensor(z["actions"])
    worst = {}
    with torch.no_grad():
        for tag, av in (("", None), ("_masked", _t(z["avail_masked"]))):
            _, probs, attn = R.policy_forward(pol, obs, av, adj, ch, N, residual)
            _check("probs" + tag, probs, z["probs" + tag], worst)
            _check("attn" + tag, attn, z["attn" + tag], worst)
        _, probs, _ = R.policy_forward(pol, obs, None, adj, ch, N, residual)
        _check("entropy", R.entropy(probs), z["entropy"], worst)
        _check("loglik", R.loglik(probs, acts), z["loglik"], worst)
        values = R.critic_values(crit, obs, adj, ch, N, residual)
        _check("values", values, z["values"], worst)
        loss = R.critic_nll(values, R.critic_std(crit), _t(z["returns"]))
        _check("critic_loss", loss, z["critic_loss"], worst)
    assert S == z["probs"].shape[0]
    print(f"{name}: worst ratio {max(worst.values()):.2e} ({max(worst, key=worst.get)})")


@pytest.mark.parametrize("name,tag", _grad_fixtures())
def test_restatement_matches_recorded_gradients(name, tag):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    N = _n_agents(z, "pol")
    k = (tag + ".") if tag else ""
    pol, crit = R.params(_sd(z, k + "pol")), R.params(_sd(z, k + "crit"))
    obs, adj, ch = _t(z["obs"]), _t(z["adj"]), _t(z["channels"])
    avail = _t(z["avail"]) if "avail" in z.files else None
    worst = {}
    _, probs, attn = R.policy_forward(pol, obs, avail, adj, ch, N)
    if k + "probs" in z.files:
        _check("probs", probs, z[k + "probs"], worst)
        _check("attn", attn, z[k + "attn"], worst)
    scalar = R.ppo_scalar(probs, torch.as_tensor(z["actions"]), _t(z["weights"]))
    scalar.backward()
    values = R.critic_values(crit, obs, adj, ch, N)
    _check("values", values, z[k + "values"], worst)
    loss = R.critic_nll(values, R.critic_std(crit), _t(z["returns"]))
    loss.backward()
    _check("scalar", scalar, z[k + "scalar"], worst)
    _check("critic_loss", loss, z[k + "critic_loss"], worst)
    n = 0
    for pre, net in (("gpol", pol), ("gcrit", crit)):
        for pname, p in net.items():
            want = z[f"{k}{pre}.{pname}"]
            got = torch.zeros_like(p) if p.grad is None else p.grad
            _check(f"{pre}.{pname}", got, want, worst)
            n += 1
    assert n == len([f for f in z.files if f.startswith(k + "gpol.") or f.startswith(k + "gcrit.")])
    print(f"{name}{'.' + tag if tag else ''}: {n} gradients, worst ratio {max(worst.values()):.2e} ({max(worst, key=worst.get)})")
