"""Time of what Comm-DP nets with non-default layer sizes gained on one MI355X, each new route against the route
it replaces, of the same build, in the same run:

  (a) the critic's no-grad forward: ONE launch (cm_critic_forward_any) against layer by layer (_general_forward = "layers")
        shape A   N = 4,  d = 21, encoder (96, 48), embedding 32, decoder (64,), 4096 envs
        shape B   N = 24, d = 77, the same sizes, 1024 envs
  (b) one training forward + backward of the policy (a fixed projection of _probs), attention and masked aggregation on the
      any-width HIP ops (nets.graph_op_route = "hip") against the framework's batched GEMMs with autograd ("framework")
        shape A at 8192 envs, shape B at 1024 envs; head (48, 24)

Each figure is REPS back-to-back eager calls between two HIP events after WARM warm-up calls, so it includes the host time of
the launches - what an update that is not replayed from a hipGraph pays (these nets step eagerly).  The two routes alternate
and the list is run ROUNDS times, so the spread between rounds is visible next to the difference between routes.  The
routes' outputs are compared first (largest difference printed).  Needs the GPU; `python tools/any_width_time.py`."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from com_marl_amd import envs as E, nets  # noqa: E402

WARM, REPS, ROUNDS = 20, 200, 3
SIZES = dict(encoder_hidden_sizes=(96, 48), embedding_dim=32)
HEAD = (48, 24)
CRITIC_CASES = [("A", 4, 21, 4096), ("B", 24, 77, 1024)]
TRAIN_CASES = [("A", 4, 21, 8192), ("B", 24, 77, 1024)]


def inputs(N, d, S):
    g = torch.Generator().manual_seed(1)
    obs = torch.rand(S, N * d, generator=g).cuda()
    adj = (torch.rand(S, N, N, generator=g) < 0.7).float()
    ch = (torch.rand(S, 2, N, N, generator=g) < 0.7).float()
    adj[:, range(N), range(N)] = 1.0
    ch[:, :, range(N), range(N)] = 1.0
    return obs, adj.cuda(), ch.cuda()


def spec(N, d):
    return E.EnvSpec(E._Box(np.zeros(N * d), np.ones(N * d)), E._Discrete(5))


def timed_us(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / REPS


def report(name, S, what, routes, run, agree):
    """routes: (route, label) pairs, the new one first.  run(route) -> a callable for the timed loop."""
    print(f"{name:8s} {what}: routes agree to {agree:.1e}")
    times = {r: [] for r, _ in routes}
    for _ in range(ROUNDS):
        for r, _ in routes:
            times[r].append(timed_us(run(r)))
    for r, label in routes:
        t = times[r]
        print(f"{name:8s} {S:5d} {label:>10s} " + " ".join(f"{x:10.1f}" for x in t) + f"   median {sorted(t)[1]:8.1f}  spread {max(t) - min(t):6.1f}")


def critic(name, N, d, S):
    torch.manual_seed(0)
    crit = nets.CommBaseCritic(spec(N, d), n_agents=N, device="cuda:0", **SIZES)
    crit.sync_weights()
    obs, adj, ch = inputs(N, d, S)
    out = torch.empty(S, device="cuda:0")

    def run(route):
        def fn():
            crit._general_forward = route
            crit.values_device(obs, adj, ch, out=out)
        return fn
    vals = {}
    for route, took in (("auto", "one_launch"), ("layers", "layers")):
        run(route)()
        assert crit._last_forward == took, (route, crit._last_forward)
        vals[route] = out.clone()
    report(name, S, "critic forward", (("auto", "one launch"), ("layers", "layers")), run, float((vals["auto"] - vals["layers"]).abs().max()))
    crit._general_forward = "auto"


def train(name, N, d, S):
    torch.manual_seed(0)
    pol = nets.CommCategoricalMLPPolicy(spec(N, d), n_agents=N, device="cuda:0", categorical_mlp_hidden_sizes=HEAD, **SIZES)
    obs, adj, ch = inputs(N, d, S)
    w = torch.randn(S, N, 5, generator=torch.Generator().manual_seed(2)).cuda()
    Em = SIZES["embedding_dim"]

    def run(route):
        def fn():
            nets.set_graph_op_route(N, Em, route)
            pol.zero_grad(set_to_none=False)
            (pol._probs(obs, None, adj, ch)[0] * w).sum().backward()
        return fn
    grads = {}
    for route in ("hip", "framework"):
        pol.zero_grad()
        run(route)()
        grads[route] = torch.cat([p.grad.reshape(-1) for p in pol.parameters()]).clone()
    scale = float(grads["framework"].abs().max())
    report(name, S, "policy forward + backward", (("hip", "hip ops"), ("framework", "framework")), run,
           float((grads["hip"] - grads["framework"]).abs().max()) / max(scale, 1e-30))
    nets.set_graph_op_route(N, Em, None)


def main():
    if not torch.cuda.is_available():
        sys.exit("any_width_time.py measures on the MI355X: no GPU found")
    print(f"{'shape':8s} {'envs':>5s} {'route':>10s} " + " ".join(f"{'round ' + str(r):>10s}" for r in range(ROUNDS)) + "   us per call")
    for c in CRITIC_CASES:
        critic(*c)
    for c in TRAIN_CASES:
        train(*c)


if __name__ == "__main__":
    main()
