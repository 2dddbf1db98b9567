"""Per-step time of the acting forward of Comm-DP policies with non-default layer sizes on one MI355X: ONE
launch of the run-time-sized kernel (cm_policy_forward_any) against the layer-by-layer route of the same build, in the same run.

  shape A   N = 4,  d = 21, encoder (96, 48), embedding 32, head (48, 24), 4096 envs
  shape B   N = 24, d = 77, the same sizes, 1024 envs
  default   N = 4,  d = 21, 128 | 64 | 128, 64, 32, 4096 envs: cm_policy_forward against _act_device_layers, for scale

Each figure is REPS back-to-back act_device calls (forward + softmax x avail + sample, outputs into fixed buffers) between
two HIP events after WARM warm-up calls, eagerly launched - the layer route therefore includes the host time of its dozen
launches, which is what it costs a rollout that is not replayed from a hipGraph.  The two routes alternate and the list is
run ROUNDS times, so the spread between rounds is visible next to the difference between routes.  The routes' probabilities
are compared first (largest difference printed).  Needs the GPU; `python tools/any_shape_time.py`."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from com_marl_amd import envs as E, nets  # noqa: E402

WARM, REPS, ROUNDS = 20, 200, 3
SIZES = dict(encoder_hidden_sizes=(96, 48), embedding_dim=32, categorical_mlp_hidden_sizes=(48, 24))
CASES = [("A", 4, 21, 4096, SIZES), ("B", 24, 77, 1024, SIZES), ("default", 4, 21, 4096, {})]


def make(N, d, S, kw):
    spec = E.EnvSpec(E._Box(np.zeros(N * d), np.ones(N * d)), E._Discrete(5))
    torch.manual_seed(0)
    pol = nets.CommCategoricalMLPPolicy(spec, n_agents=N, device="cuda:0", **kw)
    pol.set_rng(3)
    g = torch.Generator().manual_seed(1)
    obs = torch.rand(S, N * d, generator=g).cuda()
    adj = (torch.rand(S, N, N, generator=g) < 0.7).float()
    ch = (torch.rand(S, 2, N, N, generator=g) < 0.7).float()
    adj[:, range(N), range(N)] = 1.0
    ch[:, :, range(N), range(N)] = 1.0
    bufs = (torch.empty(S, N, dtype=torch.int32, device="cuda:0"), torch.empty(S, N, 5, device="cuda:0"),
            torch.empty(S, N, N, device="cuda:0"))
    return pol, obs, adj.cuda(), ch.cuda(), bufs


def call(pol, route, obs, adj, ch, bufs, step):
    a, p, m = bufs
    if pol._default_shape and route == "layers":
        with torch.no_grad():
            return pol._act_device_layers(obs, None, adj, ch, False, a, p, m, step, None, None)
    pol._general_forward = route
    return pol.act_device(obs, None, adj, ch, out_actions=a, out_probs=p, out_attn=m, policy_step=step)


def step_us(pol, route, obs, adj, ch, bufs):
    for t in range(WARM):
        call(pol, route, obs, adj, ch, bufs, t)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for t in range(REPS):
        call(pol, route, obs, adj, ch, bufs, t)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / REPS


def main():
    if not torch.cuda.is_available():
        sys.exit("any_shape_time.py measures on the MI355X: no GPU found")
    print(f"{'shape':8s} {'envs':>5s} {'route':>10s} " + " ".join(f"{'round ' + str(r):>10s}" for r in range(ROUNDS)) + "   us per step")
    for name, N, d, S, kw in CASES:
        pol, obs, adj, ch, bufs = make(N, d, S, kw)
        pol.sync_weights()
        probs = {}
        for route in ("auto", "layers"):
            probs[route] = call(pol, route, obs, adj, ch, bufs, 0)[1].clone()
        print(f"{name:8s} routes agree to {float((probs['auto'] - probs['layers']).abs().max()):.1e} on the probabilities")
        times = {"auto": [], "layers": []}
        for _ in range(ROUNDS):
            for route in ("auto", "layers"):
                times[route].append(step_us(pol, route, obs, adj, ch, bufs))
        for route, label in (("auto", "one launch"), ("layers", "layers")):
            print(f"{name:8s} {S:5d} {label:>10s} " + " ".join(f"{t:10.1f}" for t in times[route]))


if __name__ == "__main__":
    main()
