"""What params['calc_diameter'] costs on one MI355X: the ONE cm_graph_diameter launch behind a 50-step chunk
(51 slots of dist_adj, as the engine holds them after that chunk) beside the time of the chunk itself with the switch off, at
  PP map 10, N = 4, 4096 envs, range 2     (4096 x 51 graphs)
  PP map 30, N = 72, 1024 envs, range 5    (1024 x 51 graphs).
The launch: 200 calls between two HIP events after 20 warm-ups; the chunk: 20 run_chunk calls (hipGraph replay where the engine
captures one) after 3 warm-ups; three rounds each.  `python tools/diameter_time.py [map10|map30]`, no argument both."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from com_marl_amd import envs as E, nets  # noqa: E402
from com_marl_amd.rollout import RolloutEngine  # noqa: E402

H, CALLS, WARM, CHUNKS, ROUNDS = 50, 200, 20, 20, 3
CASES = {
    "map10": (4096, dict(load=2, max_env_steps=200, capture_reward=10, step_cost=0.1, rm=0, penalty=0, grid_size=10, Rsen=1,
                         n_agents=4, n_preys=4, n_gcn_layers=2, mode="train", trRcom=2, trpl=0)),
    "map30": (1024, dict(load=4, max_env_steps=200, capture_reward=10, step_cost=0.1, rm=0, penalty=0, grid_size=30, Rsen=2,
                         n_agents=72, n_preys=72, n_gcn_layers=2, mode="train", trRcom=5, trpl=0)),
}


def timed(fn, warm, calls):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls                      # us per call


def main(name):
    B, params = CASES[name]
    env = E.GridEnvBatch("pp", params, B, device="cuda:0", seed=3)   # no calc_diameter: the chunk below is today's
    N = env.N
    spec = E.EnvSpec(E._Box(np.zeros(N * env.d), np.ones(N * env.d)), E._Discrete(5))
    torch.manual_seed(0)
    pol = nets.CommCategoricalMLPPolicy(spec, n_agents=N, device="cuda:0")
    pol.set_rng(3)
    eng = RolloutEngine(env, pol, H)
    assert eng.dist_adj is not None and eng.diameter is None
    eng.reset()
    out = torch.empty(H + 1, B, dtype=torch.int32, device="cuda:0")
    for rnd in range(ROUNDS):
        chunk = timed(lambda: eng.run_chunk(weights_synced=True), 3, CHUNKS)
        launch = timed(lambda: E.graph_diameter(eng.dist_adj, out=out), WARM, CALLS)
        d = out.cpu().numpy()
        print(f"[{rnd}] pp_{name} N={N} {B} envs x {H + 1} slots: cm_graph_diameter {launch:8.1f} us, {H}-step chunk {chunk:9.1f} us "
              f"({100.0 * launch / chunk:.2f} % of the chunk); connected {100.0 * (d > 0).mean():.0f} %, largest {d.max()}", flush=True)
    env.check_status()


if __name__ == "__main__":
    for which in (sys.argv[1:] or list(CASES)):
        main(which)
