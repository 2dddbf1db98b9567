"""What the tests of Comm-DP nets with non-default layer sizes share (no test in here): the three shapes, our nets built at
them with the reference's recorded weights (A, B) or seeded ones (C), and random inputs with the awkward masks.

  A  N = 4,  d = 21   encoder (96, 48)  embedding 32  head (48, 24)          2 hops            shapes_net_grads_pp_map10.npz
  B  N = 24, d = 77   encoder (96, 48)  embedding 32  head (48, 24)          2 hops            shapes_net_grads_co_map20.npz
  C  N = 5,  d = 21   encoder (40,)     embedding 16  head (100, 20, 12, 8)  1 hop, 'dot', no residual, no GCN bias; seeded

Two encoder layers, ragged widths (no multiple of 16), a width below one MFMA tile, every head depth between them and the
too-large shape, 'dot', no residual, teams that do not divide a 16-row tile."""
import os

import numpy as np

from tests.test_oracle_golden import GOLDEN

SIZES = dict(encoder_hidden_sizes=(96, 48), embedding_dim=32)
HEAD = (48, 24)
SHAPES = {
    "A": dict(N=4, d=21, hops=2, fixture="shapes_net_grads_pp_map10", pol=dict(SIZES, categorical_mlp_hidden_sizes=HEAD), crit=SIZES),
    "B": dict(N=24, d=77, hops=2, fixture="shapes_net_grads_co_map20", pol=dict(SIZES, categorical_mlp_hidden_sizes=HEAD), crit=SIZES),
    "C": dict(N=5, d=21, hops=1, fixture=None,
              pol=dict(encoder_hidden_sizes=(40,), embedding_dim=16, categorical_mlp_hidden_sizes=(100, 20, 12, 8),
                       attention_type="dot", residual=False, gcn_bias=False, n_gcn_layers=1), crit=None),
}
N_ENVS = 37            # the last workgroup of every shape is ragged (12, 2 and 9 envs per workgroup)


def fixture(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def sd_of(z, pre):
    k0 = pre + "."
    return {k[len(k0):]: z[k] for k in z.files if k.startswith(k0)}


def spec_of(N, d):
    from com_marl_amd.envs import EnvSpec, _Box, _Discrete
    return EnvSpec(_Box(np.zeros(d * N), np.ones(d * N)), _Discrete(5))


def build(shape, device="cuda:0", critic=True):
    """-> (policy, critic | None) of ours at `shape`, the recorded reference weights loaded by name (strict) for A and B."""
    import torch
    from com_marl_amd import nets
    s = SHAPES[shape]
    spec = spec_of(s["N"], s["d"])
    torch.manual_seed(1234)
    pol = nets.CommCategoricalMLPPolicy(spec, n_agents=s["N"], device=device, **s["pol"])
    crit = nets.CommBaseCritic(spec, n_agents=s["N"], device=device, **s["crit"]) if (critic and s["crit"] is not None) else None
    if s["fixture"]:
        z = fixture(s["fixture"])
        pol.load_state_dict({k: torch.as_tensor(v) for k, v in sd_of(z, "pol").items()}, strict=True)
        if crit is not None:
            crit.load_state_dict({k: torch.as_tensor(v) for k, v in sd_of(z, "crit").items()}, strict=True)
    else:
        with torch.no_grad():
            for name, p in pol.named_parameters():
                if name.endswith("bias"):
                    p.uniform_(-0.1, 0.1)
    return pol, crit


def inputs(N, d, hops, S=N_ENVS, seed=0, A=5):
    """obs [S,N*d], avail [S,N,A], adj [S,N,N], channels [S,hops,N,N] (numpy f32): random links, one agent (env 1, agent N-1) whose
    masked row sums to zero, action 1 forbidden for ~30 % of the agents."""
    rng = np.random.RandomState(1000 + seed + 7 * N)
    obs = rng.rand(S, N * d).astype(np.float32)
    adj = (rng.rand(S, N, N) < 0.7).astype(np.float32)
    ch = (rng.rand(S, max(hops, 1), N, N) < 0.7).astype(np.float32)
    idx = np.arange(N)
    adj[:, idx, idx] = 1.0
    ch[:, :, idx, idx] = 1.0
    adj[1, N - 1, :] = 0.0
    avail = np.ones((S, N, A), np.float32)
    avail[rng.rand(S, N) < 0.3, 1] = 0.0
    return obs, avail, adj, ch[:, :hops] if hops else None
