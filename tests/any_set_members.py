"""What the tests of policy sets with mixed Comm-DP layer sizes share (no test in here): the three member families, built at a
case's (N, d, hops) with seeded weights and perturbed biases (as any_shapes.build("C") does), and the planner's arithmetic.

  m0  encoder (96, 48)     embedding 32   head (48, 24)           'general', residual
  m1  encoder (40,)        embedding 16   head (100, 20, 12, 8)   'dot', no residual, no GCN bias
  m2  encoder (8, 128, 24) embedding 128  head (5,)               'general', residual: the widest plane, ragged widths, a width
                                                                  below one MFMA tile"""
import numpy as np

FAMILIES = {
    "m0": dict(encoder_hidden_sizes=(96, 48), embedding_dim=32, categorical_mlp_hidden_sizes=(48, 24), attention_type="general"),
    "m1": dict(encoder_hidden_sizes=(40,), embedding_dim=16, categorical_mlp_hidden_sizes=(100, 20, 12, 8), attention_type="dot",
               residual=False, gcn_bias=False),
    "m2": dict(encoder_hidden_sizes=(8, 128, 24), embedding_dim=128, categorical_mlp_hidden_sizes=(5,), attention_type="general"),
}
LDS_LIMIT = 160 * 1024


def pad16(x):
    return (x + 15) & ~15


def epb_of(N):
    """Envs per workgroup of the run-time-sized forward (csrc/cm_policy_g_dev.h plan())."""
    return max(1, 48 // N)


def plan(N, d, family):
    """(SE, SW, LDS bytes) of one member by plan()."""
    f = FAMILIES[family]
    emb = f["embedding_dim"]
    widest = max((emb,) + tuple(f["encoder_hidden_sizes"]) + tuple(f["categorical_mlp_hidden_sizes"]))
    epb = epb_of(N)
    R16, SE, SW, NP = pad16(epb * N), pad16(emb) + 4, pad16(max(widest, d)) + 4, N | 1
    mat = (epb * N * NP + 3) & ~3
    return SE, SW, (R16 * (2 * SE + 2 * SW) + 2 * mat) * 4


def build(family, N, d, hops, seed, device="cuda:0", rng_seed=11):
    """One member: seeded weights (`seed`: members of one family differ in it), biases perturbed away from zero."""
    import torch
    from com_marl_amd import nets
    from tests.any_shapes import spec_of
    torch.manual_seed(seed)
    pol = nets.CommCategoricalMLPPolicy(spec_of(N, d), n_agents=N, n_gcn_layers=hops, device=device, **FAMILIES[family])
    with torch.no_grad():
        for name, p in pol.named_parameters():
            if name.endswith("bias"):
                p.uniform_(-0.1, 0.1)
    pol.set_rng(rng_seed)
    return pol


def build_default(N, d, hops, seed, device="cuda:0", rng_seed=11):
    """A member of the default layer sizes (128 | 64 | 128, 64, 32)."""
    import torch
    from com_marl_amd import nets
    from tests.any_shapes import spec_of
    torch.manual_seed(seed)
    pol = nets.CommCategoricalMLPPolicy(spec_of(N, d), n_agents=N, n_gcn_layers=hops, device=device)
    pol.set_rng(rng_seed)
    return pol


def net_struct(family, N, d, hops, n_act=5, fake=0x1000):
    """cm_net_weights of a family with fake non-null pointers (the planner never dereferences them)."""
    from com_marl_amd import _lib
    f = FAMILIES[family]
    w = _lib.NetWeights()
    w.d, w.n_agents, w.n_hops, w.n_act = d, N, hops, n_act
    w.no_residual, w.emb = 0 if f.get("residual", True) else 1, f["embedding_dim"]
    enc, head = f["encoder_hidden_sizes"], f["categorical_mlp_hidden_sizes"]
    w.n_enc, w.n_head = len(enc), len(head)
    for i, h in enumerate(enc):
        w.enc_hidden[i] = h
    for i, h in enumerate(head):
        w.head_hidden[i] = h
    for i in range(len(enc) + 1):
        w.enc_wt[i], w.enc_b[i] = fake + 16 * i, fake + 0x100 + 16 * i
    for i in range(len(head) + 1):
        w.head_wt[i], w.head_b[i] = fake + 0x200 + 16 * i, fake + 0x300 + 16 * i
    w.attn_wt = fake + 0x400 if f["attention_type"] == "general" else None
    w.gcn_w = fake + 0x500
    w.gcn_b = fake + 0x600 if f.get("gcn_bias", True) else None
    return w


def guarded(torch, shape, dtype, fill, guard=64):
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * guard,), fill, dtype=dtype, device="cuda:0")
    return flat, flat[guard:guard + n].view(*shape)
