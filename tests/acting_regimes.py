"""What the tests of the acting forward in the trained-policy regime share (no test in here, no GPU, nothing of com_marl_amd):

  REGIMES          per-layer factors over a reference-named state_dict that move a freshly initialised net - max |logit| 0.7,
                   no probability above 0.5 - to where a policy sits after a few hundred PPO epochs: logits in the tens,
                   probabilities within 1e-7 of 1 or exactly 0 after the `avail` mask, saturated tanh units, peaked attention
  apply            the scaled weights as float32 arrays: what the kernels load and what the float64 judge starts from
  split2_forward   the arithmetic scheme of the matrix-core kernels alone (cm_policy_h_dev.h: every dense-layer operand carried as
                   f16(x) + f16(x - f16(x))) with exact accumulation: what a correct kernel may lose before any f32 rounding
  inputs           observations and masks of one case, shared by the CPU test (is the input fair?) and the GPU test (the kernel)
  uniforms ..      the action sampler's Philox uniforms, its inverse-CDF rule in float64 and the draws too close to a boundary
                   of that CDF for a 1e-5 error per probability to leave them decided

Emulated ratios (max|x - f64| / max|f64|) of split2_forward - the worst of logits, probabilities and attention - and of a
float32 restatement - the lowest and highest of the three - on the recorded weights of policy_pp_map10 / policy_co_map20 at the GPU
test's inputs (tests/test_acting_regimes_cpu.py prints every row, also for policy_pp_map10_hops1_nores and policy_co_map30_iid):

  regime         scales                  max |logit|   rows p > .99   |a1| > .99    split2            float32
  init           none                    0.7 / 1.2     0              0             4.9e-7 / 4.8e-7   8e-8 .. 5e-7
  head12         HO x12                  8.6 / 14.0    0 / .18        0             1.0e-6 / 1.6e-6   2e-7 .. 1.4e-6
  head40         HO x40                  29 / 47       .38 / .56      0             4.5e-6 / 4.5e-6   2e-7 .. 4.0e-6
  enc14          E0 x14, E1 x14          1.6 / 1.8     0              .30 / .61     1.5e-6 / 1.6e-6   3e-7 .. 1.9e-6
  enc14_head12   E0 x14, E1 x14, HO x12  19 / 21       .43 / .40      .30 / .61     2.9e-6 / 1.9e-6   7e-7 .. 4.5e-6
  attn12         AT x12                  0.7 / 1.2     0              0             6.5e-7 / 1.6e-6   1e-7 .. 2.0e-6
  shift4         E0 x2^-4, E1 x2^4       1.1 / 0.9     0              0             1.6e-6 / 3.0e-6   1e-7 .. 1.6e-6
  (shift6        E0 x2^-6, E1 x2^6                                                  5.2e-6 / 5.2e-6   2e-7 .. 2.1e-6    not asserted)
  (shift10       E0 x2^-10, E1 x2^10                                                3.4e-5 / 4.6e-5   3e-7 .. 1.5e-5    not asserted)

The encoder factor is 14, not 6: at 6 only 1.4 % of the encoder's hidden units of policy_pp_map10 sit above 0.99 (17 % .. 25 % on the
larger observations), at 14 it is 30 % .. 61 %.  The worst split2 ratio over the four fixtures, seven regimes and three mask
settings is 4.5e-6 (head40, probabilities): inside the 5e-6 the CPU test asserts - half the project's 1e-5 bar - so no
(fixture, regime) pair is dropped for that.  Two are dropped because the regime does not take hold: on policy_pp_map10_hops1_nores (the head sees
H_1 alone) head12 / head40 leave max |logit| at 3 / 11 and at most 5 % of the rows above 0.99; enc14_head12 (14, 30 %) stays.  shift6 / shift10 (same inputs, same emulation) run into the split's absolute floor
of 2^-25 per operand, small weights times large ones: a property of the scheme, stated where its bound is documented, not a regime a
kernel is held to."""
import functools

import numpy as np
import torch

from tests import f64_commnet as R

F64 = torch.float64

HO = "categorical_output_layer._output_layers.0.linear.weight"
E0 = "encoder._layers.0.linear.weight"
E1 = "encoder._output_layers.0.linear.weight"
AT = "attention_layer.linear_in.weight"

# the asserted regimes: {parameter name: factor}.  Trunk names are those of policy and critic alike; HO exists in the policy only.
REGIMES = {
    "init": {},
    "head12": {HO: 12.0},
    "head40": {HO: 40.0},
    "enc14": {E0: 14.0, E1: 14.0},
    "enc14_head12": {E0: 14.0, E1: 14.0, HO: 12.0},
    "attn12": {AT: 12.0},
    "shift4": {E0: 2.0 ** -4, E1: 2.0 ** 4},
}
PEAKED = ("head40", "enc14_head12")          # the two every route runs
CRITIC_REGIMES = ("init", "enc14", "attn12", "shift4")

# the sampler's stream in every case of the GPU test (and of the fairness condition of the CPU test)
SEED, ENV_ID_OFFSET, POLICY_STEP = 0x5DEECE66D, 1000, 5
DELTA = 5e-5                                # five actions times the 1e-5 bar on each probability
GREEDY_GAP = 2e-5                           # top-two probabilities closer than this: the argmax is not decided at 1e-5 each
MAX_EXCLUDED = 0.01
MASKS = ("none", "links", "avail")


def apply(sd, regime):
    """state_dict (numpy or torch values) -> {name: float32 array}, the regime's factors applied in float32."""
    f = REGIMES[regime] if isinstance(regime, str) else regime
    out = {}
    for k, v in sd.items():
        a = np.asarray(v.detach().cpu() if torch.is_tensor(v) else v)
        if a.dtype.kind == "f":
            a = (a.astype(np.float32) * np.float32(f.get(k, 1.0))).astype(np.float32)
        out[k] = a
    return out


def split2(x):
    """cm_policy_h_dev.h: hi = f16(x), lo = f16(x - hi); the operand the matrix pipe sees is hi + lo."""
    hi = x.to(torch.float16).to(F64)
    lo = (x - hi).to(torch.float16).to(F64)
    return hi + lo


def _dense(x, w_out_in, b, tanh):
    y = split2(x) @ split2(w_out_in).T
    if b is not None:
        y = y + b
    return torch.tanh(y) if tanh else y


def split2_forward(p, obs, adj, ch, N, residual=True, avail=None):
    """Emulation of the split-f16 kernels' arithmetic scheme: f64_commnet's forward with both operands of every dense layer
    (encoder, linear_in, the scores, H W, the head) rounded by split2 and the products accumulated exactly (float64); softmax,
    the masked aggregation (f32 attention weights in the kernels) and everything else as in the restatement.  The product
    (hi + lo)(hi' + lo') is taken whole, the lo.lo' term included, which the kernels drop: 2^-22 relative per product, below what
    the 5e-6 condition can see - the emulation is a lower bound of the scheme's loss, not the scheme to the bit.
    p: float64 tensors (R.params).  -> (logits, probs, attention)."""
    obs, adj, ch = R.as_batch(obs, adj, ch, N, R.n_hops(p))
    a1 = _dense(obs, p[E0], p["encoder._layers.0.linear.bias"], True)
    e = _dense(a1, p[E1], p["encoder._output_layers.0.linear.bias"], True)
    q = _dense(e, p[AT], None, False) if AT in p else e
    m = torch.softmax(split2(q) @ split2(e).transpose(-2, -1), dim=-1)
    h = e
    for l in range(R.n_hops(p)):
        hw = split2(h) @ split2(p[f"gcn_layers.{l}.weight"])
        h = R.aggregate(m, adj, None if ch is None else ch[:, l], hw, p.get(f"gcn_layers.{l}.bias"))
    x = e + h if residual else h
    pre = "categorical_output_layer."
    for i in range(R.n_hidden(p, pre)):
        x = _dense(x, p[f"{pre}_layers.{i}.linear.weight"], p[f"{pre}_layers.{i}.linear.bias"], True)
    logits = _dense(x, p[f"{pre}_output_layers.0.linear.weight"], p[f"{pre}_output_layers.0.linear.bias"], False)
    return logits, R.masked_probs(logits, avail), m


def f32_forward(sd32, obs, avail, adj, ch, N, residual=True):
    """The restatement itself run in float32 (torch CPU): the noise floor a float32 kernel cannot be expected to beat."""
    p = {k: torch.as_tensor(np.asarray(v), dtype=torch.float32) for k, v in sd32.items()}
    f = lambda t: None if t is None else torch.as_tensor(np.asarray(t), dtype=torch.float32)      # noqa: E731
    with torch.no_grad():
        return R.policy_forward(p, f(obs), f(avail), f(adj), f(ch), N, residual)


def inputs(N, S, d, hops, masks, seed, obs_pool=None, masked_row=False):
    """One case's inputs as float32 numpy: obs [S,N*d], avail [S,N,5] | None, adj [S,N,N] | None, channels [S,hops,N,N] | None.
    obs_pool [rows, d]: recorded per-agent observations, drawn row by row (a team of recorded agents); without one, sparse
    0/1 features plus noise.  masks: 'none' (all None), 'links' (range and channel masks, self-links kept, `masked_row`: agent 0
    of env 0 hears nobody, itself included), 'avail' (the links plus action 1 removed for ~30 % of the agents and one agent - env 0's
    last - left with action 3 only)."""
    rng = np.random.RandomState(seed)
    if obs_pool is not None:
        pool = np.asarray(obs_pool, np.float32).reshape(-1, d)
        obs = pool[rng.randint(0, pool.shape[0], size=S * N)].reshape(S, N * d)
    else:
        obs = ((rng.rand(S, N * d) < 0.3) + 0.05 * rng.randn(S, N * d)).astype(np.float32)
    adj = ch = avail = None
    if masks != "none":
        idx = np.arange(N)
        adj = (rng.rand(S, N, N) < 0.7).astype(np.float32)
        adj[:, idx, idx] = 1.0
        ch = (rng.rand(S, hops, N, N) < 0.8).astype(np.float32)
        ch[:, :, idx, idx] = 1.0
        if masked_row:
            adj[0, 0, :] = 0.0
    if masks == "avail":
        avail = np.ones((S, N, 5), np.float32)
        avail[rng.rand(S, N) < 0.3, 1] = 0.0
        avail[0, N - 1] = (0, 0, 0, 1, 0)
    return np.ascontiguousarray(obs), avail, adj, ch


@functools.lru_cache(maxsize=None)
def uniforms(seed, env_id_offset, policy_step, S, N):
    """The sampler's uniform of every (env, agent): Philox counter (env_id_offset + s, policy_step, site 7, agent), key = the two
    halves of the seed, u = (first word >> 8) * 2^-24 (cm_rng.h: unit_f32) -> float64 [S,N] (each value exact in float32)."""
    from oracle import oracle as O
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    u = np.empty((S, N), np.float64)
    for s in range(S):
        for i in range(N):
            u[s, i] = (int(O.philox((env_id_offset + s, policy_step, 7, i), key)[0]) >> 8) * (1.0 / 16777216.0)
    u.setflags(write=False)
    return u


def _np64(x):
    return np.asarray(x.detach().cpu() if torch.is_tensor(x) else x, dtype=np.float64)


def cdf_actions64(probs64, u):
    """The kernels' rule in float64: the first c with u < p_0 + .. + p_c, else the last c with p_c > 0.  -> int [S,N]."""
    p = _np64(probs64)
    below = np.asarray(u)[..., None] < np.cumsum(p, axis=-1)
    A = p.shape[-1]
    first = np.where(below.any(-1), below.argmax(-1), -1)
    last = A - 1 - (p[..., ::-1] > 0).argmax(-1)
    return np.where(first >= 0, first, last).astype(np.int64)


def near_boundary(probs64, u, delta):
    """Draws whose u lies within `delta` of a boundary p_0 + .. + p_c (c < A - 1) of the float64 CDF -> bool [S,N]."""
    cs = np.cumsum(_np64(probs64), axis=-1)[..., :-1]
    return (np.abs(np.asarray(u)[..., None] - cs) <= delta).any(-1)


def greedy_undecided(probs64, gap=GREEDY_GAP):
    """Rows whose float64 top-two probabilities differ by less than `gap` -> bool [S,N]."""
    top = np.sort(_np64(probs64), axis=-1)
    return (top[..., -1] - top[..., -2]) < gap
