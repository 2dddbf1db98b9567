"""What the tests of the row-MLP forward (csrc/cm_mlp.hip, csrc/cm_mlp_body.h) at run-time layer sizes share (no test in here, no GPU,
nothing of com_marl_amd):

  CASES            the smallest shapes at which each branch of the kernel is still reached (the `reaches` text of every case)
  build            a case in a regime: float32 weights, biases and input, seeded by the case's NAME (crc32: stable between runs)
  chain64          the layer chain in float64, y = act(x @ wt + b), a None bias meaning none; probs64 the per-group softmax x avail,
                   renormalised; reference() both plus the float64 draw (acting_regimes.cdf_actions64), the greedy first maximum and
                   the draws / rows a probability error of the case's bar leaves undecided
  chain32          the same chain in float32, k-sequential accumulation, the kernel's tanh 1 - 2 / (exp2(2.88539 x) + 1) and the
                   kernel's order of the softmax: what float32 ALONE does to a case, never a reference
  judge            every applied metric of an output against the float64 reference, each in units of its bar.  ONE function for the
                   kernel (tests/test_rowmlp_forward_f64.py: every ratio <= 1, every count 0), for chain32 (tests/test_rowmlp_cases_cpu.py:
                   every ratio <= 0.5, "the inputs are fair") and for the wrong answers built in float64 (rejected() must be non-empty)

Bars (TAU = 1e-5, the project's forward bar), M = max|logit64| of the case:
  logits            |lg - lg64| <= TAU M                      (chain32 only: the kernel does not return its logits)
  log-probabilities |log p - log p64| <= 2 TAU M where p64 >= 1e-30 (log-softmax is 2-Lipschitz in the sup norm of the logits, and
                    the `avail` renormalisation is a log-softmax over the available ones); elsewhere 0 <= p <= 1e-29
  probabilities     |p - p64| <= TAU max(1, M / 2): softmax moves by at most half the sup-norm change of its logits, which are held
                    to TAU M; in `init` (M < 2) this is the strict 1e-5.  The strict ratio - against 1e-5 - is reported beside it
  values            max|v - v64| <= TAU max|v64|
Regimes: `init` (U(+-1/sqrt(fan_in)) weights and biases, x in U[0, 1)); `peaked` (the last layer's weight and bias scaled so that
M = 40); `sat` (layer 0's weight and bias x14, then the last layer scaled to M = 40; a value chain keeps its last layer).  A one-layer
policy chain has no hidden unit to saturate and takes init / peaked; value cases take init / sat."""
import functools
import zlib

import numpy as np

from tests import acting_regimes as G

TAU = 1e-5
SEED, ENV_ID_OFFSET, POLICY_STEP, STEP_BASE = G.SEED, 1000, 5, 2      # the sampler's stream: the counter's step is POLICY_STEP + STEP_BASE
PEAK = 40.0
SAT_GAIN = 14.0
ACT = {"-": 0, "t": 1, "r": 2}


def _case(in_dim, out_dim, act, groups, n_act, agents, rows, reaches, nobias=()):
    assert len(out_dim) == len(act.split())
    return dict(in_dim=in_dim, out_dim=tuple(out_dim), act=tuple(ACT[a] for a in act.split()), groups=groups, n_act=n_act,
                agents=agents, rows=rows, reaches=reaches, nobias=tuple(nobias), value=groups is None)


CASES = {
    "one_21_5": _case(21, [5], "-", 1, 5, 4, 36, "n_layers = 1 (the sampler reads layer 0's tile); ragged second k-quad; 32 + 4 rows"),
    "one_300_128": _case(300, [128], "-", 16, 8, 16, 1,
                         "8 column tiles (both tiles of every wave); 3 chunks, the last 44 wide; n_act = 8; one row"),
    "six": _case(84, [128, 624, 17, 1, 200, 20], "t r t t r -", 4, 5, 4, 65,
                 "6 layers; 624 = the LDS limit (row stride 628); one column past a tile; width 1 then K = 1; 13 tiles; mixed "
                 "activations; 2 full workgroups + 1 row"),
    "cent72": _case(5544, [128, 64, 32, 360], "t t t -", 72, 5, 72, 3, "CENT at N = 72, d = 77: 44 chunks, the last 40 wide; 23 logit tiles"),
    "maxlds": _case(129, [16, 620], "t -", 124, 5, 124, 31,
                    "K = CHUNK + 1 (a second chunk of one column); 39 tiles padded to 624; 3844 sampler items on 256 threads"),
    "relu3": _case(84, [128, 64, 32, 20], "r r r -", 4, 5, 4, 32, "ReLU hidden layers; exactly one full workgroup"),
    "obsdp_a3": _case(21, [128, 64, 32, 3], "t t t -", 1, 3, 4, 64, "n_act = 3; two full workgroups"),
    "nobias": _case(21, [128, 64, 32, 3], "t t t -", 1, 3, 4, 64, "obsdp_a3 with b[1] = b[3] = NULL (C ABI only)", nobias=(1, 3)),
    "val_1848": _case(1848, [64, 64, 64, 1], "t t t -", None, 0, 0, 37, "the Gaussian baseline at N = 24"),
    "val_1_1": _case(1, [1], "-", None, 0, 0, 1, "K = 1, one layer, one row"),
    "val_wide": _case(40, [128, 600, 1], "r r -", None, 0, 0, 33, "a wide hidden layer into a width-1 output"),
}
assert all(c["rows"] <= 65 for c in CASES.values())
MASKS = ("none", "avail")


def regimes(name):
    c = CASES[name]
    if c["value"]:
        return ("init", "sat")
    return ("init", "peaked", "sat") if len(c["out_dim"]) > 1 else ("init", "peaked")


def seed_of(name):
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


def _act64(y, a):
    return np.tanh(y) if a == 1 else (np.where(y < 0, 0.0, y) if a == 2 else y)


def chain64(x, layers, upto=None):
    """layers: [(wt [in,out], b [out] | None, activation code 0 none / 1 tanh / 2 ReLU)] -> the output of layer `upto` (default: the
    last) in float64."""
    y = np.asarray(x, np.float64)
    for wt, b, a in layers[:None if upto is None else upto + 1]:
        y = y @ np.asarray(wt, np.float64)
        if b is not None:
            y = y + np.asarray(b, np.float64)
        y = _act64(y, a)
    return y


def probs64(logits, avail, groups, n_act, renormalise=True):
    """[rows, groups * n_act] logits -> [rows * groups, n_act]: per group softmax, times avail, renormalised."""
    lg = np.asarray(logits, np.float64).reshape(-1, n_act)
    e = np.exp(lg - lg.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    if avail is not None:
        p = p * np.asarray(avail, np.float64).reshape(p.shape)
    return p / p.sum(-1, keepdims=True) if renormalise else p


def _tanh32(y):
    with np.errstate(over="ignore"):
        t = np.exp2(y * np.float32(2.8853900817779268))
    return (np.float32(1.0) - np.float32(2.0) / (t + np.float32(1.0))).astype(np.float32)


def chain32(x, layers):
    """The chain in float32: one rounded multiply and one rounded add per k, in k order; the kernel's tanh form."""
    y = np.asarray(x, np.float32)
    for wt, b, a in layers:
        wt = np.asarray(wt, np.float32)
        acc = np.zeros((y.shape[0], wt.shape[1]), np.float32)
        for k in range(wt.shape[0]):
            acc += y[:, k, None] * wt[k][None, :]
        if b is not None:
            acc = acc + np.asarray(b, np.float32)
        y = _tanh32(acc) if a == 1 else (np.where(acc < 0, np.float32(0), acc) if a == 2 else acc)
    return y.astype(np.float32)


def probs32(logits, avail, n_act):
    """cm_mlp_body.h's order in float32: exp(lg - max), / sum, x avail, / masked sum."""
    lg = np.asarray(logits, np.float32).reshape(-1, n_act)
    e = np.exp(lg - lg.max(-1, keepdims=True)).astype(np.float32)
    p = e / e.sum(-1, keepdims=True, dtype=np.float32)
    if avail is not None:
        p = p * np.asarray(avail, np.float32).reshape(p.shape)
    return (p / p.sum(-1, keepdims=True, dtype=np.float32)).astype(np.float32)


def single_action(n_act):
    return min(3, n_act - 1)


def _c(case):
    return CASES[case] if isinstance(case, str) else case


def make_avail(case, rng):
    """Action 1 forbidden on about 30 % of the agent rows; env 0's last agent is left with single_action(n_act) alone."""
    c = _c(case)
    n = c["rows"] * c["groups"]
    av = np.ones((n, c["n_act"]), np.float32)
    av[rng.rand(n) < 0.3, 1] = 0.0
    av[c["agents"] - 1] = 0.0
    av[c["agents"] - 1, single_action(c["n_act"])] = 1.0
    return av


def draw(case, regime, seed):
    """A shape (a CASES name or a dict of _case's form) in a regime from `seed` -> dict(x [rows,in_dim] float32, layers [(wt [in,out]
    float32, b float32 | None, act)], avail [rows*groups, n_act] float32: the mask of the 'avail' setting, None for a value shape)."""
    c = _c(case)
    rng = np.random.RandomState(seed)
    x = rng.rand(c["rows"], c["in_dim"]).astype(np.float32)
    layers, K = [], c["in_dim"]
    for l, (out, a) in enumerate(zip(c["out_dim"], c["act"])):
        lim = 1.0 / np.sqrt(K)
        wt = rng.uniform(-lim, lim, (K, out)).astype(np.float32)
        b = rng.uniform(-lim, lim, out).astype(np.float32)
        layers.append([wt, None if l in c["nobias"] else b, a])
        K = out
    avail = None if c["value"] else make_avail(c, rng)
    if regime == "sat":
        layers[0][0] = (layers[0][0] * np.float32(SAT_GAIN)).astype(np.float32)
        if layers[0][1] is not None:
            layers[0][1] = (layers[0][1] * np.float32(SAT_GAIN)).astype(np.float32)
    if regime in ("peaked", "sat") and not c["value"]:
        s = np.float32(PEAK / np.abs(chain64(x, layers)).max())
        layers[-1][0] = (layers[-1][0] * s).astype(np.float32)
        if layers[-1][1] is not None:
            layers[-1][1] = (layers[-1][1] * s).astype(np.float32)
    for a in [x, avail] + [t for l in layers for t in l[:2]]:
        if a is not None:
            a.setflags(write=False)
    return dict(regime=regime, x=x, layers=[tuple(l) for l in layers], avail=avail)


@functools.lru_cache(maxsize=None)
def build(case, regime, seed=None):
    """draw() of a CASES name, seeded by the name unless told otherwise.  Read-only and cached: shared between tests."""
    assert regime in regimes(case), (case, regime)
    return draw(case, regime, seed_of(case) if seed is None else seed)


def envs_of(case):
    c = _c(case)
    assert (c["rows"] * c["groups"]) % c["agents"] == 0
    return c["rows"] * c["groups"] // c["agents"]


def uniforms(case, env_id_offset=ENV_ID_OFFSET):
    """The sampler's uniform of every agent row, [rows * groups] float64 (flat = row * groups + group; env = flat // agents)."""
    return G.uniforms(SEED, env_id_offset, POLICY_STEP + STEP_BASE, envs_of(case), _c(case)["agents"]).reshape(-1)


def first_max(p):
    """Greedy as cm_mlp_body.h reads: the first maximum (a later action wins only when strictly larger)."""
    return np.asarray(p).argmax(-1).astype(np.int64)


def reference_of(case, x, layers, avail):
    """The float64 answers of a shape on (x, layers, avail | None).
    -> dict: value shapes v; policy shapes logits [rows, groups*n_act], probs [rows*groups, n_act], M = max|logit64|, bar (of the
    probabilities), actions (the float64 inverse-CDF draw), greedy, near / undecided (draws within `bar` of a float64 CDF boundary /
    rows whose float64 top two are within `bar`), avail."""
    c = _c(case)
    out = chain64(x, layers)
    if c["value"]:
        return dict(v=out[:, 0])
    p = probs64(out, avail, c["groups"], c["n_act"])
    M = float(np.abs(out).max())
    bar = TAU * max(1.0, M / 2)
    u = uniforms(case)
    return dict(logits=out, probs=p, M=M, bar=bar, avail=avail, actions=G.cdf_actions64(p, u), greedy=first_max(p),
                near=G.near_boundary(p, u, bar), undecided=G.greedy_undecided(p, bar))


def reference(case, regime, mask, layers=None):
    """reference_of() a CASES name in a regime and mask setting (with `layers` in place of the case's own: the material of a negative
    control)."""
    d = build(case, regime)
    return reference_of(case, d["x"], d["layers"] if layers is None else layers, d["avail"] if mask == "avail" else None)


def judge(case, ref, probs=None, actions=None, greedy=None, values=None, logits=None):
    """Every applied metric of an output against reference(): {name: error / bar} for the tolerances, {name: count} for what
    must not happen at all (names starting with 'n_').  rejected(judge(..)) lists what fails."""
    c, m = _c(case), {}
    if values is not None:
        m["values"] = float(np.abs(np.asarray(values, np.float64) - ref["v"]).max() / (TAU * np.abs(ref["v"]).max()))
        m["n_not_finite"] = int((~np.isfinite(np.asarray(values, np.float64))).sum())
        return m
    if logits is not None:
        m["logits"] = float(np.abs(np.asarray(logits, np.float64) - ref["logits"]).max() / (TAU * ref["M"]))
    p64, av = ref["probs"], ref["avail"]
    if probs is not None:
        p = np.asarray(probs, np.float64).reshape(p64.shape)
        ok = np.isfinite(p) & (p >= 0)
        m["n_not_finite_or_negative"] = int((~ok).sum())
        p = np.where(ok, p, 0.0)
        m["n_rows_not_summing_to_1"] = int((np.abs(p.sum(-1) - 1) > 1e-6).sum())
        if av is not None:
            m["n_masked_not_0"] = int((p[av == 0] != 0).sum())
            m["n_single_action_row_not_1"] = int(p[c["agents"] - 1, single_action(c["n_act"])] != 1.0)
        m["probs_strict"] = float(np.abs(p - p64).max() / TAU)
        m["probs"] = float(np.abs(p - p64).max() / ref["bar"])
        big = p64 >= 1e-30
        with np.errstate(divide="ignore"):
            m["logp"] = float(np.abs(np.log(p[big]) - np.log(p64[big])).max() / (2 * TAU * ref["M"]))
        m["n_tiny_above_1e-29"] = int((p[~big] > 1e-29).sum())
    for name, got, want, skip in (("actions", actions, ref["actions"], ref["near"]), ("greedy", greedy, ref["greedy"], ref["undecided"])):
        if got is None:
            continue
        a = np.asarray(got, np.int64).reshape(-1)
        m[f"n_{name}_out_of_range"] = int(((a < 0) | (a >= c["n_act"])).sum())
        a = np.clip(a, 0, c["n_act"] - 1)
        m[f"n_{name}_differ_from_f64"] = int((a[~skip] != want[~skip]).sum())
        if av is not None:
            m[f"n_{name}_unavailable"] = int((np.take_along_axis(av, a[:, None], -1)[:, 0] != 1).sum())
    return m


def rejected(m):
    """The metrics of judge() that fail: a ratio above 1 (probs_strict is reported, never applied) or a count above 0."""
    return sorted(k for k, v in m.items() if k != "probs_strict" and (v > 0 if k.startswith("n_") else not v <= 1.0))


def worst_applied(m):
    return max([v for k, v in m.items() if not k.startswith("n_") and k != "probs_strict"], default=0.0)


def float32_of(case, x, layers, ref):
    """chain32's output of a shape as the kernel would return it, judged against `ref` -> judge()'s metrics."""
    c = _c(case)
    out = chain32(x, layers)
    if c["value"]:
        return judge(case, ref, values=out[:, 0])
    return judge(case, ref, probs=probs32(out, ref["avail"], c["n_act"]), logits=out)


@functools.lru_cache(maxsize=None)
def _chain32_of_case(case, regime):
    d = build(case, regime)
    return chain32(d["x"], d["layers"])


def float32_alone(case, regime, mask):
    """float32_of() a CASES name (the chain's float32 output computed once per case and regime)."""
    c, ref, out = CASES[case], reference(case, regime, mask), _chain32_of_case(case, regime)
    if c["value"]:
        return judge(case, ref, values=out[:, 0])
    return judge(case, ref, probs=probs32(out, ref["avail"], c["n_act"]), logits=out)
