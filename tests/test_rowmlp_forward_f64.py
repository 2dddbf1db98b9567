"""The row-MLP forward (csrc/cm_mlp.hip, csrc/cm_mlp_body.h: the acting forward of the Obs-DP and CENT policies, of GaussianMLPBaseline and
of the head + sampler of Comm-DP teams above 80 agents) at RUN-TIME layer sizes against float64, through the C ABI with _lib.MlpWeights as
nets._RowMLPPolicy builds it.  tests/f64_rowmlp.py has the cases (one to six layers, widths of 1, of no multiple of 16, of the LDS limit
624, in_dim 1 / 129 / 5544, n_act 3 / 5 / 8, a NULL bias, one row to two workgroups and a row), the float64 restatement and judge(), the
one function that applies every bar; tests/test_rowmlp_cases_cpu.py shows on the CPU that the restatement is the reference's arithmetic,
that each regime took hold, that plain float32 stays within half of every bar on every case, and that judge() rejects wrong answers.

Per case, regime (init / peaked / sat) and mask setting (none / `avail`), with the operand pack of cm_mlp_pack and again with
mfma_pack = NULL (the plain-weight gather Python never reaches), outputs NaN (actions -1) inside 64-element guard bands,
env_id_offset = 1000, policy_step = 5 and a device policy_step_base of 2, TAU = 1e-5, M = max|logit64|:
  * every probability row finite, non-negative, summing to 1 within 1e-6; a masked action exactly 0; the single-action row exactly 1;
  * log-probabilities within 2 TAU M where p64 >= 1e-30, elsewhere 0 <= p <= 1e-29; probabilities within TAU max(1, M / 2) (the strict
    ratio against 1e-5 is printed beside it); values within TAU max|v64|;
  * sampled actions == the oracle's inverse-CDF draw on the kernel's own probabilities, exactly; == the float64 rule on the float64
    probabilities off the draws the CPU test counted as undecided; never an unavailable action; greedy == the first maximum of the
    kernel's own probabilities, exactly, and == the float64 argmax off the undecided rows;
  * plain-weight outputs == packed outputs bit for bit (both routes feed the same operands to the same instruction sequence:
    pack_layer_kernel zero-pads exactly as the gather does); probs = NULL gives the same actions, actions = NULL the same probability
    bits, the greedy call the same probability bits; guard bands untouched; rows = 0 returns 0 and writes nothing.
Each case prints its worst strict and worst applied ratio next to chain32's (float32 alone, tests/f64_rowmlp.py).

The set launch (cm_mlp_policy_forward_multi, three members each) equals one launch per member bit for bit for `cent72` (env rows, groups of
[33, 1, 2] envs) and for `six` with groups of [9, 1, 7] envs.  The planner takes groups == 1 or groups == agents_per_env: the 4 x 5 logits
of `six` are env rows to it (9 / 1 / 7 rows), so the agent-row form (groups = 1, agents_per_env = 4: 36 / 4 / 28 rows, a full workgroup
and a ragged one in a member) is run as well on the same chain with a last layer of 5 outputs (`six_agent_rows`).

The Python route - CentralizedCategoricalMLPPolicy(hidden_sizes=(128, 200, 17)) at N = 4, d = 21 and GaussianMLPBaseline(hidden_sizes=(64,
600)) - must be seen (the spy of tests/test_acting_forward_f64.py) to run cm_mlp_policy_forward / cm_mlp_value_forward, return the bits of
the direct C-ABI call and meet the bars.  The shapes the kernel cannot run are refused: rc < 0, a text in cm_last_error, outputs untouched.

Measured on an MI355X: the table in DESIGN.md §2 ("Row-MLP forward at run-time layer sizes")."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import f64_rowmlp as M
from tests.lib_spy import spy  # noqa: F401  (the fixture: a recording proxy around _lib.lib())

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
POLICY = [(c, r) for c in M.CASES for r in M.regimes(c) if not M.CASES[c]["value"]]
VALUE = [(c, r) for c in M.CASES for r in M.regimes(c) if M.CASES[c]["value"]]


def _L():
    from com_marl_amd import _lib as L
    return L


def _guarded(shape, dtype, fill):
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return flat, flat[GUARD:GUARD + n].view(*shape)


def _bands_untouched(flat, fill):
    for band in (flat[:GUARD], flat[-GUARD:]):
        b = band.cpu().numpy()
        if not (np.isnan(b).all() if fill is None else (b == fill).all()):
            return False
    return True


def _dev(a):
    return None if a is None else torch.as_tensor(np.array(a)).to(DEV)       # (a copy: the shared arrays are read-only)


class _Weights:
    """A chain's float32 arrays on the device and the cm_mlp_weights over them; `packed`: with cm_mlp_pack's output."""

    def __init__(self, shape, layers, packed):
        L, c = _L(), M._c(shape)
        self.keep = []
        w = self.w = L.MlpWeights()
        w.in_dim, w.n_layers, w.tanh_mask, w.relu_mask = c["in_dim"], len(layers), 0, 0
        for l, (wt, b, a) in enumerate(layers):
            assert wt.shape[1] == c["out_dim"][l]
            w.out_dim[l] = wt.shape[1]
            t, tb = _dev(wt), _dev(b)
            self.keep += [t, tb]
            w.wt[l], w.b[l] = t.data_ptr(), None if tb is None else tb.data_ptr()
            w.tanh_mask |= int(a == 1) << l
            w.relu_mask |= int(a == 2) << l
        if packed:
            n = L.lib().cm_mlp_pack_bytes(C.byref(w))
            assert n > 0 and n % 4 == 0
            self.pack = torch.zeros(n // 4, dtype=torch.float32, device=DEV)
            L.check(L.lib().cm_mlp_pack(C.byref(w), L.ptr(self.pack), L.current_stream()), "cm_mlp_pack")
            w.mfma_pack = self.pack.data_ptr()


def _base():
    return torch.full((1,), M.STEP_BASE, dtype=torch.int32, device=DEV)


def _policy(shape, w, x, avail, greedy, want_probs=True, want_actions=True, rows=None, env_id_offset=M.ENV_ID_OFFSET):
    """One cm_mlp_policy_forward -> (rc, probs [rows*groups, n_act] | None, actions [rows*groups] | None); asserts the guard bands."""
    L, c = _L(), M._c(shape)
    rows = x.shape[0] if rows is None else rows
    n = x.shape[0] * c["groups"]
    fp, probs = _guarded((n, c["n_act"]), torch.float32, float("nan"))
    fa, actions = _guarded((n,), torch.int32, -1)
    base = _base()
    rc = L.lib().cm_mlp_policy_forward(C.byref(w), rows, c["groups"], c["n_act"], c["agents"], L.ptr(x), L.ptr(avail), M.SEED,
                                       env_id_offset, M.POLICY_STEP, L.ptr(base), int(greedy), L.ptr(actions) if want_actions else None,
                                       L.ptr(probs) if want_probs else None, L.current_stream())
    torch.cuda.synchronize()
    assert _bands_untouched(fp, None) and _bands_untouched(fa, -1), "a guard band was written"
    return rc, probs.cpu().numpy(), actions.cpu().numpy().astype(np.int64)


def _value(w, x, rows=None):
    L = _L()
    fv, values = _guarded((x.shape[0],), torch.float32, float("nan"))
    rc = L.lib().cm_mlp_value_forward(C.byref(w), x.shape[0] if rows is None else rows, L.ptr(x), L.ptr(values), L.current_stream())
    torch.cuda.synchronize()
    assert _bands_untouched(fv, None), "a guard band was written"
    return rc, values.cpu().numpy()


def _untouched(probs=None, actions=None, values=None):
    return all([probs is None or np.isnan(probs).all(), actions is None or (actions == -1).all(), values is None or np.isnan(values).all()])


def _ok(rc):
    assert rc == 0, (rc, _L().lib().cm_last_error())


def _fmt(m):
    which = max((k for k in m if not k.startswith("n_") and k != "probs_strict"), key=lambda k: m[k])
    strict = f"strict {m['probs_strict']:.3f}, " if "probs_strict" in m else ""
    return f"{strict}applied {m[which]:.3f} ({which})"


def _judge_policy(tag, shape, ref, f32, w_packed, w_plain, x, avail_dev):
    """Everything the module docstring lists for one (case, regime, mask); -> judge()'s metrics of the packed route."""
    c = M._c(shape)
    rc, probs, acts = _policy(shape, w_packed.w, x, avail_dev, greedy=False)
    _ok(rc)
    rc, g_probs, g_acts = _policy(shape, w_packed.w, x, avail_dev, greedy=True)
    _ok(rc)
    m = M.judge(shape, ref, probs=probs, actions=acts, greedy=g_acts)
    print(f"ROWMLP {tag} | kernel {_fmt(m)} | float32 alone {_fmt(f32)} | M {ref['M']:.1f}, undecided draws {int(ref['near'].sum())}, "
          f"rows {int(ref['undecided'].sum())}")
    assert not M.rejected(m), f"{tag}: {M.rejected(m)} of {m} (float32 alone: {f32})"
    np.testing.assert_array_equal(g_probs, probs, err_msg=f"{tag}: greedy and sampled calls returned other probabilities")
    want = O.sample_actions(np.ascontiguousarray(probs.reshape(M.envs_of(shape), c["agents"], c["n_act"]), np.float32), M.SEED,
                            M.ENV_ID_OFFSET, M.POLICY_STEP + M.STEP_BASE).reshape(-1)
    np.testing.assert_array_equal(acts, want, err_msg=f"{tag}: sampled actions != the oracle's draw on the kernel's own probabilities")
    np.testing.assert_array_equal(g_acts, M.first_max(probs), err_msg=f"{tag}: greedy != the first maximum of the kernel's own probabilities")
    # the plain-weight gather: the same bits
    for greedy, p0, a0 in ((False, probs, acts), (True, probs, g_acts)):
        rc, p1, a1 = _policy(shape, w_plain.w, x, avail_dev, greedy=greedy)
        _ok(rc)
        np.testing.assert_array_equal(p1, p0, err_msg=f"{tag}: plain-weight probabilities differ from the packed ones (greedy={greedy})")
        np.testing.assert_array_equal(a1, a0, err_msg=f"{tag}: plain-weight actions differ from the packed ones (greedy={greedy})")
    # one output only
    rc, p1, a1 = _policy(shape, w_packed.w, x, avail_dev, greedy=False, want_probs=False)
    _ok(rc)
    assert _untouched(probs=p1), f"{tag}: probs = NULL, yet something wrote the buffer the test kept"
    np.testing.assert_array_equal(a1, acts, err_msg=f"{tag}: probs = NULL changed the actions")
    rc, p1, a1 = _policy(shape, w_packed.w, x, avail_dev, greedy=False, want_actions=False)
    _ok(rc)
    assert _untouched(actions=a1)
    np.testing.assert_array_equal(p1, probs, err_msg=f"{tag}: actions = NULL changed the probabilities")
    return m


@pytest.mark.parametrize("case,regime", POLICY)
def test_policy_forward_matches_f64(case, regime):
    d = M.build(case, regime)
    w_packed, w_plain = _Weights(case, d["layers"], True), _Weights(case, d["layers"], False)
    assert w_packed.w.mfma_pack and not w_plain.w.mfma_pack
    x = _dev(d["x"])
    for mask in M.MASKS:
        ref = M.reference(case, regime, mask)
        _judge_policy(f"{case} {regime} {mask}", case, ref, M.float32_alone(case, regime, mask), w_packed, w_plain, x,
                      _dev(ref["avail"]))


@pytest.mark.parametrize("case,regime", VALUE)
def test_value_forward_matches_f64(case, regime):
    d = M.build(case, regime)
    ref, x = M.reference(case, regime, "none"), _dev(d["x"])
    w_packed, w_plain = _Weights(case, d["layers"], True), _Weights(case, d["layers"], False)       # (kept alive: they own the device arrays)
    rc, v = _value(w_packed.w, x)
    _ok(rc)
    m, f32 = M.judge(case, ref, values=v), M.float32_alone(case, regime, "none")
    print(f"ROWMLP {case} {regime} none | kernel {_fmt(m)} | float32 alone {_fmt(f32)} | max|v64| {np.abs(ref['v']).max():.3g}")
    assert not M.rejected(m), f"{case} {regime}: {m} (float32 alone: {f32})"
    rc, v1 = _value(w_plain.w, x)
    _ok(rc)
    np.testing.assert_array_equal(v1, v, err_msg=f"{case} {regime}: plain-weight values differ from the packed ones")


def test_an_empty_batch_writes_nothing():
    for case, packed in (("obsdp_a3", True), ("obsdp_a3", False)):
        d = M.build(case, "init")
        w = _Weights(case, d["layers"], packed)
        rc, p, a = _policy(case, w.w, _dev(d["x"]), None, greedy=False, rows=0)
        assert rc == 0 and _untouched(probs=p, actions=a)
    d = M.build("val_wide", "init")
    w = _Weights("val_wide", d["layers"], True)
    rc, v = _value(w.w, _dev(d["x"]), rows=0)
    assert rc == 0 and _untouched(values=v)


# ---- the set launch -------------------------------------------------------------------------------------------------------------------
SIX_AGENT_ROWS = M._case(84, [128, 624, 17, 1, 200, 5], "t r t t r -", 1, 5, 4, 0, "the chain of `six` over agent rows: groups = 1")
SETS = {"six": (M.CASES["six"], [9, 1, 7]), "six_agent_rows": (SIX_AGENT_ROWS, [9, 1, 7]), "cent72": (M.CASES["cent72"], [33, 1, 2])}


@pytest.mark.parametrize("name", sorted(SETS))
def test_set_launch_equals_a_launch_per_member(name):
    L = _L()
    shape, sizes = SETS[name]
    per_env = shape["agents"] // shape["groups"]
    shape = dict(shape, rows=sum(sizes) * per_env)
    K, n_envs = len(sizes), sum(sizes)
    draws = [M.draw(shape, "peaked", M.seed_of(name) + k) for k in range(K)]
    ws = [_Weights(shape, d["layers"], True) for d in draws]
    x, avail = _dev(draws[0]["x"]), _dev(draws[0]["avail"])
    arr, grp, n_wg = (L.MlpWeights * K)(*[w.w for w in ws]), (C.c_int32 * K)(*sizes), C.c_int32(0)
    plan = (arr, grp, K, n_envs, shape["groups"], shape["n_act"], shape["agents"])
    need = L.lib().cm_mlp_forward_multi_plan(*plan, None, 0, C.byref(n_wg))
    assert need > 0 and n_wg.value == sum(-(-s * per_env // 32) for s in sizes), (need, n_wg.value, L.lib().cm_last_error())
    image = bytearray(need)
    assert L.lib().cm_mlp_forward_multi_plan(*plan, (C.c_char * need).from_buffer(image), need, C.byref(n_wg)) == need
    table = torch.frombuffer(image, dtype=torch.uint8).to(DEV)
    n = shape["rows"] * shape["groups"]
    for greedy in (False, True):
        ref_p, ref_a, lo = [], [], 0
        for k, s in enumerate(sizes):
            r0, r1 = lo * per_env, (lo + s) * per_env
            rc, p, a = _policy(shape, ws[k].w, x[r0:r1], avail[r0 * shape["groups"]:r1 * shape["groups"]], greedy,
                               env_id_offset=M.ENV_ID_OFFSET + lo)
            _ok(rc)
            ref_p.append(p), ref_a.append(a)
            lo += s
        ref_p, ref_a = np.concatenate(ref_p), np.concatenate(ref_a)
        assert not np.isnan(ref_p).any() and (ref_a >= 0).all() and ref_p.max() > 0.99
        fp, probs = _guarded((n, shape["n_act"]), torch.float32, float("nan"))
        fa, actions = _guarded((n,), torch.int32, -1)
        base = _base()
        rc = L.lib().cm_mlp_policy_forward_multi(C.byref(ws[0].w), L.ptr(table), n_wg.value, n_envs, shape["groups"], shape["n_act"],
                                                 shape["agents"], L.ptr(x), L.ptr(avail), M.SEED, M.ENV_ID_OFFSET, M.POLICY_STEP,
                                                 L.ptr(base), int(greedy), L.ptr(actions), L.ptr(probs), L.current_stream())
        _ok(rc)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(probs.cpu().numpy(), ref_p, err_msg=f"{name}: the set launch's probabilities (greedy={greedy})")
        np.testing.assert_array_equal(actions.cpu().numpy(), ref_a, err_msg=f"{name}: the set launch's actions (greedy={greedy})")
        assert _bands_untouched(fp, None) and _bands_untouched(fa, -1), "a guard band was written"


# ---- the Python route -----------------------------------------------------------------------------------------------------------------
def _spec(d_total):
    from com_marl_amd.envs import EnvSpec, _Box, _Discrete
    return EnvSpec(_Box(np.zeros(d_total), np.ones(d_total)), _Discrete(5))


def _load(net, layers):
    with torch.no_grad():
        for (lin, _), (wt, b, _) in zip(net._chain(), layers):
            lin.weight.copy_(torch.as_tensor(np.array(wt.T)))
            lin.bias.copy_(torch.as_tensor(np.array(b)))


PY_CENT = M._case(84, [128, 200, 17, 20], "t t t -", 4, 5, 4, 37, "CentralizedCategoricalMLPPolicy(hidden_sizes=(128, 200, 17)), N = 4, d = 21")
PY_GB = M._case(84, [64, 600, 1], "t t -", None, 0, 0, 33, "GaussianMLPBaseline(hidden_sizes=(64, 600))")


@pytest.mark.parametrize("regime", ["init", "peaked", "sat"])
def test_python_route_centralized_policy(regime, spy):  # noqa: F811
    from com_marl_amd import nets
    pol = nets.CentralizedCategoricalMLPPolicy(_spec(84), n_agents=4, hidden_sizes=(128, 200, 17), device=DEV)
    d = M.draw(PY_CENT, regime, M.seed_of("py_cent"))
    assert [(l.in_features, l.out_features, int(a)) for l, a in pol._chain()] == [(w.shape[0], w.shape[1], a) for w, _, a in d["layers"]]
    _load(pol, d["layers"])
    pol.set_rng(M.SEED, M.ENV_ID_OFFSET)
    x, base = _dev(d["x"]), _base()
    w_packed, w_plain = _Weights(PY_CENT, d["layers"], True), _Weights(PY_CENT, d["layers"], False)
    for mask in M.MASKS:
        ref = M.reference_of(PY_CENT, d["x"], d["layers"], d["avail"] if mask == "avail" else None)
        if regime != "init":
            assert ref["M"] >= 20 and ref["probs"].max() > 0.99
        av = _dev(ref["avail"])
        for greedy in (False, True):
            spy.calls.clear()
            a, p, _ = pol.act_device(x, None if av is None else av.reshape(37, 4, 5), greedy=greedy, policy_step=M.POLICY_STEP, step_base=base)
            torch.cuda.synchronize()
            assert "cm_mlp_policy_forward" in spy.calls, spy.calls
            assert a.shape == (37, 4) and p.shape == (37, 4, 5)
            rc, p0, a0 = _policy(PY_CENT, w_packed.w, x, av, greedy)
            _ok(rc)
            np.testing.assert_array_equal(p.cpu().numpy().reshape(-1, 5), p0, err_msg="act_device's probabilities are not the C-ABI call's")
            np.testing.assert_array_equal(a.cpu().numpy().reshape(-1), a0, err_msg="act_device's actions are not the C-ABI call's")
        f32 = M.float32_of(PY_CENT, d["x"], d["layers"], ref)
        assert M.worst_applied(f32) <= 0.5, f32
        _judge_policy(f"py_cent {regime} {mask}", PY_CENT, ref, f32, w_packed, w_plain, x, av)


@pytest.mark.parametrize("regime", ["init", "sat"])
def test_python_route_gaussian_baseline(regime, spy):  # noqa: F811
    from com_marl_amd import nets
    gb = nets.GaussianMLPBaseline(env_spec=_spec(84), hidden_sizes=(64, 600), device=DEV)
    d = M.draw(PY_GB, regime, M.seed_of("py_gb"))
    assert [(l.in_features, l.out_features, int(a)) for l, a in gb._chain()] == [(w.shape[0], w.shape[1], a) for w, _, a in d["layers"]]
    _load(gb, d["layers"])
    x = _dev(d["x"])
    spy.calls.clear()
    with torch.no_grad():
        v = gb.forward(x.reshape(1, 33, 84))
    torch.cuda.synchronize()
    assert "cm_mlp_value_forward" in spy.calls and v.shape == (1, 33), spy.calls
    w = _Weights(PY_GB, d["layers"], True)
    rc, v0 = _value(w.w, x)
    _ok(rc)
    np.testing.assert_array_equal(v.cpu().numpy()[0], v0, err_msg="the baseline's values are not the C-ABI call's")
    ref = M.reference_of(PY_GB, d["x"], d["layers"], None)
    m, f32 = M.judge(PY_GB, ref, values=v0), M.float32_of(PY_GB, d["x"], d["layers"], ref)
    print(f"ROWMLP py_gb {regime} none | kernel {_fmt(m)} | float32 alone {_fmt(f32)} | max|v64| {np.abs(ref['v']).max():.3g}")
    assert M.worst_applied(f32) <= 0.5 and not M.rejected(m), (m, f32)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def _refusal_shape(out_dim, groups=1, n_act=5, act=None):
    return M._case(8, out_dim, act or " ".join(["t"] * (len(out_dim) - 1) + ["-"]), groups, n_act, 1 if groups is not None else 0, 4, "a shape to refuse")


# name: (shape, what to change in the cm_mlp_weights / the call)
REFUSALS = {
    "first layer 129 wide": (_refusal_shape([129, 5]), {}),
    "a later layer 625 wide": (_refusal_shape([16, 625, 5]), {}),
    "a later layer 1024 wide": (_refusal_shape([16, 1024, 5]), {}),
    "n_layers 0": (_refusal_shape([16, 5]), {"n_layers": 0}),
    "n_layers 7": (_refusal_shape([16, 5]), {"n_layers": 7}),
    "both mask bits of a layer": (_refusal_shape([16, 5]), {"relu_mask": 1}),
    "last width != groups x n_act": (_refusal_shape([16, 6]), {}),
    "n_act = 9": (_refusal_shape([16, 9], n_act=9), {}),
    "value forward with last width 2": (_refusal_shape([16, 2], groups=None, n_act=0), {}),
    "neither output requested": (_refusal_shape([16, 5]), {"no_output": True}),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refused_shapes(name):
    L = _L()
    shape, change = REFUSALS[name]
    d = M.draw(shape, "init", 1)
    x = _dev(d["x"])
    for packed in (False, True):
        w = _Weights(shape, d["layers"], False)             # (cm_mlp_pack is not what refuses: the pack of a refused shape is a buffer of
        if packed:                                           # the right size, zeros - nothing reads it)
            n = L.lib().cm_mlp_pack_bytes(C.byref(w.w))
            w.pack = torch.zeros(n // 4, dtype=torch.float32, device=DEV)
            w.w.mfma_pack = w.pack.data_ptr()
        for field in ("n_layers", "relu_mask"):
            if field in change:
                setattr(w.w, field, change[field])
        if shape["value"]:
            rc, v = _value(w.w, x)
            out = dict(values=v)
        else:
            none = bool(change.get("no_output"))
            rc, p, a = _policy(shape, w.w, x, None, greedy=False, want_probs=not none, want_actions=not none)
            out = dict(probs=p, actions=a)
        assert rc < 0, f"{name}: accepted (rc {rc})"
        assert L.lib().cm_last_error(), f"{name}: no text in cm_last_error"
        assert _untouched(**out), f"{name}: refused, yet an output was written"


def test_width_624_is_the_widest_accepted():
    """The limit the header states: `six` runs a layer of 624 (asserted with the rest of the case above); here the bare claim, a later
    layer of 624 accepted and the next padded width, 625 -> 640, refused, on one small chain."""
    for width, accepted in ((624, True), (625, False)):
        shape = _refusal_shape([16, width, 5])
        d = M.draw(shape, "init", 2)
        w = _Weights(shape, d["layers"], True)
        rc, p, a = _policy(shape, w.w, _dev(d["x"]), None, greedy=False)
        assert (rc == 0) == accepted and (rc <= 0), (width, rc)
        assert _untouched(probs=p, actions=a) == (not accepted)
