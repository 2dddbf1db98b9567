"""CPU side of tests/test_rowmlp_forward_f64.py (the row-MLP forward at run-time layer sizes against float64): everything that can be
known about its cases before a kernel runs, from float64 and a float32 emulation alone (tests/f64_rowmlp.py).

  * chain64 / probs64 are the reference's arithmetic: the recorded outputs of its classes (tests/golden/variants_*.npz: dec.probs,
    dec.probs_masked, cent.probs, cent.probs_masked, gb.values) are rebuilt from the fixtures' state dicts at rtol = 1e-5;
  * each regime took hold: peaked / sat reach max|logit64| >= 20 and a probability above 0.99, init leaves every probability below
    0.6; under sat at least 30 % of a tanh first layer's units lie above 0.99 in magnitude.  A ReLU unit does not saturate: the
    analogue asserted for a ReLU first layer (relu3, val_wide) is that at least 30 % of its units exceed 1 - in init fewer than 1 %
    do - so that the layers behind it see inputs an order of magnitude above the trained-from-init scale;
  * the inputs are fair: chain32 - plain float32, k-sequential, the kernel's tanh form and softmax order - stays within HALF of every
    applied bar for every case x regime x mask.  A kernel ratio above a bar is then a kernel finding, not float32 noise;
  * the sampler condition: at the GPU test's stream, pooled over the cases of a regime, at most 1 % of the draws lie within the
    case's probability bar of a float64 CDF boundary and at most 1 % of the rows have their float64 top two within it (a cap on what
    the GPU test may leave unjudged, not a measurement);
  * negative controls: wrong answers built in float64 - never by running anything wrong - and handed to the same judge() as the
    kernel's output.  Each must be rejected in every case, regime and mask setting it applies to:
        layer 0 without its last input column; layer 0 without column 128, the first of the second chunk (every case wider than one
        chunk, maxlds and one_300_128 among them); the last column tile's bias dropped; tanh where the chain has ReLU; the `avail`
        renormalisation skipped; the last agent row's action drawn from the previous agent row's probabilities.
    Two coincide with the right answer and are asserted to coincide: the dropped bias of `nobias` (its last layer has none to drop),
    and the previous row's probabilities wherever they give the last row's uniform the same action and the same first maximum
    (COINCIDES_PREV_ROW lists them: three settings of one_21_5 and all six of obsdp_a3, whose last two rows agree throughout - `nobias`,
    the same shape, rejects it in all six; every other combination is rejected)."""
import os

import numpy as np
import pytest

from tests import f64_rowmlp as M
from tests.test_oracle_golden import GOLDEN
from tests.test_variants_parity import FIX, _state_dict

ALL = [(c, r) for c in M.CASES for r in M.regimes(c)]
POLICY = [(c, r) for c, r in ALL if not M.CASES[c]["value"]]


def _masks(case):
    return ("none",) if M.CASES[case]["value"] else M.MASKS


# ---- chain64 is the reference's arithmetic ----------------------------------------------------------------------------------------
def _layers(sd, prefix, out_tanh=False):
    ls, i = [], 0
    while f"{prefix}_layers.{i}.linear.weight" in sd:
        ls.append((sd[f"{prefix}_layers.{i}.linear.weight"].T, sd[f"{prefix}_layers.{i}.linear.bias"], 1))
        i += 1
    return ls + [(sd[f"{prefix}_output_layers.0.linear.weight"].T, sd[f"{prefix}_output_layers.0.linear.bias"], int(out_tanh))]


@pytest.mark.parametrize("name,N", FIX)
def test_chain64_rebuilds_the_reference_recordings(name, N):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    obs = z["obs"]
    S = obs.shape[0]
    dec, cent, gb = (_state_dict(z, t) for t in ("dec", "cent", "gb"))
    chains = {"dec": (_layers(dec, "encoder.", out_tanh=True) + _layers(dec, ""), obs.reshape(S * N, -1), 1),
              "cent": (_layers(cent, ""), obs, N)}
    for tag, (layers, x, groups) in chains.items():
        lg = M.chain64(x, layers)
        for suffix, av in (("", None), ("_masked", z["avail_masked"])):
            p = M.probs64(lg, av, groups, 5).reshape(S, N, 5)
            np.testing.assert_allclose(p, z[f"{tag}.probs{suffix}"], rtol=1e-5, atol=0, err_msg=f"{tag}{suffix}")
    v = M.chain64(obs, _layers(gb, "module._mean_module."))[:, 0]
    np.testing.assert_allclose(v, z["gb.values"], rtol=1e-5, atol=0)


# ---- each regime took hold ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,regime", ALL)
def test_regime_took_hold(case, regime):
    c, d = M.CASES[case], M.build(case, regime)
    if not c["value"]:
        for mask in M.MASKS:
            ref = M.reference(case, regime, mask)
            top = ref["probs"].max()
            if regime == "init":                             # (of the unmasked rows: the single-action row is 1 by construction)
                if mask == "none":
                    assert top < 0.6, f"{case} init: a probability of {top:.3f}"
            else:
                assert ref["M"] >= 20 and top > 0.99, f"{case} {regime} {mask}: max|logit64| {ref['M']:.1f}, top probability {top:.4f}"
                assert abs(ref["M"] - M.PEAK) < 1e-3
    if regime == "sat" and len(c["out_dim"]) > 1:
        a0 = M.chain64(d["x"], d["layers"], upto=0)
        i0 = M.chain64(d["x"], M.build(case, "init")["layers"], upto=0)
        if c["act"][0] == 1:
            frac = float((np.abs(a0) > 0.99).mean())
            assert frac >= 0.30 and float((np.abs(i0) > 0.99).mean()) < 0.01, f"{case}: {frac:.2f} of the first layer's tanh units above 0.99"
        else:
            assert c["act"][0] == 2
            frac = float((a0 > 1.0).mean())
            assert frac >= 0.30 and float((i0 > 1.0).mean()) < 0.01, f"{case}: {frac:.2f} of the first layer's ReLU units above 1"


# ---- the inputs are fair --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,regime", ALL)
def test_float32_alone_stays_within_half_of_every_bar(case, regime):
    for mask in _masks(case):
        m = M.float32_alone(case, regime, mask)
        print(f"{case} {regime} {mask}: " + ", ".join(f"{k} {v:.3g}" for k, v in m.items() if not k.startswith("n_")))
        assert not [k for k, v in m.items() if k.startswith("n_") and v], m
        assert M.worst_applied(m) <= 0.5, f"{case} {regime} {mask}: float32 alone at {M.worst_applied(m):.2f} of a bar: {m}"


# ---- the sampler condition --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["init", "peaked", "sat"])
def test_next_to_no_draw_is_undecided(regime):
    for mask in M.MASKS:
        refs = [M.reference(c, regime, mask) for c, r in POLICY if r == regime]
        near = np.concatenate([r["near"] for r in refs])
        und = np.concatenate([r["undecided"] for r in refs])
        print(f"{regime} {mask}: {near.sum()} of {near.size} draws near a boundary, {und.sum()} rows with undecided top two")
        assert near.mean() <= 0.01 and und.mean() <= 0.01


def test_uniforms_are_the_oracles_stream():
    """uniforms() against the oracle's sampler on a probability row whose CDF boundaries are the uniforms' bins: flat agent row ->
    (env, agent) as the kernel maps it, step = POLICY_STEP + STEP_BASE."""
    from oracle import oracle as O
    case = "obsdp_a3"
    c = M.CASES[case]
    u = M.uniforms(case)
    p = np.tile(np.float32([0.25, 0.25, 0.25, 0.25]), (M.envs_of(case), c["agents"], 1))
    a = O.sample_actions(p, M.SEED, M.ENV_ID_OFFSET, M.POLICY_STEP + M.STEP_BASE).reshape(-1)
    np.testing.assert_array_equal(a, np.floor(u * 4).astype(np.int64))
    assert len(np.unique(u)) == u.size


# ---- negative controls ----------------------------------------------------------------------------------------------------------------
def _swap(layers, l, wt=None, b=None, act=None):
    out = list(layers)
    w0, b0, a0 = out[l]
    out[l] = (w0 if wt is None else wt, b0 if b is None else b, a0 if act is None else act)
    return out


def _judge_wrong(case, regime, mask, layers):
    ref, wrong = M.reference(case, regime, mask), M.reference(case, regime, mask, layers=layers)
    if M.CASES[case]["value"]:
        return M.judge(case, ref, values=wrong["v"]), np.array_equal(wrong["v"], ref["v"])
    same = np.array_equal(wrong["probs"], ref["probs"])
    return M.judge(case, ref, probs=wrong["probs"], actions=wrong["actions"], greedy=wrong["greedy"]), same


def _without_input_column(layers, k):
    wt = np.array(layers[0][0])
    wt[k] = 0.0
    return _swap(layers, 0, wt=wt)


@pytest.mark.parametrize("case,regime", ALL)
def test_a_missing_input_column_is_rejected(case, regime):
    layers = M.build(case, regime)["layers"]
    K = M.CASES[case]["in_dim"]
    for mask in _masks(case):
        for k in [K - 1] + ([128] if K > 128 else []):
            m, same = _judge_wrong(case, regime, mask, _without_input_column(layers, k))
            assert M.rejected(m) and not same, f"{case} {regime} {mask}: layer 0 without input column {k} passes: {m}"


def test_the_column_128_control_covers_maxlds_and_one_300_128():
    assert M.CASES["maxlds"]["in_dim"] == 129 and M.CASES["one_300_128"]["in_dim"] > 128


@pytest.mark.parametrize("case,regime", ALL)
def test_a_dropped_bias_of_the_last_column_tile_is_rejected(case, regime):
    layers = M.build(case, regime)["layers"]
    b = layers[-1][1]
    for mask in _masks(case):
        if b is None:                                        # nobias: nothing to drop, the wrong answer is the right one
            assert case == "nobias"
            continue
        wrong = np.array(b)
        wrong[16 * ((len(b) - 1) // 16):] = 0.0
        m, same = _judge_wrong(case, regime, mask, _swap(layers, len(layers) - 1, b=wrong))
        assert M.rejected(m) and not same, f"{case} {regime} {mask}: the last tile's bias dropped passes: {m}"


@pytest.mark.parametrize("case,regime", [(c, r) for c, r in ALL if 2 in M.CASES[c]["act"]])
def test_tanh_for_relu_is_rejected(case, regime):
    layers = [(w, b, 1 if a == 2 else a) for w, b, a in M.build(case, regime)["layers"]]
    for mask in _masks(case):
        m, same = _judge_wrong(case, regime, mask, layers)
        assert M.rejected(m) and not same, f"{case} {regime} {mask}: tanh in place of ReLU passes: {m}"


def test_the_relu_cases_are_the_three():
    assert sorted(c for c in M.CASES if 2 in M.CASES[c]["act"]) == ["relu3", "six", "val_wide"]


@pytest.mark.parametrize("case,regime", POLICY)
def test_a_skipped_renormalisation_is_rejected(case, regime):
    c, ref = M.CASES[case], M.reference(case, regime, "avail")
    p = M.probs64(ref["logits"], ref["avail"], c["groups"], c["n_act"], renormalise=False)
    m = M.judge(case, ref, probs=p)
    # (a peaked row whose forbidden action had next to no mass still sums to 1 within 1e-6: the single-action row is what always tells)
    assert set(M.rejected(m)) & {"n_rows_not_summing_to_1", "n_single_action_row_not_1"}, m
    if regime == "init":
        assert "n_rows_not_summing_to_1" in M.rejected(m), m


# (case, regime, mask) where the previous agent row's probabilities give the last agent row's uniform the same action AND have the same
# first maximum: the wrong answer coincides with the right one there.  From float64 alone; filled from the run that printed them.
COINCIDES_PREV_ROW = {("one_21_5", "init", "none"), ("one_21_5", "peaked", "none"), ("one_21_5", "peaked", "avail")} | {
    ("obsdp_a3", r, m) for r in ("init", "peaked", "sat") for m in M.MASKS}
# obsdp_a3's last two agent rows agree in every regime (three actions, one of them dominant): the control shows nothing there; `nobias`,
# the same shape with other weights, rejects it in all six
NEVER_REJECTS_PREV_ROW = {"obsdp_a3"}


@pytest.mark.parametrize("case", sorted({c for c, _ in POLICY}))
def test_the_previous_rows_probabilities_are_rejected(case):
    from tests import acting_regimes as G
    u = M.uniforms(case)
    n_rejected = 0
    for regime in M.regimes(case):
        for mask in M.MASKS:
            ref = M.reference(case, regime, mask)
            assert not ref["near"][-1] and not ref["undecided"][-1], f"{case} {regime} {mask}: the last agent row is not judged"
            acts, greedy = ref["actions"].copy(), ref["greedy"].copy()
            acts[-1] = G.cdf_actions64(ref["probs"][-2], u[-1])
            greedy[-1] = M.first_max(ref["probs"][-2])
            m = M.judge(case, ref, probs=ref["probs"], actions=acts, greedy=greedy)
            same = acts[-1] == ref["actions"][-1] and greedy[-1] == ref["greedy"][-1]
            print(f"{case} {regime} {mask}: {'coincides' if same else 'rejected by ' + ', '.join(M.rejected(m))}")
            assert same == ((case, regime, mask) in COINCIDES_PREV_ROW), (case, regime, mask, same)
            assert bool(M.rejected(m)) == (not same), m
            n_rejected += not same
    assert bool(n_rejected) == (case not in NEVER_REJECTS_PREV_ROW), f"{case}: rejected in {n_rejected} regime and mask settings"


def test_the_right_answer_passes():
    """judge() on the reference itself: every ratio 0, every count 0 (a judge that rejects everything would pass every control)."""
    for case, regime in ALL:
        for mask in _masks(case):
            ref = M.reference(case, regime, mask)
            if M.CASES[case]["value"]:
                m = M.judge(case, ref, values=ref["v"])
            else:
                m = M.judge(case, ref, probs=ref["probs"], actions=ref["actions"], greedy=ref["greedy"], logits=ref["logits"])
            assert not M.rejected(m) and M.worst_applied(m) == 0, (case, regime, mask, m)
