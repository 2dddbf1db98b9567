"""eval_summary / eval_sweep with ci= and contrast=: bootstrap intervals, standard errors and paired contrasts of every score,
against the numpy reference (tests/boot_ref.py) applied to the episode tables the same call returns - under the comparison rules
of tests/test_boot_kernels.py - with all four statistics families on.  The shape is test_eval_sweep's pp4: 2 policies x 3
conditions x 8 envs, 12 episodes a cell (a second round that takes 4), 20 steps; co24 for the Coverage summary."""
import numpy as np
import pytest

from tests import boot_ref as R
from tests import test_eval_sweep as S
from tests import test_value_stats as V
from tests.lib_spy import spy as lib_spy  # noqa: F401  (the fixture: a recording proxy around _lib.lib())

pytestmark = pytest.mark.gpu

K, E, N_EPI, T = S.K, S.E, S.N_EPI, S.T
LEVEL, N_BOOT, SEED = 0.9, 257, 6
DERIVED = {"columns": (), "comm": (4,), "value": (3, 4)}


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch


def _tables(families):
    """-> [(the dicts' table key, kind, names)] of the summary and the active families, in the launches' order."""
    from com_marl_amd import evaluate as ev
    every = dict(comm=("comm_episodes", "comm", ev.COMM_KEYS), attn=("attn_episodes", "columns", ev.ATTN_KEYS),
                 listen=("listen_episodes", "columns", ev.LISTEN_KEYS), value=("value_episodes", "value", ev.VALUE_KEYS))
    return [("episodes", "columns", ["success"] + ev.VECTORS)] + [every[f] for f in families]


def _setup(shape="pp4", families=("comm", "attn", "listen", "value"), same_policy=False):
    """A fresh wrapper of the shape, its K policies (one twice with same_policy) and the switches of the families with their critics."""
    scen, params, channel, conds = S.SHAPES[shape]
    env = S._wrapper(scen, params, K * len(conds) * E, channel, conditions=conds)
    pols = S._policies(env, K)
    kw = {f + "_stats": True for f in families}
    if "value" in families:
        kw["baselines"] = V._critics(env, K)
    if same_policy:
        pols = [pols[0]] * K
        if "value" in families:
            kw["baselines"] = [kw["baselines"][0]] * K
    return env, pols, conds, kw


def _cells(res):
    return [d for row in res for d in row] if isinstance(res[0], list) else list(res)


def _check(cells, families, n_boot, level, seed, ref=None):
    """Every cell's ci / se (ref None) or contrast (ref: per cell the cell it is compared with) against the reference on the cells'
    own episode tables."""
    lo, hi = R.ranks(level, n_boot)
    covered = set()
    for key, kind, names in _tables(families):
        table = np.stack([d[key].cpu().numpy() for d in cells])
        assert table.shape[1:] == (N_EPI, {"episodes": 9, "comm_episodes": 4}.get(key, 6))
        want, v = R.quantiles(R.means(table, n_boot, seed), lo, hi, kind, ref)
        got = want.copy()                                       # (p_gt is the contrast's alone: the reference's own otherwise)
        for g, d in enumerate(cells):
            for i, name in enumerate(names):
                if ref is None:
                    got[g, i, :3] = [*d["ci"][name], d["se"][name]]
                else:
                    c = d["contrast"][name]
                    got[g, i] = [c["lo"], c["hi"], c["se"], c["p_gt"]]
                    assert c["diff"] == d[name] - cells[ref[g]][name], (g, name)
                    assert set(c) == {"diff", "lo", "hi", "se", "p_gt"}
        R.check_out(got, want, v, DERIVED[kind], key)
        print(f"{key}: max |got - want| {np.abs(got - want).max():.3e}")
        covered |= set(names)
    for d in cells:
        assert set(d["ci"]) == covered and set(d["se"]) == covered
        assert all(isinstance(x, float) for pair in d["ci"].values() for x in pair) and all(lo_ <= hi_ for lo_, hi_ in d["ci"].values())
        assert not covered & {"return_std", "return_min", "return_max", "bound_return", "curves"}
        if ref is not None:
            assert set(d["contrast"]) == covered


def _same_but(a, b, extra, torch):
    assert set(a) == set(b) | extra
    for key, v in b.items():
        if torch.is_tensor(v):
            assert torch.equal(a[key], v), key
        elif isinstance(v, dict) and key == "curves":
            assert set(a[key]) == set(v) and all(np.array_equal(a[key][n], v[n]) for n in v), key
        else:
            assert a[key] == v, key


def _boot_calls(spy):
    return spy.count("cm_boot_means"), spy.count("cm_boot_quantiles")


def test_off_launches_nothing_and_on_changes_nothing_else(gpu, lib_spy):  # noqa: F811
    from com_marl_amd.evaluate import eval_sweep
    env, pols, conds, kw = _setup()
    plain = eval_sweep(env, pols, 0, n_eval_episodes=N_EPI, max_env_steps=T, episodes=True, curves=True, **kw)
    assert not [c for c in lib_spy.calls if c.startswith("cm_boot")]
    assert all("ci" not in d and "se" not in d and "contrast" not in d for d in _cells(plain))
    env, pols, conds, kw = _setup()
    lib_spy.calls.clear()
    on = eval_sweep(env, pols, 0, n_eval_episodes=N_EPI, max_env_steps=T, episodes=True, curves=True, ci=LEVEL, n_boot=N_BOOT, **kw)
    assert _boot_calls(lib_spy) == (5, 5)                       # one of each per table: the summary and the four families
    order = [c for c in lib_spy.calls if c != "cm_env_destroy"]          # (a collected wrapper of an earlier test)
    assert order[-10:] == ["cm_boot_means", "cm_boot_quantiles"] * 5     # behind every other launch of the call
    assert [c.args[5] for c in lib_spy.calls if c == "cm_boot_quantiles"] == [None] * 5
    for a, b in zip(_cells(on), _cells(plain)):
        _same_but(a, b, {"ci", "se"}, gpu)
    _check(_cells(on), ("comm", "attn", "listen", "value"), N_BOOT, LEVEL, 0)


def test_intervals_equal_the_reference_on_the_returned_tables(gpu):
    from com_marl_amd.evaluate import eval_sweep
    env, pols, conds, kw = _setup()
    got = eval_sweep(env, pols, 0, n_eval_episodes=N_EPI, max_env_steps=T, episodes=True, ci=0.95, n_boot=2000, boot_seed=SEED, **kw)
    cells = _cells(got)
    _check(cells, ("comm", "attn", "listen", "value"), 2000, 0.95, SEED)
    for d in cells:                                             # the point estimate of a mean lies in its own interval
        for name in ("reward", "step_cnt", "nodeDeg", "range_degree", "attn_entropy", "value_return"):
            assert d["ci"][name][0] <= d[name] <= d["ci"][name][1], (name, d[name], d["ci"][name])
    assert any(d["se"]["reward"] > 0 for d in cells)
    # another seed, other resamples; the same seed, the same bits
    env, pols, conds, kw = _setup()
    again = eval_sweep(env, pols, 0, n_eval_episodes=N_EPI, max_env_steps=T, episodes=True, ci=0.95, n_boot=2000, boot_seed=SEED, **kw)
    assert all(a["ci"] == b["ci"] and a["se"] == b["se"] for a, b in zip(_cells(again), cells))
    env, pols, conds, kw = _setup()
    other = eval_sweep(env, pols, 0, n_eval_episodes=N_EPI, max_env_steps=T, ci=0.95, n_boot=2000, boot_seed=SEED + 1, **kw)
    assert any(a["se"] != b["se"] for a, b in zip(_cells(other), cells))


def test_eval_summary_of_two_policies_resamples_every_policy_alike(gpu, lib_spy):  # noqa: F811
    from com_marl_amd.evaluate import eval_summary
    scen, params, channel, _ = S.SHAPES["pp4"]
    env = S._wrapper(scen, params, K * E, channel)
    pols = S._policies(env, K)
    lib_spy.calls.clear()
    got = eval_summary(env, pols, 0, n_eval_episodes=N_EPI, max_env_steps=T, episodes=True, comm_stats=True, attn_stats=True,
                       listen_stats=True, value_stats=True, baselines=V._critics(env, K), ci=LEVEL, n_boot=N_BOOT, boot_seed=SEED)
    assert _boot_calls(lib_spy) == (5, 5)
    for d in got:                                               # each policy alone: its cell index plays no part in the resamples
        _check([d], ("comm", "attn", "listen", "value"), N_BOOT, LEVEL, SEED)
    _check(got, ("comm", "attn", "listen", "value"), N_BOOT, LEVEL, SEED)
    one = eval_summary(S._wrapper(scen, params, E, channel), pols[0], 0, n_eval_episodes=N_EPI, max_env_steps=T, ci=LEVEL, n_boot=N_BOOT,
                       boot_seed=SEED)
    from com_marl_amd.evaluate import VECTORS
    assert set(one["ci"]) == set(["success"] + VECTORS) == set(one["se"])      # no family on: the summary's nine names
    assert one["ci"] == {name: got[0]["ci"][name] for name in one["ci"]}


@pytest.mark.parametrize("axis", ["condition", "policy"])
def test_contrasts_equal_the_reference_and_cost_one_launch_per_table(gpu, lib_spy, axis):  # noqa: F811
    from com_marl_amd.evaluate import eval_sweep
    env, pols, conds, kw = _setup()
    Cn = len(conds)
    lib_spy.calls.clear()
    got = eval_sweep(env, pols, 0, n_eval_episodes=N_EPI, max_env_steps=T, episodes=True, ci=LEVEL, n_boot=N_BOOT, boot_seed=SEED,
                     contrast={axis: 0}, **kw)
    assert _boot_calls(lib_spy) == (5, 10)                      # one more cm_boot_quantiles per table
    assert [c.args[5] is None for c in lib_spy.calls if c == "cm_boot_quantiles"] == [True, False] * 5
    ref = [(g // Cn) * Cn if axis == "condition" else g % Cn for g in range(K * Cn)]
    cells = _cells(got)
    _check(cells, ("comm", "attn", "listen", "value"), N_BOOT, LEVEL, SEED)
    _check(cells, ("comm", "attn", "listen", "value"), N_BOOT, LEVEL, SEED, ref)
    for g, d in enumerate(cells):
        assert d["contrast_ref"] == (ref[g] // Cn, ref[g] % Cn)
        if ref[g] == g:                                         # the reference cells: exact zeros
            assert all(c == dict(diff=0.0, lo=0.0, hi=0.0, se=0.0, p_gt=0.5) for c in d["contrast"].values()), d["contrast"]
    others = [d for g, d in enumerate(cells) if ref[g] != g]
    assert any(c["diff"] != 0 and c["se"] > 0 for d in others for c in d["contrast"].values())


def test_the_same_policy_twice_pins_the_pairing(gpu):
    """Row e of every cell is the same scenario: two rows of cells playing ONE policy hold identical episode tables, so every contrast
    against the first row is exactly zero."""
    from com_marl_amd.evaluate import eval_sweep
    env, pols, conds, kw = _setup(same_policy=True)
    got = eval_sweep(env, pols, 0, n_eval_episodes=N_EPI, max_env_steps=T, episodes=True, ci=LEVEL, n_boot=N_BOOT,
                     contrast=dict(policy=0), **kw)
    for c in range(len(conds)):
        for key, _, _ in _tables(("comm", "attn", "listen", "value")):
            assert gpu.equal(got[0][c][key], got[1][c][key]), (c, key)
        for k in range(K):
            assert got[k][c]["contrast_ref"] == (0, c)
            assert all(v == dict(diff=0.0, lo=0.0, hi=0.0, se=0.0, p_gt=0.5) for v in got[k][c]["contrast"].values()), got[k][c]["contrast"]
        assert got[0][c]["ci"] == got[1][c]["ci"] and got[0][c]["se"] == got[1][c]["se"]
    assert got[0][0]["ci"] != got[0][2]["ci"]                   # (the conditions differ)


def test_refusals_on_a_real_wrapper_launch_nothing(gpu, lib_spy):  # noqa: F811
    from com_marl_amd.evaluate import eval_summary, eval_sweep
    env, pols, conds, kw = _setup(families=("comm",))
    lib_spy.calls.clear()
    run = dict(n_eval_episodes=N_EPI, max_env_steps=T, **kw)
    for bad, match in ((dict(ci=1.0), "ci="), (dict(ci=0.9, n_boot=4097), "n_boot="), (dict(ci=0.9, boot_seed=-1), "boot_seed="),
                       (dict(n_boot=100), "n_boot="), (dict(contrast=dict(policy=0)), "contrast="),
                       (dict(ci=0.9, contrast=dict(policy=0), paired=False), "paired=True"),
                       (dict(ci=0.9, contrast=dict(policy=K)), "contrast="), (dict(ci=0.9, contrast=dict(condition=len(conds))), "contrast="),
                       (dict(ci=0.9, contrast=dict(policy=0, condition=0)), "contrast=")):
        with pytest.raises(ValueError, match=match):
            eval_sweep(env, pols, 0, **run, **bad)
    with pytest.raises(ValueError, match="contrast="):
        eval_summary(env, pols, 0, ci=0.9, contrast=dict(policy=0), **run)
    assert not [c for c in lib_spy.calls if c != "cm_env_destroy"]


def test_coverage_summary_of_nine_columns(gpu, lib_spy):  # noqa: F811
    """co24 with comm_stats alone: the Coverage scenario fills every one of the nine summary columns (vars2 too)."""
    from com_marl_amd.evaluate import eval_sweep
    env, pols, conds, kw = _setup("co24", families=("comm",))
    lib_spy.calls.clear()
    got = eval_sweep(env, pols, 0, n_eval_episodes=N_EPI, max_env_steps=T, episodes=True, ci=LEVEL, n_boot=N_BOOT, boot_seed=SEED,
                     contrast=dict(condition=1), **kw)
    assert _boot_calls(lib_spy) == (2, 4)
    cells = _cells(got)
    Cn = len(conds)
    _check(cells, ("comm",), N_BOOT, LEVEL, SEED)
    _check(cells, ("comm",), N_BOOT, LEVEL, SEED, [(g // Cn) * Cn + 1 for g in range(K * Cn)])
    assert any(d["se"]["vars2"] > 0 for d in cells) and all(d["contrast_ref"][1] == 1 for d in cells)
