"""The numpy float64 restatement of the critic statistics (tests/value_stats_ref.py) on hand cases, its reducers against plain loops
written out here, and what answers without a GPU: the symbols, the keywords, the refusals, the layout of the summary buffer."""
import ctypes as C
import inspect
import math
import os

import numpy as np
import pytest

from tests import value_stats_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["cm_value_stats", "cm_episode_value", "cm_value_means", "cm_value_curves", "cm_value_curve_means"]
f32 = np.float32


def _one_env(r, n_end=None):
    """Rewards of one env -> (rewards [T,1], path_len [T,1] ending the episode at step n_end - 1 when given)."""
    r = np.asarray(r, np.float64)[:, None]
    pl = np.zeros(r.shape, np.int32)
    if n_end is not None:
        pl[n_end - 1, 0] = n_end
    return r, pl


def _episode_keys(stats, n):
    return R.keys(stats[:n, 0].sum(0) / n)


def test_a_perfect_critic_has_no_error_and_explains_everything():
    r, pl = _one_env([1.0, 2.0, -4.0, 8.0, 0.5])
    G = np.array([0.5 * (0.5 * (0.5 * (0.5 * 0.5 + 8.0) - 4.0) + 2.0) + 1.0, 0.5 * (0.5 * (0.5 * 0.5 + 8.0) - 4.0) + 2.0,
                  0.5 * (0.5 * 0.5 + 8.0) - 4.0, 0.5 * 0.5 + 8.0, 0.5])                # gamma = 0.5: exact in f32 and f64
    v = G.astype(f32)[:, None]
    assert (v.astype(np.float64)[:, 0] == G).all()
    out = R.value_stats(r, pl, v, None, None, 0.5)
    assert (out[:, 0, 1] == G).all() and (out[:, 0, 0] == G).all()
    assert (out[:, 0, 2] == 0).all() and (out[:, 0, 3] == G * G).all() and (out[:, 0, 4:] == 0).all()
    k = _episode_keys(out, 5)
    assert k["value_rmse"] == 0.0 and k["value_bias"] == 0.0 and k["value_ev"] == 1.0


def test_an_all_zero_critic_on_returns_that_vary_explains_nothing():
    r, pl = _one_env([1.0, 2.0, 3.0, 4.0])
    out = R.value_stats(r, pl, np.zeros((4, 1), f32), None, None, 1.0)
    k = _episode_keys(out, 4)
    assert k["value_mean"] == 0.0 and k["value_bias"] == -k["value_return"] and k["value_return"] == (10 + 9 + 7 + 4) / 4
    assert k["value_ev"] == pytest.approx(0.0, abs=1e-15)
    assert k["value_rmse"] == pytest.approx(math.sqrt((100 + 81 + 49 + 16) / 4), rel=1e-15)
    # a critic that is anti-correlated with the returns is worse than a constant: negative
    worse = R.value_stats(r, pl, -out[:, :, 1].astype(f32), None, None, 1.0)
    assert _episode_keys(worse, 4)["value_ev"] < -1


def test_constant_returns_take_the_degenerate_rule():
    r, pl = _one_env([0.0, 0.0, 0.0, 2.0])                              # gamma = 1: G = 2 at every step
    same = R.value_stats(r, pl, np.full((4, 1), 7.0, f32), None, None, 1.0)
    k = _episode_keys(same, 4)
    assert k["value_return"] == 2.0 and k["value_bias"] == 5.0 and k["value_rmse"] == 5.0
    assert k["value_ev"] == 1.0                                         # a constant critic on constant returns: nothing left unexplained
    noisy = R.value_stats(r, pl, np.array([[1.0], [3.0], [1.0], [3.0]], f32), None, None, 1.0)
    k = _episode_keys(noisy, 4)
    assert k["value_bias"] == 0.0 and k["value_rmse"] == 1.0 and k["value_ev"] == 0.0
    # the threshold scales with E[G^2]: a variance of rounding size next to large returns is degenerate too
    assert R.explained(0.0, 0.0, 1e6, 1e12 * (1 + 1e-15)) == 1.0 and R.explained(4.0, 0.0, 1e6, 1e12 * (1 + 1e-15)) == 0.0
    assert R.explained(0.5, 0.0, 0.0, 1.0) == 0.5


def test_gamma_zero_gives_the_rewards_and_gamma_one_the_suffix_sums():
    rng = np.random.default_rng(0)
    r = rng.standard_normal((9, 3))
    pl = np.zeros((9, 3), np.int32)
    pl[5, 1] = 6                                                        # env 1: n = 6
    pl[0, 2] = 1                                                        # env 2: n = 1
    v = rng.standard_normal((9, 3)).astype(f32)
    zero = R.value_stats(r, pl, v, None, None, 0.0)
    one = R.value_stats(r, pl, v, None, None, 1.0)
    for b, n in ((0, 9), (1, 6), (2, 1)):
        assert (zero[:n, b, 1] == r[:n, b]).all()
        want = [math.fsum(r[t:n, b]) for t in range(n)]
        np.testing.assert_allclose(one[:n, b, 1], want, rtol=1e-14, atol=1e-15)
        for out in (zero, one):
            assert out[n - 1, b, 1] == r[n - 1, b]                      # the last step's return is its reward, whatever gamma is
            assert (out[n:, b] == 0).all() and not np.signbit(out[n:, b]).any()      # rows behind the episode: zeros
            assert (out[:n, b, 0] == v[:n, b].astype(np.float64)).all()


def test_counterfactual_columns_and_none():
    r, pl = _one_env([1.0, 1.0, 1.0], n_end=2)
    v, m, l = (np.array(x, f32)[:, None] for x in ([2.0, 3.0, 9.0], [0.5, 3.0, 9.0], [2.25, 2.0, 9.0]))
    out = R.value_stats(r, pl, v, m, l, 0.99)
    assert out[:2, 0, 4].tolist() == [1.5, 0.0] and out[:2, 0, 5].tolist() == [0.25, -1.0] and (out[2] == 0).all()
    assert (R.value_stats(r, pl, v, None, l, 0.99)[..., 4] == 0).all()
    assert (R.value_stats(r, pl, v, m, None, 0.99)[..., 5] == 0).all()
    np.testing.assert_array_equal(R.value_stats(r, pl, v, None, None, 0.99)[..., :4], out[..., :4])


def test_seeded_inputs_hold_the_cases_the_tests_name():
    for kind, T, B in (("none", 7, 5), ("all0", 7, 5), ("mixed", 70, 9), ("mixed", 1, 1)):
        r, pl, v, m, l = R.seeded(T, B, kind, seed=5)
        assert r.dtype == np.float64 and pl.dtype == np.int32 and v.dtype == m.dtype == l.dtype == f32
        assert r.shape == pl.shape == v.shape == m.shape == l.shape == (T, B)
        lengths = [R.episode_length(pl[:, b]) for b in range(B)]
        if kind == "none":
            assert lengths == [T] * B
        if kind == "all0":
            assert lengths == [1] * B
        if kind == "mixed" and T > 1:
            assert len(set(lengths)) > 2 and T in lengths
        out = R.value_stats(r, pl, v, m, l, 0.99)
        assert np.isfinite(out).all()
        if B > 1:
            assert (out[:, 1, 5] == 0).all()
        atol = R.env_atol(r, v)
        assert atol.shape == (B, 6) and np.allclose(atol[:, 2], atol[:, 0] ** 2 * 1e12, rtol=1e-14, atol=0) and (atol >= 1e-12).all()


def test_reducers_equal_plain_loops():
    T, B = 5, 6
    rng = np.random.default_rng(7)
    stats = rng.standard_normal((T, B, R.VALUE_COLS))
    path_len = np.zeros((T, B), np.int32)
    path_len[2, 0] = 3                                                   # env 0: n = 3
    path_len[0, 1] = 1                                                   # env 1: n = 1
    path_len[4, 3] = 5                                                   # env 3: n = 5 (ends at the last step)
    path_len[1, 4], path_len[3, 4] = 2, 2                                # env 4: n = 2, the second end is another episode
    lengths = [3, 1, T, 5, 2, T]
    episodes = np.full((2 * 4, R.EPV_COLS), -1.0)
    R.episode_value(path_len, stats, 3, 2, 4, 1, episodes)               # groups of 3, take 2, rows 1 .. 2 of 4
    for k in range(2):
        for j in range(2):
            b = 3 * k + j
            want = sum(stats[t, b] for t in range(lengths[b])) / lengths[b]       # ONE divisor, n, for all six columns
            np.testing.assert_allclose(episodes[4 * k + 1 + j], want, rtol=1e-15)
        assert (episodes[4 * k] == -1).all() and (episodes[4 * k + 3] == -1).all()
    np.testing.assert_allclose(R.value_means(episodes.reshape(2, 4, 6)), episodes.reshape(2, 4, 6).sum(1) / 4, rtol=1e-15)

    sums = np.full((2, T, R.VALUE_COLS), -1.0)
    R.value_curves(path_len, stats, 3, 2, 0, sums)                       # overwrites
    np.testing.assert_allclose(sums[0, 0], stats[0, 0] + stats[0, 1], rtol=1e-15)
    np.testing.assert_array_equal(sums[0, 1], stats[1, 0])               # env 1 has ended: it adds nothing
    np.testing.assert_array_equal(sums[0, 3], 0.0)                       # both have
    np.testing.assert_allclose(sums[1, 1], stats[1, 3] + stats[1, 4], rtol=1e-15)
    np.testing.assert_array_equal(sums[1, 2], stats[2, 3])
    first = sums.copy()
    R.value_curves(path_len, stats, 3, 2, 1, sums)                       # adds
    np.testing.assert_allclose(sums, 2 * first, rtol=1e-15)
    np.testing.assert_array_equal(R.value_curve_means(sums, 4), sums / 4.0)
    assert R.value_curves(path_len, stats, 3, 0, 0, sums.copy()).tolist() == sums.tolist()      # take = 0: untouched


def test_curve_keys_are_taken_over_the_episodes_still_running():
    # two episodes: both run at step 0, one at step 1, none at step 2
    rows = np.zeros((3, 2, 6))
    rows[0, 0], rows[0, 1], rows[1, 0] = [1, 3, 4, 9, .5, .25], [5, 3, 4, 9, .5, .25], [2, 2, 0, 4, 1, 1]
    curves = rows.sum(1) / 2
    got = R.curve_keys(curves, np.array([1.0, 0.5, 0.0]))
    assert got["value_mean"].tolist() == [3.0, 1.0, 0.0] and got["value_return"].tolist() == [3.0, 1.0, 0.0]
    assert got["msg_value"].tolist() == [0.5, 0.5, 0.0] and got["loss_value"].tolist() == [0.25, 0.5, 0.0]
    assert got["value_rmse"].tolist() == [2.0, 0.0, 0.0]                 # sqrt(4), sqrt(0 / 0.5), nothing runs
    assert got["value_ev"].tolist() == [0.0, 1.0, 1.0]                   # constant returns: 0 with an error left, 1 without; 1 where none runs
    from com_marl_amd.evaluate import FAMILIES, VALUE_KEYS
    value = FAMILIES["value_stats"]
    mine = value.curve_keys(np.ascontiguousarray(curves.T), np.array([1.0, 0.5, 0.0]))
    assert list(mine) == VALUE_KEYS == R.KEYS
    for k in R.KEYS:
        np.testing.assert_array_equal(mine[k], got[k], err_msg=k)
    rng = np.random.default_rng(3)
    for _ in range(20):
        v, g = rng.standard_normal(7), rng.standard_normal(7)
        row = [v.mean(), g.mean(), ((v - g) ** 2).mean(), (g * g).mean(), 0.25, -0.5]
        a, b = value.keys(row), R.keys(row)
        assert a == b and list(a) == R.KEYS
        assert a["value_ev"] == pytest.approx(1 - np.var(g - v) / np.var(g), rel=1e-9)


def test_symbols_are_declared_bound_and_exported():
    from com_marl_amd import _lib as L, evaluate
    hdr = open(os.path.join(ROOT, "include", "commarl.h")).read()
    for name in SYMBOLS:
        assert name in L.EXPORTED and hasattr(L.lib(), name) and name + "(" in hdr
    assert "#define CM_VALUE_COLS 6" in hdr and "#define CM_EPV_COLS 6" in hdr
    assert (L.VALUE_COLS, L.EPV_COLS) == (R.VALUE_COLS, R.EPV_COLS) == (6, 6)
    assert evaluate.VALUE_KEYS == R.KEYS
    assert "cm_value_stats.hip" in open(os.path.join(ROOT, "com-marl_amd", "csrc", "Makefile")).read()


def test_the_keywords_and_their_defaults():
    from com_marl_amd import envs, evaluate, nets, rollout
    for fn in (evaluate.eval_summary, evaluate.eval_sweep, evaluate._score):
        par = inspect.signature(fn).parameters
        assert list(par)[-3:] == ["value_stats", "baselines", "discount"]
        assert par["value_stats"].default is False
    for fn in (evaluate.eval_summary, evaluate.eval_sweep, evaluate._score):
        par = inspect.signature(fn).parameters
        assert par["baselines"].default is None and par["discount"].default == 0.99
        assert list(par).index("listen_stats") == len(par) - 4          # appended behind the existing keywords
    assert list(evaluate.FAMILIES)[-2:] == ["listen_stats", "value_stats"]      # the buffer's layout: the families in this order
    assert list(inspect.signature(envs.value_stats).parameters) == ["rewards", "path_len", "values", "mute", "lossless", "discount", "out"]
    assert inspect.signature(envs.value_stats).parameters["discount"].default == 0.99
    assert list(inspect.signature(rollout.RolloutEngine.replay_values).parameters) == ["self", "t0", "n", "channels", "critics", "out"]
    par = inspect.signature(nets.GaussianMLPBaseline.values_device).parameters
    assert list(par) == ["self", "obs", "out"] and par["out"].default is None


class _Policy:
    comm = True
    _n_agents, _dec_obs_dim = 4, 10


class _Critic:
    _n_agents, _dec_obs_dim = 4, 10

    def values_device(self, *a, **kw):
        raise AssertionError("refused before anything is built")


class _Baseline:                                                # (as GaussianMLPBaseline: the joint observation's width alone)
    input_dim = 40
    values_device = _Critic.values_device


def test_refusals_name_value_stats_before_anything_is_built():
    from com_marl_amd import evaluate
    wide, big = _Critic(), _Critic()
    wide._dec_obs_dim, big._n_agents = 11, 5
    narrow = _Baseline()
    narrow.input_dim = 44
    cases = [
        (_Policy(), dict(value_stats=True)),                                        # no baselines
        (_Policy(), dict(baselines=_Critic())),                                     # baselines without the switch
        ([_Policy(), _Policy()], dict(value_stats=True, baselines=[_Critic()])),    # lengths
        ([_Policy(), _Policy()], dict(value_stats=True, baselines=_Critic())),
        (_Policy(), dict(value_stats=True, baselines=[_Critic(), _Critic()])),
        (_Policy(), dict(value_stats=True, baselines=object())),                    # no values_device
        ([_Policy(), _Policy()], dict(value_stats=True, baselines=[_Critic(), _Baseline()])),   # classes
        (_Policy(), dict(value_stats=True, baselines=wide)),                        # observation width
        (_Policy(), dict(value_stats=True, baselines=big)),                         # team size
        (_Policy(), dict(value_stats=True, baselines=narrow)),
        (_Policy(), dict(value_stats=True, baselines=_Critic(), discount=1.5)),
        (_Policy(), dict(value_stats=True, baselines=_Critic(), discount=float("nan"))),
    ]
    for policies, kw in cases:
        with pytest.raises(ValueError, match="value_stats"):    # (the wrapper is never touched)
            evaluate.eval_summary(None, policies, **kw)
        with pytest.raises(ValueError, match="value_stats"):    # (eval_sweep behind its look at the wrapper's conditions)
            evaluate._score("eval_sweep", None, policies, 8, 6, True, None, False, False, conds=[{}], **kw)
    # what passes the checks goes on to the wrapper (None here)
    for policies, kw in ((_Policy(), dict(value_stats=True, baselines=_Critic())), (_Policy(), dict(value_stats=True, baselines=_Baseline())),
                         ([_Policy(), _Policy()], dict(value_stats=True, baselines=[_Critic(), _Critic()]))):
        with pytest.raises(AttributeError):
            evaluate.eval_summary(None, policies, **kw)


def test_summary_buffers_put_the_value_views_last_and_leave_the_others_where_they_were():
    """Restated on evaluate._layout, for every combination of the four family switches and curves: every active section at the
    byte offset the buffer's order gives it - summary, comm, curves, comm curves, attn, attn curves, listen, listen curves, value,
    value curves - no section for what is off, and the host slices on the same bytes as the device views."""
    import itertools
    import torch
    from com_marl_amd import _lib as L
    from com_marl_amd.evaluate import FAMILIES, _cut, _layout
    cells, T = 3, 5
    for comm, attn, listen, value, curves in itertools.product((False, True), repeat=5):
        on = dict(comm_stats=comm, attn_stats=attn, listen_stats=listen, value_stats=value)
        layout = _layout(cells, T, [fam for switch, fam in FAMILIES.items() if on[switch]], curves)
        # the order written down: (name, shape, present)
        want = [("summary", (cells, L.SUM_COLS), True), ("comm", (cells, L.EPC_COLS), comm),
                ("curves", (cells, T, L.EPI_COLS), curves), ("comm_curves", (cells, T, L.EPC_COLS), comm and curves),
                ("attn", (cells, L.EPA_COLS), attn), ("attn_curves", (cells, T, L.EPA_COLS), attn and curves),
                ("listen", (cells, L.EPL_COLS), listen), ("listen_curves", (cells, T, L.EPL_COLS), listen and curves),
                ("value", (cells, L.EPV_COLS), value), ("value_curves", (cells, T, L.EPV_COLS), value and curves)]
        total = sum(int(np.prod(shape)) for _, shape, present in want if present)
        flat = torch.empty(total, dtype=torch.float64, device="cpu")
        device, host = _cut(flat, layout), _cut(flat.numpy(), layout)
        assert list(device) == list(host) == [name for name, _, present in want if present]     # nothing for what is off
        offset = 0
        for name, shape, present in want:
            if not present:
                continue
            assert tuple(device[name].shape) == host[name].shape == shape, name
            assert device[name].data_ptr() - flat.data_ptr() == 8 * offset, name
            assert host[name].ctypes.data == device[name].data_ptr() and host[name].flags["C_CONTIGUOUS"], name
            offset += int(np.prod(shape))
        assert offset == total


def test_argument_errors_answer_without_a_gpu():
    from com_marl_amd import _lib as L
    lib = L.lib()
    p = C.c_void_p(16)                                          # plausible, never dereferenced: the checks precede the launch

    def stats(T=3, B=4, r=p, pl=p, v=p, mu=p, lo=p, gamma=0.99, out=p):
        return lib.cm_value_stats(T, B, r, pl, v, mu, lo, gamma, out, None)

    for kw in (dict(T=-1), dict(B=-1), dict(gamma=-0.01), dict(gamma=1.0000001), dict(gamma=float("nan")), dict(gamma=float("inf")),
               dict(r=None), dict(pl=None), dict(v=None), dict(out=None)):
        assert stats(**kw) == -1, kw                            # CM_ERR_ARG
        assert b"cm_value_stats" in lib.cm_last_error(), kw
    assert stats(T=0) == 0 and stats(B=0) == 0 and stats(T=0, r=None, pl=None, v=None, out=None) == 0    # nothing to do, nothing launched
    assert stats(B=0, mu=None, lo=None) == 0

    def epi(T=5, B=6, pl=p, st=p, g=3, take=2, epg=4, row0=1, ep=p):
        return lib.cm_episode_value(T, B, pl, st, g, take, epg, row0, ep, None)

    for kw in (dict(pl=None), dict(st=None), dict(ep=None), dict(T=0), dict(B=-1), dict(g=0), dict(g=4), dict(take=4), dict(row0=-1),
               dict(row0=3), dict(take=3, epg=3)):
        assert epi(**kw) == -1, kw
        assert b"cm_episode_value" in lib.cm_last_error(), kw
    assert epi(B=0) == 0 and epi(take=0) == 0
    for K, E, ep, out in ((0, 4, p, p), (2, 0, p, p), (2, 4, None, p), (2, 4, p, None)):
        assert lib.cm_value_means(K, E, ep, out, None) == -1
        assert b"cm_value_means" in lib.cm_last_error()

    def crv(T=5, B=6, pl=p, st=p, g=3, take=2, acc=0, sums=p):
        return lib.cm_value_curves(T, B, pl, st, g, take, acc, sums, None)

    for kw in (dict(pl=None), dict(st=None), dict(sums=None), dict(T=0), dict(B=-1), dict(g=0), dict(g=4), dict(take=4), dict(take=-1),
               dict(acc=2)):
        assert crv(**kw) == -1, kw
        assert b"cm_value_curves" in lib.cm_last_error(), kw
    assert crv(B=0) == 0 and crv(take=0) == 0
    for args in ((0, 5, 3, p, p), (2, 0, 3, p, p), (2, 5, 0, p, p), (2, 5, 3, None, p), (2, 5, 3, p, None)):
        assert lib.cm_value_curve_means(*args, None) == -1, args
        assert b"cm_value_curve_means" in lib.cm_last_error(), args
