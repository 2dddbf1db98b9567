"""The numpy float64 restatement of the listening statistics (tests/listen_stats_ref.py) on hand cases, its reducers against plain
loops written out here, and what answers without a GPU: the symbols, the keywords, the refusals."""
import ctypes as C
import inspect
import math
import os

import numpy as np
import pytest

from tests import listen_stats_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["cm_listen_stats", "cm_episode_listen", "cm_listen_means", "cm_listen_curves", "cm_listen_curve_means"]
f32 = np.float32


def test_identical_rows_give_zeros():
    p = R.softmax_rows(np.random.default_rng(0).standard_normal((3, 4, 5)) * 4)
    out = R.listen_stats(p, p.copy(), p.copy())
    assert out.shape == (3, 6) and (out == 0).all()
    assert (R.listen_stats(p, None, None) == 0).all()
    half = R.listen_stats(p, None, np.roll(p, 1, axis=0))
    assert (half[:, :3] == 0).all() and (half[:, 3:5] > 0).all()


def test_a_two_action_row_with_known_kl_and_tv():
    p, q = np.array([0.75, 0.25], f32), np.array([0.5, 0.5], f32)          # exact in f32
    kl, tv, flip = R.row_terms(p, q)
    assert kl == pytest.approx(0.75 * math.log(1.5) + 0.25 * math.log(0.5), rel=1e-15)
    assert tv == 0.25 and flip == 0.0
    kl, tv, flip = R.row_terms(q, p[::-1])
    assert kl == pytest.approx(0.5 * math.log(2.0) + 0.5 * math.log(2.0 / 3.0), rel=1e-15) and tv == 0.25
    assert flip == 1.0                                                      # q ties -> 0; reversed p peaks at 1
    # the graph row sums the agents in order; mute in columns 0-2, lossless in 3-5
    row = R.graph_row(np.stack([p, q]), np.stack([q, q]), np.stack([p, p[::-1]]))
    assert row[0] == R.row_terms(p, q)[0] and row[1] == 0.25 and row[2] == 0.0
    assert row[3] == R.row_terms(q, p[::-1])[0] and row[4] == 0.25 and row[5] == 1.0


def test_a_zero_in_q_under_a_positive_p_gives_the_finite_flt_min_value():
    assert R.FLT_MIN == float(np.finfo(f32).tiny)
    p, q = np.array([0.5, 0.5, 0.0], f32), np.array([1.0, 0.0, 0.0], f32)
    kl, tv, flip = R.row_terms(p, q)
    assert math.isfinite(kl)
    assert kl == pytest.approx(0.5 * math.log(0.5) + 0.5 * (math.log(0.5) + 126 * math.log(2.0)), rel=1e-15)
    assert tv == 0.5 and flip == 0.0
    # p[a] == 0 adds nothing, whatever q[a] is; a q below FLT_MIN counts as FLT_MIN
    assert R.row_terms(np.array([1.0, 0.0], f32), np.array([1.0, 0.0], f32)) == (0.0, 0.0, 0.0)
    tiny = np.array([1.0, 1e-42], f32)
    assert R.row_terms(np.array([0.5, 0.5], f32), tiny)[0] == R.row_terms(np.array([0.5, 0.5], f32), np.array([1.0, 0.0], f32))[0]
    # not clamped: an f32 row that sums to a hair above 1 against one that sums to 1 may come out below 0
    assert R.row_terms(np.array([0.5, 0.5], f32), np.array([0.5, 0.5 + 2.0 ** -24 * 2], f32))[0] < 0


def test_a_tie_in_p_or_in_q_resolves_to_the_first_index():
    tie, second = np.array([0.4, 0.4, 0.2], f32), np.array([0.3, 0.5, 0.2], f32)
    assert R.row_terms(tie, second)[2] == 1.0                                # p: index 0, q: index 1
    assert R.row_terms(second, tie)[2] == 1.0
    assert R.row_terms(tie, np.array([0.5, 0.3, 0.2], f32))[2] == 0.0
    assert R.row_terms(tie[::-1].copy(), np.array([0.1, 0.5, 0.4], f32))[2] == 0.0      # [0.2, 0.4, 0.4] ties at 1, 2 -> 1
    # compared on the f32 values: two doubles that round to the same float tie
    a = np.array([0.3, 0.3 + 1e-10, 0.4 - 1e-10]).astype(f32)
    assert a[0] == a[1] and R.row_terms(np.array([0.5, 0.5, 0.0], f32), np.array([a[0], a[1], 0.0], f32))[2] == 0.0


def test_seeded_inputs_hold_the_cases_the_tests_name():
    for N, A in ((1, 5), (4, 5), (24, 2), (9, 8)):
        p, m, l = R.seeded(37, N, A, seed=N + A)
        for x in (p, m, l):
            assert x.dtype == f32 and x.shape == (37, N, A)
            np.testing.assert_allclose(x.sum(-1), 1.0, atol=3e-6)
        a = int(np.argmax(p[0, 0]))
        assert m[0, 0, a] == 0.0 and p[0, 0, a] > 0                            # the FLT_MIN term
        assert p[1, 0, 0] == 1.0 and m[1, 0, A - 1] == 1.0 and (l[1, 0] == p[1, 0]).all()
        assert p[2, 0, A - 2] == p[2, 0, A - 1] == p[2, 0].max() and m[2, 0, 0] == m[2, 0, 1] == m[2, 0].max()
        assert (m[3] == p[3]).all() and (l[3] == p[3]).all()
        want = R.listen_stats(p, m, l)
        assert (want[3] == 0).all() and want[0, 0] > 10 and np.isfinite(want).all()
        assert N > 2 or (want[1, 3:] == 0).all()                           # rows 0 and N - 1 of graph 1: lossless == p
        assert want[1, 2] >= 1                                             # one-hot rows on different actions flip
        assert (want[:, R.FLIP_COLS] == np.round(want[:, R.FLIP_COLS])).all() and want[:, R.FLIP_COLS].max() <= N
        assert 0 < np.abs(want[5:, 3]).max() < 1 and want[5:, 0].min() > 0    # the perturbed rows nearly cancel, the others do not


def test_reducers_equal_plain_loops():
    T, B, N = 5, 6, 4
    rng = np.random.default_rng(7)
    stats = rng.random((T, B, R.LISTEN_COLS))
    path_len = np.zeros((T, B), np.int32)
    path_len[2, 0] = 3                                                   # env 0: n = 3
    path_len[0, 1] = 1                                                   # env 1: n = 1
    path_len[4, 3] = 5                                                   # env 3: n = 5 (ends at the last step)
    path_len[1, 4], path_len[3, 4] = 2, 2                                # env 4: n = 2, the second end is another episode
    lengths = [3, 1, T, 5, 2, T]
    episodes = np.full((2 * 4, R.EPL_COLS), -1.0)
    R.episode_listen(path_len, stats, N, 3, 2, 4, 1, episodes)           # groups of 3, take 2, rows 1 .. 2 of 4
    for k in range(2):
        for j in range(2):
            b = 3 * k + j
            want = sum(stats[t, b] for t in range(lengths[b])) / (lengths[b] * N)      # ONE divisor for all six columns
            np.testing.assert_allclose(episodes[4 * k + 1 + j], want, rtol=1e-15)
        assert (episodes[4 * k] == -1).all() and (episodes[4 * k + 3] == -1).all()
    np.testing.assert_allclose(R.listen_means(episodes.reshape(2, 4, 6)), episodes.reshape(2, 4, 6).sum(1) / 4, rtol=1e-15)

    sums = np.full((2, T, R.LISTEN_COLS), -1.0)
    R.listen_curves(path_len, stats, 3, 2, 0, sums)                      # overwrites
    np.testing.assert_allclose(sums[0, 0], stats[0, 0] + stats[0, 1], rtol=1e-15)
    np.testing.assert_array_equal(sums[0, 1], stats[1, 0])               # env 1 has ended: it adds nothing
    np.testing.assert_array_equal(sums[0, 3], 0.0)                       # both have
    np.testing.assert_allclose(sums[1, 1], stats[1, 3] + stats[1, 4], rtol=1e-15)
    np.testing.assert_array_equal(sums[1, 2], stats[2, 3])
    first = sums.copy()
    R.listen_curves(path_len, stats, 3, 2, 1, sums)                      # adds
    np.testing.assert_allclose(sums, 2 * first, rtol=1e-15)
    np.testing.assert_array_equal(R.listen_curve_means(sums, 4, N), sums / 16.0)
    assert R.listen_curves(path_len, stats, 3, 0, 0, sums.copy()).tolist() == sums.tolist()      # take = 0: untouched


def test_symbols_are_declared_bound_and_exported():
    from com_marl_amd import _lib as L, evaluate
    hdr = open(os.path.join(ROOT, "include", "commarl.h")).read()
    for name in SYMBOLS:
        assert name in L.EXPORTED and hasattr(L.lib(), name) and name + "(" in hdr
    assert "#define CM_LISTEN_COLS 6" in hdr and "#define CM_EPL_COLS 6" in hdr
    assert (L.LISTEN_COLS, L.EPL_COLS) == (R.LISTEN_COLS, R.EPL_COLS) == (6, 6)
    assert evaluate.LISTEN_KEYS == R.KEYS
    assert "cm_listen_stats.hip" in open(os.path.join(ROOT, "com-marl_amd", "csrc", "Makefile")).read()


def test_eval_summary_and_eval_sweep_take_listen_stats():
    from com_marl_amd import envs, evaluate, rollout
    for fn in (evaluate.eval_summary, evaluate.eval_sweep):
        par = inspect.signature(fn).parameters
        assert "listen_stats" in par and par["listen_stats"].default is False
    assert list(inspect.signature(envs.listen_stats).parameters) == ["probs", "mute", "lossless", "out"]
    assert list(inspect.signature(rollout.RolloutEngine.replay_probs).parameters) == ["self", "t0", "n", "channels", "out"]
    assert rollout.REPLAY_MASK_BYTES >= 4 * 8 * 255 * 255                  # one env state of the largest shape fits


def test_a_policy_without_a_comm_trunk_is_refused_before_anything_is_built():
    from com_marl_amd import evaluate

    class ObsDP:                                                # no `comm` attribute: what marks an Obs-DP / CENT policy
        pass

    class CommDP:
        comm = True

    for policies in (ObsDP(), [CommDP(), ObsDP()]):
        with pytest.raises(ValueError, match="listen_stats"):   # (the wrapper is never touched)
            evaluate.eval_summary(None, policies, listen_stats=True)
        with pytest.raises(ValueError, match="listen_stats"):
            evaluate._score("eval_sweep", None, policies, 8, 6, True, None, False, False, conds=[{}], listen_stats=True)


def test_argument_errors_answer_without_a_gpu():
    from com_marl_amd import _lib as L
    lib = L.lib()
    p = C.c_void_p(16)                                          # plausible, never dereferenced: the checks precede the launch

    def stats(S=3, N=4, A=5, pr=p, p_st=20, mu=p, m_st=20, lo=p, l_st=20, out=p):
        return lib.cm_listen_stats(S, N, A, pr, p_st, mu, m_st, lo, l_st, out, None)

    for kw in (dict(S=-1), dict(N=0), dict(N=256), dict(A=1), dict(A=9), dict(A=0), dict(p_st=19), dict(p_st=0), dict(m_st=19),
               dict(m_st=0), dict(l_st=19), dict(l_st=-20), dict(out=None), dict(pr=None)):
        assert stats(**kw) == -1, kw                            # CM_ERR_ARG
        assert b"cm_listen_stats" in lib.cm_last_error(), kw
    assert stats(S=0) == 0 and stats(S=0, out=None, pr=None) == 0         # nothing to do, nothing launched
    assert stats(S=0, mu=None, m_st=0, lo=None, l_st=0) == 0              # a NULL counterfactual's stride is not looked at

    def epi(T=5, B=6, N=4, pl=p, st=p, g=3, take=2, epg=4, row0=1, ep=p):
        return lib.cm_episode_listen(T, B, N, pl, st, g, take, epg, row0, ep, None)

    for kw in (dict(pl=None), dict(st=None), dict(ep=None), dict(T=0), dict(N=0), dict(N=256), dict(g=0), dict(g=4), dict(take=4),
               dict(row0=-1), dict(row0=3), dict(take=3, epg=3)):
        assert epi(**kw) == -1, kw
        assert b"cm_episode_listen" in lib.cm_last_error(), kw
    assert epi(B=0) == 0 and epi(take=0) == 0
    for K, E, ep, out in ((0, 4, p, p), (2, 0, p, p), (2, 4, None, p), (2, 4, p, None)):
        assert lib.cm_listen_means(K, E, ep, out, None) == -1
        assert b"cm_listen_means" in lib.cm_last_error()

    def crv(T=5, B=6, N=4, pl=p, st=p, g=3, take=2, acc=0, sums=p):
        return lib.cm_listen_curves(T, B, N, pl, st, g, take, acc, sums, None)

    for kw in (dict(pl=None), dict(st=None), dict(sums=None), dict(T=0), dict(B=-1), dict(N=0), dict(N=256), dict(g=0), dict(g=4),
               dict(take=4), dict(take=-1), dict(acc=2)):
        assert crv(**kw) == -1, kw
        assert b"cm_listen_curves" in lib.cm_last_error(), kw
    assert crv(B=0) == 0 and crv(take=0) == 0
    for args in ((0, 5, 3, 4, p, p), (2, 0, 3, 4, p, p), (2, 5, 0, 4, p, p), (2, 5, 3, 0, p, p), (2, 5, 3, 256, p, p),
                 (2, 5, 3, 4, None, p), (2, 5, 3, 4, p, None)):
        assert lib.cm_listen_curve_means(*args, None) == -1, args
        assert b"cm_listen_curve_means" in lib.cm_last_error(), args
