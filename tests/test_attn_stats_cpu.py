"""cm_attn_stats and its four reductions (csrc/cm_attn_stats.hip), the part that needs no GPU: the restatement the GPU tests compare
against (tests/attn_stats_ref.py) on cases worked by hand, the declarations and bindings, the new keyword of eval_summary /
eval_sweep, and the argument checks, which answer before anything is launched."""
import ctypes as C
import inspect
import math
import os

import numpy as np
import pytest

from tests import attn_stats_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("cm_attn_stats", "cm_episode_attn", "cm_attn_means", "cm_attn_curves", "cm_attn_curve_means")


@pytest.mark.parametrize("N,L", [(1, 1), (4, 2), (9, 3), (70, 8)])
def test_uniform_rows_on_a_full_graph(N, L):
    attn = np.full((N, N), 1.0 / N, np.float32)
    for adj, chan in ((None, None), (np.ones((N, N), np.float32), np.ones((L, N, N), np.float32))):
        got = R.graph_stats(attn, adj, chan, N, L)
        u = float(np.float32(1.0 / N))                           # the f32 weight; N u is 1 within f32 rounding
        np.testing.assert_allclose(got, [N * u, -N * N * u * math.log(u), N * N * u, L * N * N * u, L, L * N * math.log(N)],
                                   rtol=1e-6)
        np.testing.assert_allclose([got[1], got[3], got[4]], [N * math.log(N), N * L, L], rtol=1e-6)
        assert got[4] == pytest.approx(L, rel=1e-14)             # u / (N u): the f32 rounding of u cancels


def test_a_one_hot_row_on_the_diagonal_has_no_entropy():
    N, L = 5, 2
    got = R.graph_stats(np.eye(N, dtype=np.float32), None, None, N, L)
    assert got == [N, 0.0, N, N * L, N * L, 0.0]
    # off the diagonal: still no entropy, and no self weight
    attn = np.roll(np.eye(N, dtype=np.float32), 1, axis=1)
    assert R.graph_stats(attn, None, None, N, L) == [0.0, 0.0, N, N * L, 0.0, 0.0]


def test_a_row_whose_kept_set_is_empty_adds_nothing_to_the_effective_columns():
    N, L = 3, 2
    attn = np.full((N, N), 1.0 / 3.0, np.float32)
    adj = np.ones((N, N), np.float32)
    base = R.graph_stats(attn, adj, None, N, L)
    adj[0] = 0.0                                                 # row 0 hears nobody, not even itself
    got = R.graph_stats(attn, adj, None, N, L)
    assert got[0] == base[0] and got[1] == base[1]
    assert got[2] == pytest.approx(base[2] * 2 / 3) and got[3] == pytest.approx(base[3] * 2 / 3)
    assert got[4] == pytest.approx(base[4] * 2 / 3) and got[5] == pytest.approx(base[5] * 2 / 3)
    # the diagonal is used as recorded: clearing only it drops the self weight and renormalises the rest
    adj = np.ones((N, N), np.float32)
    adj[0, 0] = 0.0
    got = R.graph_stats(attn, adj, None, N, L)
    assert got[4] == pytest.approx(L * (2 * 1 / 3 + 0.0)) and got[5] == pytest.approx(L * (2 * math.log(3) + math.log(2)))


def test_halving_the_kept_set_of_a_uniform_row_lowers_its_entropy_by_ln_2():
    N, L = 8, 1
    attn = np.full((N, N), 0.125, np.float32)
    full = R.graph_stats(attn, None, None, N, L)
    chan = np.ones((L, N, N), np.float32)
    chan[0, 2, 4:] = 0.0                                         # row 2 keeps agents 0 .. 3, itself among them
    half = R.graph_stats(attn, None, chan, N, L)
    assert full[5] - half[5] == pytest.approx(math.log(2), rel=1e-14)
    assert half[4] - full[4] == pytest.approx(0.25 - 0.125) and full[3] - half[3] == pytest.approx(0.5)
    assert half[:3] == full[:3]                                  # the channel does not touch the first three columns


def test_a_zero_weight_adds_no_entropy_term_and_set_means_nonzero():
    attn = np.array([[0.5, 0.5, 0.0], [1.0, 0.0, 0.0], [0.25, 0.25, 0.5]], np.float32)
    adj = np.array([[-2.0, 0.5, 1.0], [-0.0, 0.0, 1.0], [1.0, 1.0, 1.0]], np.float32)
    got = R.graph_stats(attn, adj, None, 3, 1)
    assert got[0] == 1.0 and got[1] == pytest.approx(math.log(2) + 1.5 * math.log(2))
    assert got[2] == 2.0 and got[3] == 2.0                       # row 1's whole weight is on a link out of range
    assert got[4] == pytest.approx(0.5 + 0.0 + 0.5) and got[5] == pytest.approx(math.log(2) + 1.5 * math.log(2))
    many = R.attn_stats(np.stack([attn] * 3), adj, np.ones((1, 3, 3), np.float32), 3, 1)          # one block for all
    np.testing.assert_array_equal(many, np.array([got] * 3))


def test_episode_rows_means_and_curves_follow_the_comm_rules():
    T, B, N, L = 4, 2, 3, 2
    path_len = np.zeros((T, B), np.int32)
    path_len[1, 0] = 2                                           # env 0 ends at step 1: slots 0, 1
    stats = np.arange(T * B * 6, dtype=np.float64).reshape(T, B, 6)
    ep = np.full((2, 6), -1.0)
    R.episode_attn(path_len, stats, N, L, 2, 2, 2, 0, ep)
    np.testing.assert_array_equal(ep[0], (stats[0, 0] + stats[1, 0]) / [6, 6, 6, 12, 12, 12])
    np.testing.assert_allclose(ep[1], stats[:, 1].sum(0) / [12, 12, 12, 24, 24, 24], rtol=1e-15)
    np.testing.assert_allclose(R.attn_means(ep[None])[0], (ep[0] + ep[1]) / 2, rtol=1e-15)
    sums = np.full((1, T, 6), 7.0)
    R.attn_curves(path_len, stats, 2, 2, 0, sums)
    np.testing.assert_array_equal(sums[0, 1], stats[1, 0] + stats[1, 1])
    np.testing.assert_array_equal(sums[0, 2], stats[2, 1])       # the ended episode counts as zero
    R.attn_curves(path_len, stats, 2, 2, 1, sums)
    np.testing.assert_array_equal(sums[0, 3], 2 * stats[3, 1])
    curves = R.attn_curve_means(sums, 4, N, L)
    np.testing.assert_array_equal(curves[0, 3], 2 * stats[3, 1] / [12, 12, 12, 24, 24, 24])
    assert R.path_lens(5, 6, 1, "none").sum() == 0 and (R.path_lens(5, 6, 1, "all0")[0] > 0).all()


def test_seeded_inputs_hold_the_cases_the_tests_name():
    attn, adj, chan = R.seeded(37, 24, 2, seed=1)
    np.testing.assert_allclose(attn.sum(-1), 1.0, atol=3e-6)
    assert attn[0, 0, 1] == 0.0 and attn[0, 0].sum() == pytest.approx(1.0, abs=3e-6)      # the planted zero
    assert 0 < attn[5:].min() < 1e-20                           # weights far below f32 epsilon next to weights near 1
    assert (attn[1] == np.eye(24)).all() and attn[2, 0, 23] == 1.0
    assert not adj[3, 0].any() and not chan[4, 0, 0].any()
    assert set(np.unique(adj)) == {0.0, 1.0} and 0.4 < adj.mean() < 0.6 and 0.4 < chan.mean() < 0.6


def test_symbols_are_declared_bound_and_exported():
    from com_marl_amd import _lib as L, evaluate
    hdr = open(os.path.join(ROOT, "include", "commarl.h")).read()
    for name in SYMBOLS:
        assert name in L.EXPORTED and hasattr(L.lib(), name) and name + "(" in hdr
    assert "#define CM_ATTN_COLS 6" in hdr and "#define CM_EPA_COLS 6" in hdr
    assert (L.ATTN_COLS, L.EPA_COLS) == (R.ATTN_COLS, R.EPA_COLS) == (6, 6)
    assert "#define CM_ABI_VERSION 3" in hdr and L.lib().cm_abi_version() == 3
    assert evaluate.ATTN_KEYS == R.KEYS
    assert "cm_attn_stats.hip" in open(os.path.join(ROOT, "com-marl_amd", "csrc", "Makefile")).read()


def test_eval_summary_and_eval_sweep_take_attn_stats():
    from com_marl_amd import envs, evaluate
    for fn in (evaluate.eval_summary, evaluate.eval_sweep):
        par = inspect.signature(fn).parameters
        assert "attn_stats" in par and par["attn_stats"].default is False
    assert list(inspect.signature(envs.attn_stats).parameters)[:4] == ["attn", "dist_adj", "channels", "n_hops"]


def test_a_policy_without_attention_is_refused_before_anything_is_built():
    from com_marl_amd import evaluate

    class ObsDP:                                                # no `comm` attribute: what marks an Obs-DP / CENT policy
        pass

    class CommDP:
        comm = True

    for policies in (ObsDP(), [CommDP(), ObsDP()]):
        with pytest.raises(ValueError, match="attn_stats"):     # (the wrapper is never touched)
            evaluate.eval_summary(None, policies, attn_stats=True)
        with pytest.raises(ValueError, match="attn_stats"):
            evaluate._score("eval_sweep", None, policies, 8, 6, True, None, False, False, conds=[{}], attn_stats=True)


def test_argument_errors_answer_without_a_gpu():
    from com_marl_amd import _lib as L
    lib = L.lib()
    p = C.c_void_p(16)                                          # plausible, never dereferenced: the checks precede the launch

    def stats(S=3, N=4, Lh=2, at=p, t_st=16, adj=p, a_st=16, ch=p, c_st=32, out=p):
        return lib.cm_attn_stats(S, N, Lh, at, t_st, adj, a_st, ch, c_st, out, None)

    for kw in (dict(S=-1), dict(N=0), dict(N=256), dict(Lh=0), dict(Lh=9), dict(t_st=15), dict(t_st=0), dict(a_st=15), dict(a_st=-16),
               dict(c_st=31), dict(c_st=16), dict(out=None), dict(at=None)):
        assert stats(**kw) == -1, kw                            # CM_ERR_ARG
        assert b"cm_attn_stats" in lib.cm_last_error(), kw
    assert stats(S=0) == 0 and stats(S=0, out=None, at=None) == 0        # nothing to do, nothing launched

    def epi(T=5, B=6, N=4, Lh=2, pl=p, st=p, g=3, take=2, epg=4, row0=1, ep=p):
        return lib.cm_episode_attn(T, B, N, Lh, pl, st, g, take, epg, row0, ep, None)

    for kw in (dict(pl=None), dict(st=None), dict(ep=None), dict(T=0), dict(N=0), dict(N=256), dict(Lh=0), dict(Lh=9), dict(g=0),
               dict(g=4), dict(take=4), dict(row0=-1), dict(row0=3), dict(take=3, epg=3)):
        assert epi(**kw) == -1, kw
        assert b"cm_episode_attn" in lib.cm_last_error(), kw
    assert epi(B=0) == 0 and epi(take=0) == 0
    for K, E, ep, out in ((0, 4, p, p), (2, 0, p, p), (2, 4, None, p), (2, 4, p, None)):
        assert lib.cm_attn_means(K, E, ep, out, None) == -1
        assert b"cm_attn_means" in lib.cm_last_error()

    def crv(T=5, B=6, N=4, Lh=2, pl=p, st=p, g=3, take=2, acc=0, sums=p):
        return lib.cm_attn_curves(T, B, N, Lh, pl, st, g, take, acc, sums, None)

    for kw in (dict(pl=None), dict(st=None), dict(sums=None), dict(T=0), dict(B=-1), dict(N=0), dict(N=256), dict(Lh=0), dict(Lh=9),
               dict(g=0), dict(g=4), dict(take=4), dict(take=-1), dict(acc=2)):
        assert crv(**kw) == -1, kw
        assert b"cm_attn_curves" in lib.cm_last_error(), kw
    assert crv(B=0) == 0 and crv(take=0) == 0
    for args in ((0, 5, 3, 4, 2, p, p), (2, 0, 3, 4, 2, p, p), (2, 5, 0, 4, 2, p, p), (2, 5, 3, 0, 2, p, p), (2, 5, 3, 256, 2, p, p),
                 (2, 5, 3, 4, 0, p, p), (2, 5, 3, 4, 9, p, p), (2, 5, 3, 4, 2, None, p), (2, 5, 3, 4, 2, p, None)):
        assert lib.cm_attn_curve_means(*args, None) == -1, args
        assert b"cm_attn_curve_means" in lib.cm_last_error(), args
