"""cm_comm_stats / cm_episode_comm / cm_comm_means (csrc/cm_comm_stats.hip), the part that needs no GPU: the restatement the GPU
tests compare against (tests/comm_ref.py) on cases worked by hand, the declarations and bindings, the new keyword of
eval_summary / eval_sweep, and the argument checks, which answer before anything is launched."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from tests import comm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_a_single_agent_has_nobody_to_hear():
    for L in (1, 2, 8):
        assert R.graph_stats(np.ones((1, 1), np.float32), np.ones((L, 1, 1), np.float32), 1, L) == [0, 0, 0, 0]
        assert R.graph_stats(None, None, 1, L) == [0, 0, 0, 0]


@pytest.mark.parametrize("N,L", [(2, 1), (5, 1), (5, 2), (5, 8), (9, 3), (70, 2)])
def test_path_graph_reaches_L_neighbours_on_each_side(N, L):
    adj, chan, want = R.path_graph(N, L)
    assert want[2] == sum(min(i, L) + min(N - 1 - i, L) for i in range(N))
    assert R.graph_stats(adj, chan, N, L) == want
    assert R.graph_stats(adj, None, N, L) == want                  # NULL channels are ones


def test_the_order_of_the_hops_matters():
    first, second = R.hop_order_pair()
    assert R.graph_stats(first[0], first[1], 3, 2) == first[2] == [6, 2, 3, 6]
    assert R.graph_stats(second[0], second[1], 3, 2) == second[2] == [6, 2, 2, 6]


def test_set_means_nonzero_and_the_diagonals_are_ignored():
    adj = np.array([[0.0, 0.5, -0.0], [-2.0, 0.0, 0.0], [1.0, 1.0, -0.0]], np.float32)
    chan = np.ones((1, 3, 3), np.float32)
    chan[0, 2, 1] = -0.0
    base = R.graph_stats(adj, chan, 3, 1)
    assert base == [4, 3, 3, 4]
    adj2, chan2 = adj.copy(), chan.copy()
    adj2[np.eye(3, dtype=bool)] = [7.0, 0.0, -1.0]
    chan2[0][np.eye(3, dtype=bool)] = [0.0, 3.0, 0.0]
    assert R.graph_stats(adj2, chan2, 3, 1) == base
    # stride 0: one block for every graph
    S = 3
    many = R.comm_stats(np.stack([adj] * S), chan[0][None], 3, 1)
    np.testing.assert_array_equal(many, np.array([base] * S))
    np.testing.assert_array_equal(R.comm_stats(np.stack([adj] * S), np.stack([chan] * S), 3, 1), many)


def test_seeded_graphs_hold_the_values_the_tests_name():
    adj, chan = R.seeded(16, 5, 2, seed=1)
    off = ~np.eye(5, dtype=bool)
    assert not adj[0][off].any() and (adj[3][off] != 0).all()                        # densities 0 and 1
    vals = set(np.unique(adj).tolist()) | set(np.unique(chan).tolist())
    assert {0.5, -2.0, 1.0, 0.0} <= vals and np.signbit(adj[adj == 0]).any() and (~np.signbit(adj[adj == 0])).any()
    assert (adj != np.swapaxes(adj, 1, 2)).any()                                     # asymmetric
    st = R.comm_stats(adj, chan, 5, 2)
    assert (st[:, 1] <= 2 * st[:, 0]).all() and (st[:, 2] <= st[:, 3]).all() and (st[:, 3] <= 20).all()


def test_episode_rows_divide_integer_sums_once():
    path_len = np.zeros((4, 2), np.int32)
    path_len[1, 0] = 2                                                               # env 0 ends at step 1: slots 0, 1
    stats = np.arange(5 * 2 * 4, dtype=np.int32).reshape(5, 2, 4)
    ep = np.full((2, 4), -1.0)
    R.episode_comm(path_len, stats, 3, 2, 2, 2, 2, 0, ep)
    np.testing.assert_array_equal(ep[0], [(0 + 8) / 6, (1 + 9) / 12, (2 + 10) / 6, (3 + 11) / 6])
    np.testing.assert_array_equal(ep[1], [(4 + 12 + 20 + 28) / 12, (5 + 13 + 21 + 29) / 24, (6 + 14 + 22 + 30) / 12,
                                          (7 + 15 + 23 + 31) / 12])
    np.testing.assert_array_equal(R.comm_means(ep[None])[0], [(ep[0, c] + ep[1, c]) / 2 for c in range(4)])
    assert R.summary_keys([0.0, 0.0, 0.0, 0.0])["delivery"] == 1.0 and R.summary_keys([2.0, 1.0, 1.5, 3.0])["delivery"] == 0.5


def test_symbols_are_declared_bound_and_exported():
    from com_marl_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "commarl.h")).read()
    for name in ("cm_comm_stats", "cm_episode_comm", "cm_comm_means"):
        assert name in L.EXPORTED and hasattr(L.lib(), name) and name + "(" in hdr
    assert "#define CM_COMM_COLS 4" in hdr and "#define CM_EPC_COLS 4" in hdr
    assert (L.COMM_COLS, L.EPC_COLS) == (R.COMM_COLS, R.EPC_COLS) == (4, 4)
    assert L.lib().cm_abi_version() == 3
    from com_marl_amd import evaluate
    assert evaluate.COMM_STATS == R.EPC and evaluate.COMM_KEYS == R.EPC + ["delivery"]


def test_eval_summary_and_eval_sweep_take_comm_stats():
    from com_marl_amd import envs, evaluate
    for fn in (evaluate.eval_summary, evaluate.eval_sweep):
        par = inspect.signature(fn).parameters
        assert "comm_stats" in par and par["comm_stats"].default is False
    assert list(inspect.signature(envs.comm_stats).parameters)[:3] == ["dist_adj", "channels", "n_hops"]


def test_argument_errors_answer_without_a_gpu():
    from com_marl_amd import _lib as L
    lib = L.lib()
    p = C.c_void_p(16)                                          # plausible, never dereferenced: the checks precede the launch

    def stats(S=3, N=4, Lh=2, adj=p, a_st=16, ch=p, c_st=32, out=p):
        return lib.cm_comm_stats(S, N, Lh, adj, a_st, ch, c_st, out, None)

    for kw in (dict(S=-1), dict(N=0), dict(N=256), dict(Lh=0), dict(Lh=9), dict(a_st=15), dict(a_st=-16), dict(c_st=31), dict(c_st=16),
               dict(out=None)):
        assert stats(**kw) == -1, kw                            # CM_ERR_ARG
        assert b"cm_comm_stats" in lib.cm_last_error(), kw
    assert stats(S=0) == 0 and stats(S=0, out=None) == 0        # nothing to do, nothing launched

    def epi(T=5, B=6, N=4, Lh=2, pl=p, st=p, g=3, take=2, epg=4, row0=1, ep=p):
        return lib.cm_episode_comm(T, B, N, Lh, pl, st, g, take, epg, row0, ep, None)

    for kw in (dict(pl=None), dict(st=None), dict(ep=None), dict(T=0), dict(N=0), dict(N=256), dict(Lh=0), dict(Lh=9), dict(g=0),
               dict(g=4), dict(take=4), dict(row0=-1), dict(row0=3), dict(take=3, epg=3)):
        assert epi(**kw) == -1, kw
        assert b"cm_episode_comm" in lib.cm_last_error(), kw
    assert epi(B=0) == 0 and epi(take=0) == 0
    for K, E, ep, out in ((0, 4, p, p), (2, 0, p, p), (2, 4, None, p), (2, 4, p, None)):
        assert lib.cm_comm_means(K, E, ep, out, None) == -1
        assert b"cm_comm_means" in lib.cm_last_error()
