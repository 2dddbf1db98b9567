"""cm_episode_stats / cm_episode_means (csrc/cm_episode.hip), the part that needs no GPU: the numpy restatement the GPU tests
compare against (tests/episode_ref.py) gives the written-down answers of hand-made trajectories and agrees with
evaluate._episode - the host loop eval_models runs - on seeded random arrays; the two symbols are declared, bound and exported;
their argument errors come back as codes before anything is launched; and the ISA of the unit has no private segment, no spill
and no flat or scratch addressing."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import episode_ref as R, isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- hand-made trajectories: T = 4, N = 2 --------------------------------------------------------------------------------------
REWARD = np.array([1.5, -0.25, 2.0, 4.0])
DETAILS = np.array([[1, 2, 3, 4, 5, 9], [2, 0, 1, 1, 1, 9], [0, 4, 0, 2, 3, 9], [3, 2, 2, 0, 1, 9]], np.int32)
SUCCESS = np.array([0, 1, 0, 1], np.int32)
# slot sums 2, 4, 0, 3, 1 -> deg = 1, 2, 0, 1.5, 0.5
ADJ = np.array([[[1, 0], [0, 1]], [[1, 1], [1, 1]], [[0, 0], [0, 0]], [[1, 1], [0, 1]], [[0, 0], [1, 0]]], np.float32)


def _row(path_len, scenario=R.PP, adj=ADJ):
    return R.episode_row(REWARD, DETAILS, SUCCESS, np.array(path_len, np.int32), adj, 2, scenario)


def test_written_down_answers_of_hand_made_trajectories():
    # n = 1: the single degree entry is deg[0]
    assert _row([1, 0, 0, 0]) == [0.0, 1.5, 1.0, 1.0, 1.0, 3.0, 1.0, 2.5, 0.0]
    # an end at T-1: n = 4, degrees deg[1], deg[2], deg[3], deg[3] - the last one repeated, deg[4] never read
    assert _row([0, 0, 0, 4]) == [1.0, 7.25, 6.0, 4.0, 4.0, 6.0, (2 + 0 + 1.5 + 1.5) / 4, 5.0, 0.0]
    # no end: the step limit cuts the episode at n = T, the same sums, success of the last step
    assert _row([0, 0, 0, 0]) == _row([0, 0, 0, 4])
    # two ends in T: only the first episode counts (n = 2: degrees deg[1], deg[1])
    assert _row([0, 2, 0, 2]) == [1.0, 1.25, 3.0, 2.0, 1.0, 4.0, 2.0, 3.0, 0.0]
    # Coverage: every detail column / nA, vars2 from column 3
    assert _row([0, 2, 0, 2], R.CO) == [1.0, 1.25, 1.5, 2.0, 1.0, 2.0, 2.0, 3.0, 2.5]
    # dist_adj = None: the constant full graph, nodeDeg = N
    assert _row([0, 0, 3, 0], adj=None) == [0.0, 3.25, 3.0, 3.0, 3.0, 4.0, 2.0, 4.5, 0.0]


def test_stats_rows_and_means_written_down():
    # B = 4 in two groups of 2, take 1: envs 0 and 2 -> rows 0*3+1 and 1*3+1 of a [2*3, 9] table, nothing else touched
    path_len = np.array([[1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 4, 0]], np.int32)
    tile = lambda a: np.repeat(a[:, None], 4, 1)    # noqa: E731
    ep = np.full((6, 9), -7.0)
    R.episode_stats(tile(REWARD), tile(DETAILS), tile(SUCCESS), path_len, tile(ADJ), 2, R.PP, 2, 1, 3, 1, ep)
    assert ep[1].tolist() == _row([1, 0, 0, 0]) and ep[4].tolist() == _row([0, 0, 0, 4])
    assert (ep[[0, 2, 3, 5]] == -7.0).all()
    table = np.zeros((1, 4, 9))
    table[0, :, 1] = [1.0, 3.0, 5.0, 7.0]
    table[0, :, 3] = [2.0, 2.0, 4.0, 4.0]
    s = R.episode_means(table)
    assert s.shape == (1, 12) and s[0, 1] == 4.0 and s[0, 3] == 3.0 and s[0, 0] == 0.0
    assert s[0, 9] == np.sqrt(5.0) and s[0, 10] == 1.0 and s[0, 11] == 7.0


@pytest.mark.parametrize("scenario,N,with_adj", [(R.PP, 4, True), (R.CO, 5, True), (R.PP, 3, False), (R.CO, 24, True)])
def test_restatement_equals_the_host_loop_of_eval_models(scenario, N, with_adj):
    """evaluate._episode on the host arrays _rounds would hand it (degrees rounded to f32 per step, as torch computes them):
    integer-valued results equal, sums within 2 n 2^-53 sum|x_t| (two n-term f64 sums in different orders), nodeDeg to
    rtol 2^-23 (the host path's f32 degrees)."""
    import torch
    from com_marl_amd.evaluate import VECTORS, _episode
    T, B = 33, 12
    buf = R.buffers(T, B, N, seed=11 + N, with_adj=with_adj)
    ended = buf["path_len"] > 0
    first = np.where(ended.any(0), ended.argmax(0), T - 1)
    h = dict(first=first, reward=buf["reward"], details=buf["details"], success=buf["success"])
    if with_adj:
        h["deg"] = torch.from_numpy(buf["dist_adj"]).sum(-1).mean(-1).numpy()
        assert h["deg"].dtype == np.float32
    lengths = set()
    for b in range(B):
        adj_b = buf["dist_adj"][:, b] if with_adj else None
        row, absrow, n = R.episode_row(buf["reward"][:, b], buf["details"][:, b], buf["success"][:, b], buf["path_len"][:, b],
                                       adj_b, N, scenario, with_abs=True)
        n_host, cols, _ = _episode(h, b, N, scenario == R.PP)
        assert n == n_host == row[3]
        lengths.add(n)
        assert row[0] == int(buf["success"][n - 1, b])
        for i, vec in enumerate(VECTORS):
            got, bound = row[1 + i], R.sum_bound(n, absrow[1 + i])
            if vec == "nodeDeg":
                assert got == pytest.approx(float(np.mean(cols[vec])), rel=2.0 ** -23, abs=0.0), (b, vec)
            elif bound == 0.0:
                assert got == float(np.sum(cols[vec])), (b, vec)
            else:
                assert abs(got - float(np.sum(cols[vec]))) <= bound, (b, vec)
    assert {1, 2, T} <= lengths                                            # ends at 0, at T-1 / never, and in between


def test_buffers_hold_every_kind():
    buf = R.buffers(5, 4, 2, seed=0)
    assert sorted(buf["kinds"]) == sorted(R.KINDS)
    n_ends = (buf["path_len"] > 0).sum(0)
    assert sorted(n_ends.tolist()) == [0, 1, 1, 2]
    assert set(np.unique(buf["dist_adj"])) <= {0.0, 1.0} and buf["dist_adj"].shape == (6, 4, 2, 2)


def test_symbols_are_declared_bound_and_exported():
    from com_marl_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "commarl.h")).read()
    for name in ("cm_episode_stats", "cm_episode_means"):
        assert name in L.EXPORTED and hasattr(L.lib(), name) and name + "(" in hdr
    assert "#define CM_EPI_COLS 9" in hdr and "#define CM_SUM_COLS 12" in hdr
    assert (L.EPI_COLS, L.SUM_COLS) == (R.EPI_COLS, R.SUM_COLS) == (9, 12)
    assert "cm_episode" in isa.units()
    from com_marl_amd.evaluate import VECTORS
    assert R.COLS == ["success"] + VECTORS


def test_argument_errors_answer_without_a_gpu():
    from com_marl_amd import _lib as L
    lib = L.lib()
    p = C.c_void_p(16)                                          # plausible, never dereferenced: the checks precede the launch

    def stats(T=5, B=6, N=4, scen=0, rew=p, det=p, suc=p, pl=p, adj=p, g=3, take=2, epg=4, row0=1, ep=p):
        return lib.cm_episode_stats(T, B, N, scen, rew, det, suc, pl, adj, g, take, epg, row0, ep, None)

    bad = [dict(rew=None), dict(det=None), dict(suc=None), dict(pl=None), dict(ep=None), dict(T=0), dict(N=0), dict(N=256),
           dict(scen=2), dict(scen=-1), dict(g=0), dict(g=4), dict(take=4), dict(row0=-1), dict(row0=3), dict(take=3, epg=3)]
    for kw in bad:
        assert stats(**kw) == -1, kw                            # CM_ERR_ARG
        assert b"cm_episode_stats" in lib.cm_last_error(), kw
    assert stats(B=0) == 0 and stats(take=0) == 0               # nothing to do, nothing launched
    for K, E, ep, out in ((0, 4, p, p), (2, 0, p, p), (2, 4, None, p), (2, 4, p, None)):
        assert lib.cm_episode_means(K, E, ep, out, None) == -1
        assert b"cm_episode_means" in lib.cm_last_error()


def test_kernels_have_no_private_segment_no_spill_and_no_flat_or_scratch_addressing():
    ks = isa.kernels(isa.listing("cm_episode"))
    names = [k.name for k in ks]
    assert len(ks) == 3, names                                  # the stats kernel with 16-byte and 4-byte positions, the means kernel
    assert sum("episode_stats_kernel" in n for n in names) == 2 and sum("episode_means_kernel" in n for n in names) == 1
    for k in ks:
        assert k.private_segment_fixed_size == 0, k.name
        assert k.vgpr_spill_count == 0, k.name
        assert not k.has_flat_or_scratch, k.name
        assert k.count("global_atomic") == 0 and k.count("ds_add") == 0 and k.barriers == 0, k.name
