"""cm_episode_curves / cm_curve_means / cm_comm_curves / cm_comm_curve_means (csrc/cm_episode_curves.hip), the part that needs no
GPU: the four symbols are declared, bound and exported and the unit is one of the library's; their argument errors come back as
codes before anything is launched; the ISA of the unit has no private segment, no spill, no flat or scratch addressing, no atomic
and no barrier; and the numpy restatement the GPU tests compare against (tests/curves_ref.py) gives the written-down answers of a
hand-made round and ties to the reference rule - evaluate._episode's per-step lists, zero-padded to T and averaged over the
episodes in plain numpy (pad_sequence + mean, exp_runners/testing.py:307-324)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import comm_ref, curves_ref as V, episode_ref as R, isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cm_episode_curves", "cm_curve_means", "cm_comm_curves", "cm_comm_curve_means")


def test_symbols_are_declared_bound_and_exported():
    from com_marl_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "commarl.h")).read()
    for name in NAMES:
        assert name in L.EXPORTED and hasattr(L.lib(), name) and name + "(" in hdr
    assert "#define CM_ABI_VERSION 3" in hdr and L.lib().cm_abi_version() == 3         # symbols were only added
    assert "cm_episode_curves" in isa.units()
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert f'({len(L.EXPORTED)} `extern "C"` entry points)' in readme


def test_argument_errors_answer_without_a_gpu():
    from com_marl_amd import _lib as L
    lib = L.lib()
    p = C.c_void_p(16)                                          # plausible, never dereferenced: the checks precede the launch

    def curves(T=5, B=6, N=4, scen=0, rew=p, det=p, suc=p, pl=p, adj=p, g=3, take=2, acc=0, sums=p):
        return lib.cm_episode_curves(T, B, N, scen, rew, det, suc, pl, adj, g, take, acc, sums, None)

    bad = [dict(rew=None), dict(det=None), dict(suc=None), dict(pl=None), dict(sums=None), dict(T=0), dict(B=-3), dict(N=0),
           dict(N=256), dict(scen=2), dict(scen=-1), dict(g=0), dict(g=4), dict(take=4), dict(take=-1), dict(acc=2), dict(acc=-1)]
    for kw in bad:
        assert curves(**kw) == -1, kw                           # CM_ERR_ARG
        assert b"cm_episode_curves" in lib.cm_last_error(), kw
    assert curves(B=0) == 0 and curves(take=0) == 0             # nothing to do, nothing launched
    assert curves(B=0, sums=None) == 0 and curves(take=0, rew=None) == 0

    def comm(T=5, B=6, N=4, Lh=2, pl=p, st=p, g=3, take=2, acc=1, sums=p):
        return lib.cm_comm_curves(T, B, N, Lh, pl, st, g, take, acc, sums, None)

    bad = [dict(pl=None), dict(st=None), dict(sums=None), dict(T=0), dict(N=0), dict(N=256), dict(Lh=0), dict(Lh=9), dict(g=0),
           dict(g=4), dict(take=4), dict(take=-1), dict(acc=2), dict(acc=-1)]
    for kw in bad:
        assert comm(**kw) == -1, kw
        assert b"cm_comm_curves" in lib.cm_last_error(), kw
    assert comm(B=0) == 0 and comm(take=0) == 0

    for cells, T, n_epi, scen, N, sums, out in ((0, 5, 3, 0, 4, p, p), (2, 0, 3, 0, 4, p, p), (2, 5, 0, 0, 4, p, p), (2, 5, 3, 2, 4, p, p),
                                                (2, 5, 3, 0, 0, p, p), (2, 5, 3, 0, 256, p, p), (2, 5, 3, 1, 4, None, p),
                                                (2, 5, 3, 1, 4, p, None)):
        assert lib.cm_curve_means(cells, T, n_epi, scen, N, sums, out, None) == -1
        assert b"cm_curve_means" in lib.cm_last_error()
    for cells, T, n_epi, N, Lh, sums, out in ((0, 5, 3, 4, 2, p, p), (2, 0, 3, 4, 2, p, p), (2, 5, 0, 4, 2, p, p), (2, 5, 3, 0, 2, p, p),
                                              (2, 5, 3, 4, 0, p, p), (2, 5, 3, 4, 9, p, p), (2, 5, 3, 4, 2, None, p),
                                              (2, 5, 3, 4, 2, p, None)):
        assert lib.cm_comm_curve_means(cells, T, n_epi, N, Lh, sums, out, None) == -1
        assert b"cm_comm_curve_means" in lib.cm_last_error()


def test_kernels_have_no_private_segment_no_spill_no_flat_or_scratch_addressing_no_atomic_and_no_barrier():
    ks = isa.kernels(isa.listing("cm_episode_curves"))
    names = [k.name for k in ks]
    # the curves kernel with 16-byte and 4-byte adjacency positions and its means kernel (the comm family's two are shared
    # reductions of cm_stat_rows: tests/test_stat_rows_isa.py)
    assert len(ks) == 3, names
    assert sum("episode_curves_kernel" in n for n in names) == 2 and sum("curve_means_kernel" in n for n in names) == 1
    for k in ks:
        assert k.private_segment_fixed_size == 0, k.name
        assert k.vgpr_spill_count == 0, k.name
        assert not k.has_flat_or_scratch, k.name
        assert k.count("global_atomic") == 0 and k.count("ds_add") == 0 and k.barriers == 0, k.name


# ---- a hand-made round: T = 4, N = 2, three envs in one group ------------------------------------------------------------------
REWARD = np.array([[1.5, 1.0, 0.5], [-0.25, 2.0, 0.0], [2.0, 3.0, 8.0], [4.0, 5.0, 16.0]])
DETAILS = np.array([[1, 2, 3, 4, 5, 9], [2, 0, 1, 1, 1, 9], [0, 4, 0, 2, 3, 9], [3, 2, 2, 0, 1, 9]], np.int32)
SUCCESS = np.array([[0, 1, 1], [1, 0, 1], [0, 0, 1], [1, 1, 1]], np.int32)
# slot sums 2, 4, 0, 3, 1 for every env
ADJ = np.array([[[1, 0], [0, 1]], [[1, 1], [1, 1]], [[0, 0], [0, 0]], [[1, 1], [0, 1]], [[0, 0], [1, 0]]], np.float32)
PATH_LEN = np.array([[0, 1, 0], [2, 0, 0], [0, 0, 0], [2, 3, 0]], np.int32)     # n = 2 (a second end later), 1, 4 (never ends)


def _round(scenario, adj=True, take=3, acc=0, sums=None):
    det = np.repeat(DETAILS[:, None], 3, 1)
    a = np.repeat(ADJ[:, None], 3, 1) if adj else None
    sums = np.full((1, 4, 9), -7.0) if sums is None else sums
    return V.episode_curves(REWARD, det, SUCCESS, PATH_LEN, a, 2, 3, take, acc, sums)


def test_written_down_answers_of_a_hand_made_round():
    s = _round(R.PP)
    # step 0: all three run; env 1 is at its terminal step (n = 1: slot 0, sum 2), the others read slot 1 (sum 4)
    assert s[0, 0].tolist() == [2.0, 3.0, 3.0, 3.0, 6.0, 9.0, 10.0, 15.0, 12.0]
    # step 1: env 0 (terminal: slot n-1 = 1, sum 4) and env 2 (slot 2, sum 0); step 2, 3: env 2 alone (slots 3 and, terminal, 3)
    assert s[0, 1].tolist() == [2.0, -0.25, 4.0, 2.0, 0.0, 2.0, 4.0, 2.0, 2.0]
    assert s[0, 2].tolist() == [1.0, 8.0, 0.0, 1.0, 4.0, 0.0, 3.0, 3.0, 2.0]
    assert s[0, 3].tolist() == [1.0, 16.0, 3.0, 1.0, 2.0, 2.0, 3.0, 1.0, 0.0]
    c = V.curve_means(s, 3, R.PP, 2)
    assert c[0, :, 3].tolist() == [1.0, 2 / 3, 1 / 3, 1 / 3]                       # the share of episodes still running
    assert c[0, 0].tolist() == [2 / 3, 1.0, 1.0, 1.0, 1.0, 3.0, 10 / 6, 2.5, 0.0]
    assert V.curve_means(s, 3, R.CO, 2)[0, 0].tolist() == [2 / 3, 1.0, 0.5, 1.0, 1.0, 1.5, 10 / 6, 2.5, 2.0]
    # the constant full graph: N per running episode
    assert V.curve_means(_round(R.PP, adj=False), 3, R.PP, 2)[0, :, 6].tolist() == [2.0, 4 / 3, 2 / 3, 2 / 3]
    # take = 2 leaves env 2 out; a second round with accumulate = 1 adds to the first, take = 0 writes nothing
    two = _round(R.PP, take=2)
    assert two[0, :, 3].tolist() == [2.0, 1.0, 0.0, 0.0] and (two[0, 2:] == 0.0).all()
    both = _round(R.PP, take=2, acc=1, sums=s.copy())
    assert (both == s + two).all()
    assert (_round(R.PP, take=0) == -7.0).all()
    # a step's curve summed over the steps is the mean of the episodes' sums: cm_episode_stats's rows
    rows = np.zeros((3, 9))
    R.episode_stats(REWARD, np.repeat(DETAILS[:, None], 3, 1), SUCCESS, PATH_LEN, np.repeat(ADJ[:, None], 3, 1), 2, R.PP, 3, 3, 3, 0, rows)
    for col in (1, 2, 3, 4, 5, 7, 8):
        assert c[0, :, col].sum() == pytest.approx(rows[:, col].mean(), rel=1e-15)


def test_comm_curves_written_down():
    stats = np.arange(5 * 3 * 4, dtype=np.int32).reshape(5, 3, 4)
    s = V.comm_curves(PATH_LEN, stats, 3, 3, 0, np.full((1, 4, 4), -7.0))
    assert s[0, 0].tolist() == (stats[0, 0] + stats[0, 1] + stats[0, 2]).tolist()
    assert s[0, 1].tolist() == (stats[1, 0] + stats[1, 2]).tolist() and s[0, 3].tolist() == stats[3, 2].tolist()   # slot t, never T
    c = V.comm_curve_means(s, 3, 2, 2)
    assert c[0, 3].tolist() == [stats[3, 2, 0] / 6, stats[3, 2, 1] / 12, stats[3, 2, 2] / 6, stats[3, 2, 3] / 6]
    assert V.delivery(np.array([[0.0, 0.0, 0, 0], [2.0, 1.0, 0, 0]])).tolist() == [1.0, 0.5]
    # summed over the steps and the n N per episode put back: cm_episode_comm's rows, as integers
    rows = np.zeros((3, 4))
    comm_ref.episode_comm(PATH_LEN, stats, 2, 2, 3, 3, 3, 0, rows)
    n = np.array([2, 1, 4])
    assert s[0, :, 0].sum() == (rows[:, 0] * n * 2).sum() and s[0, :, 1].sum() == (rows[:, 1] * n * 4).sum()


@pytest.mark.parametrize("scenario,N,with_adj", [(R.PP, 4, True), (R.CO, 5, True), (R.PP, 3, False), (R.CO, 24, True)])
def test_restatement_equals_the_reference_rule_on_the_host_loop_of_eval_models(scenario, N, with_adj):
    """evaluate._episode on the host arrays the evaluation rounds would hand it (degrees rounded to f32 per step, as torch computes
    them), zero-padded to T and averaged: whole-valued columns equal up to the one division; the others within the bound on two
    E-term f64 sums in different orders, / E (the host sums d / nA per step); nodeDeg additionally to rtol 2^-23."""
    import torch
    from com_marl_amd.evaluate import VECTORS, _episode
    T, B, take = 33, 12, 11
    buf = R.buffers(T, B, N, seed=11 + N, with_adj=with_adj)
    assert set(buf["kinds"]) == set(R.KINDS)
    ended = buf["path_len"] > 0
    first = np.where(ended.any(0), ended.argmax(0), T - 1)
    h = dict(first=first, reward=buf["reward"], details=buf["details"], success=buf["success"])
    if with_adj:
        h["deg"] = torch.from_numpy(buf["dist_adj"]).sum(-1).mean(-1).numpy()
    sums = np.zeros((1, T, 9))
    V.episode_curves(buf["reward"], buf["details"], buf["success"], buf["path_len"], buf["dist_adj"], N, B, take, 0, sums)
    got = V.curve_means(sums, take, scenario, N)[0]
    eps = [_episode(h, b, N, scenario == R.PP) for b in range(take)]
    lists = {vec: [cols[vec] for _, cols, _ in eps] for vec in VECTORS}
    lists["success"] = [buf["success"][:n, b] for b, (n, _, _) in enumerate(eps)]
    whole = {"success", "step_cnt"} | ({"capture_cnt", "penalty_cnt", "vars2"} if scenario == R.PP else set())
    for c, name in enumerate(R.COLS):
        want, mean_abs = V.padded_mean(lists[name], T)
        bound = R.sum_bound(take, mean_abs * take) / take
        if name in whole:
            bound = np.zeros(T)                                  # the same integer, divided once here and by np.mean there
        if name == "nodeDeg":
            bound = bound + 2.0 ** -23 * np.abs(want)
        assert (np.abs(got[:, c] - want) <= bound).all(), (name, np.abs(got[:, c] - want).max())
    assert got[0, 3] == 1.0 and (np.diff(got[:, 3]) <= 0).all() and got[-1, 3] > 0
