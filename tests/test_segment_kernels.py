"""The rollout-segment kernels (csrc/cm_segments.hip) against the float64 reference of tests/segments_ref.py.

Tolerances are derived from the number formats (u = 2^-24, the unit roundoff of f32), not from what the kernels give:
  returns     the f64 recurrence is the reference's own, cast once: |err| <= u |R_t|
  advantages  the final cast, u |A_t|, plus every f32 delta of the rest of the piece (cast of r, gamma * V, the sum, the
              difference: <= 4u times the size of its terms), weighted as the accumulator weights it: segments_ref.adv_bound
  normalised  (x - (float)mean) * (1 / sqrtf((float)var + eps)): u (3 |x| + 2 |mean| / std)
The reference takes the recurrences' coefficients as the kernel is specified to form them (segments_ref.kernel_coefficients)."""
import numpy as np
import pytest

from tests import segments_ref as R

pytestmark = pytest.mark.gpu

GAMMA, LAM, EPS = 0.99, 0.97, 1e-8
CASES = [(70, 37), (1, 1), (3, 2)]          # two workgroups, the second ragged; the smallest; a small one with every override
_DATA = {}


@pytest.fixture
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need the MI355X")
    return torch


def _case(P, T):
    """Inputs and their float64 reference, computed once per case and left unchanged."""
    if (P, T) not in _DATA:
        rng = np.random.default_rng(1000 * P + T)
        rew = rng.normal(size=(P, T))
        val = rng.normal(size=(P, T)).astype(np.float32)
        x = rng.normal(size=P)
        v_last = np.where(x >= 0, x + 0.5, x - 0.5).astype(np.float32)          # non-zero everywhere
        dones = R.draw_dones(P, T, rng)
        g, gl, gr = R.kernel_coefficients(GAMMA, LAM)
        ref = R.segment_targets(rew, dones, val, v_last, g, gl, gr)
        ref0 = R.segment_targets(rew, dones, val, np.zeros(P), g, gl, gr)
        _DATA[P, T] = dict(rew=rew, val=val, v_last=v_last, dones=dones, ref=ref, ref0=ref0)
    return _DATA[P, T]


def _targets(torch, L, c, v_last, time_major=True):
    P, T = c["rew"].shape
    rew, dn = torch.as_tensor(c["rew"]), torch.as_tensor(c["dones"].astype(np.uint8))
    if time_major:                                                               # the engine's layout: [T, P]
        rew, dn, strides = rew.t().contiguous().cuda(), dn.t().contiguous().cuda(), (1, P)
    else:
        rew, dn, strides = rew.contiguous().cuda(), dn.contiguous().cuda(), (T, 1)
    val, vl = torch.as_tensor(c["val"]).cuda(), torch.as_tensor(np.asarray(v_last, np.float32)).cuda()
    adv = torch.full((P, T), float("nan"), device="cuda")
    ret = torch.full((P, T), float("nan"), device="cuda")
    L.check(L.lib().cm_segment_targets(P, T, L.ptr(rew), L.ptr(dn), *strides, L.ptr(val), L.ptr(vl), GAMMA, LAM, L.ptr(adv),
                                       L.ptr(ret), L.current_stream()), "cm_segment_targets")
    torch.cuda.synchronize()
    return adv.cpu().numpy(), ret.cpu().numpy()


@pytest.mark.parametrize("P,T", CASES)
def test_targets_against_float64(P, T, gpu):
    torch = gpu
    from com_marl_amd import _lib as L
    c = _case(P, T)
    d = c["dones"]
    if (P, T) == (70, 37):                      # the set holds: no done, only the last step, a done at step 0, two in a row
        assert not d[0].any() and d[1].sum() == 1 and d[1, -1] and d[2, 0] and d[3, 1] and d[3, 2]
        assert 0.05 < d[4:].mean() < 0.15
    assert (c["v_last"] != 0).all()
    adv, ret = _targets(torch, L, c, c["v_last"])
    adv64, ret64, terms = c["ref"]
    e_ret, e_adv = np.abs(ret - ret64), np.abs(adv - adv64)
    b_ret, b_adv = R.U * np.abs(ret64), R.adv_bound(adv64, terms)
    print(f"\n({P}, {T}): returns worst err/bound {np.max(e_ret / np.maximum(b_ret, 1e-300)):.3f}, "
          f"advantages worst err/bound {np.max(e_adv / b_adv):.3f}")
    assert (e_ret <= b_ret).all()
    assert (e_adv <= b_adv).all()
    # the [P,T] layout of the same data: the same bits
    adv_r, ret_r = _targets(torch, L, c, c["v_last"], time_major=False)
    assert adv_r.tobytes() == adv.tobytes() and ret_r.tobytes() == ret.tobytes()
    # a row that ends in a done never sees v_last; the others do
    adv2, ret2 = _targets(torch, L, c, -3.0 * c["v_last"])
    ends = d[:, -1]
    assert adv2[ends].tobytes() == adv[ends].tobytes() and ret2[ends].tobytes() == ret[ends].tobytes()
    for p in np.nonzero(~ends)[0]:
        first = R.pieces(d[p])[-1][0]
        assert (ret2[p, first:] != ret[p, first:]).all() and adv2[p, -1] != adv[p, -1]
        assert adv2[p, :first].tobytes() == adv[p, :first].tobytes() and ret2[p, :first].tobytes() == ret[p, :first].tobytes()


@pytest.mark.parametrize("P,T", CASES)
def test_pieces_are_the_whole_path_kernels_on_each_piece_alone(P, T, gpu):
    """v_last = 0: every piece between dones is what cm_gae (normalize = 0, lens = NULL) and cm_discount_returns give for that
    piece as a path of its own.  Pieces of one length share a launch (rows of a batch are independent)."""
    torch = gpu
    from com_marl_amd import _lib as L
    lib = L.lib()
    c = _case(P, T)
    adv, ret = _targets(torch, L, c, np.zeros(P, np.float32))
    adv64, ret64, terms = c["ref0"]
    b_adv, b_ret = R.adv_bound(adv64, terms), R.U * np.abs(ret64)
    by_len = {}
    for p in range(P):
        for first, last in R.pieces(c["dones"][p]):
            by_len.setdefault(last - first + 1, []).append((p, first))
    n_pieces, equal = 0, True
    for n, where in sorted(by_len.items()):
        rows = np.array([[p * T + first + k for k in range(n)] for p, first in where])
        r64 = torch.as_tensor(c["rew"].reshape(-1)[rows]).cuda()
        r32, v32 = r64.to(torch.float32).contiguous(), torch.as_tensor(c["val"].reshape(-1)[rows]).cuda()
        a, y = torch.full((len(where), n), float("nan"), device="cuda"), torch.full((len(where), n), float("nan"), device="cuda")
        L.check(lib.cm_gae(len(where), n, L.ptr(r32), L.ptr(v32), None, GAMMA, LAM, 0, EPS, L.ptr(a), L.current_stream()), "cm_gae")
        L.check(lib.cm_discount_returns(len(where), n, L.ptr(r64), None, GAMMA, L.ptr(y), L.current_stream()), "cm_discount_returns")
        torch.cuda.synchronize()
        a, y = a.cpu().numpy(), y.cpu().numpy()
        assert (np.abs(a - adv.reshape(-1)[rows]) <= b_adv.reshape(-1)[rows]).all(), n
        assert (np.abs(y - ret.reshape(-1)[rows]) <= b_ret.reshape(-1)[rows]).all(), n
        equal &= a.tobytes() == adv.reshape(-1)[rows].tobytes() and y.tobytes() == ret.reshape(-1)[rows].tobytes()
        n_pieces += len(where)
    assert n_pieces >= P
    print(f"\n({P}, {T}): {n_pieces} pieces of {len(by_len)} lengths, bit-equal to cm_gae / cm_discount_returns: {equal}")


def _normalize(torch, L, x):
    nb = L.lib().cm_adv_normalize_ws_bytes()
    ws = torch.full((nb // 8,), float("nan"), dtype=torch.float64, device="cuda")           # a partial read unwritten shows
    a = torch.as_tensor(x).cuda()
    L.check(L.lib().cm_adv_normalize(a.numel(), L.ptr(a), EPS, L.ptr(ws), nb, L.current_stream()), "cm_adv_normalize")
    torch.cuda.synchronize()
    return a.cpu().numpy()


def test_adv_normalize_against_float64(gpu):
    torch = gpu
    from com_marl_amd import _lib as L
    x = np.random.default_rng(2590).normal(0.7, 1.9, 2590).astype(np.float32)
    mean, std = float(x.astype(np.float64).mean()), float(x.astype(np.float64).std())
    assert std >= abs(mean)
    want = R.adv_normalize(x, EPS)
    got = _normalize(torch, L, x)
    bound = R.U * (3 * np.abs(want) + 2 * abs(mean) / std)
    err = np.abs(got - want)
    print(f"\n2590 values: worst err/bound {np.max(err / bound):.3f}; mean {got.astype(np.float64).mean():.2e}, "
          f"std {got.astype(np.float64).std():.8f}")
    assert (err <= bound).all()
    assert _normalize(torch, L, x).tobytes() == got.tobytes()                               # two runs, identical bits
    # more than one workgroup (4 x 256 values each) and a ragged last round
    big = np.random.default_rng(7).normal(-0.2, 1.0, 5 * 1024 + 3).astype(np.float32)
    w = R.adv_normalize(big, EPS)
    m, s = float(big.astype(np.float64).mean()), float(big.astype(np.float64).std())
    g = _normalize(torch, L, big)
    assert (np.abs(g - w) <= R.U * (3 * np.abs(w) + 2 * abs(m) / s)).all()
    assert _normalize(torch, L, big).tobytes() == g.tobytes()


@pytest.mark.parametrize("value", [0.0, 0.75])
def test_adv_normalize_of_one_value(value, gpu):
    """count = 1: mean = the value, variance 0 (std >= |mean| only for 0.0; any other value is normalised to exactly 0 too)."""
    torch = gpu
    from com_marl_amd import _lib as L
    x = np.array([value], np.float32)
    got = _normalize(torch, L, x)
    assert R.adv_normalize(x, EPS)[0] == 0.0 and got[0] == 0.0
    assert _normalize(torch, L, x).tobytes() == got.tobytes()


def test_episode_bookkeeping_against_numpy(gpu):
    """Synthetic slots, 300 envs (two workgroups, the second ragged), two segments of 7 and 5 steps in a row: every table equals
    numpy's over the episodes that ended in that segment, the records carry the open episodes across the border."""
    torch = gpu
    from com_marl_amd import _lib as L
    B, gamma = 300, 0.99
    rng = np.random.default_rng(11)
    nb = L.lib().cm_segment_episodes_ws_bytes(B)
    rec_f = torch.zeros(3, B, dtype=torch.float64, device="cuda")
    rec_f[2].fill_(1.0)
    rec_i = torch.zeros(6, B, dtype=torch.int64, device="cuda")
    carry, seen = None, 0
    for n in (7, 5):
        rew = rng.normal(size=(n, B))
        done = rng.random((n, B)) < 0.15
        done[:, 0] = False                                                       # an env whose episode never ends
        done[:, 1] = True                                                        # one whose every step is an episode
        det = rng.integers(0, 5, (n, B, 6)).astype(np.int32)
        succ = rng.integers(0, 2, (n, B)).astype(np.int32)
        eps, carry = R.episodes(rew, done, det, succ, gamma, carry)
        want = R.episode_table(eps)
        table = torch.full((L.SEG_COLS,), float("nan"), dtype=torch.float64, device="cuda")
        ws = torch.full((nb // 8,), float("nan"), dtype=torch.float64, device="cuda")
        dev = [torch.as_tensor(a).cuda() for a in (rew, done.astype(np.uint8), det, succ)]
        L.check(L.lib().cm_segment_episodes(n, B, *[L.ptr(t) for t in dev], gamma, L.ptr(rec_f), L.ptr(rec_i), L.ptr(table), L.ptr(ws),
                                            nb, L.current_stream()), "cm_segment_episodes")
        torch.cuda.synchronize()
        got = dict(zip(L.SEG_COLUMNS, table.cpu().tolist()))
        for k in ("count", "ret_min", "ret_max", "len_sum", "success") + tuple(f"details_{j}" for j in range(5)):
            assert got[k] == want[k], (n, k, got[k], want[k])
        for k in ("ret_sum", "ret_sumsq", "disc_sum"):
            assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (n, k, got[k], want[k])
        seen += len(eps)
        f, i = rec_f.cpu().numpy(), rec_i.cpu().numpy()
        for b in (0, 1, 2, 255, 256, B - 1):
            cb = carry[b]
            assert abs(f[0, b] - cb["ret"]) <= 1e-12 * max(1.0, abs(cb["ret"])) and abs(f[1, b] - cb["disc"]) <= 1e-12 * max(1.0, abs(cb["disc"]))
            assert abs(f[2, b] - cb["gp"]) <= 1e-15 and i[0, b] == cb["n"] and (i[1:, b] == cb["det"]).all()
    assert seen > 2 * B * 0.1 and carry[0]["n"] == 12 and carry[1]["n"] == 0
    # no episode ends: count 0, sums 0, min / max at their neutral values
    none = torch.zeros(3, B, dtype=torch.uint8, device="cuda")
    table = torch.full((L.SEG_COLS,), float("nan"), dtype=torch.float64, device="cuda")
    L.check(L.lib().cm_segment_episodes(3, B, L.ptr(dev[0]), L.ptr(none), L.ptr(dev[2]), L.ptr(dev[3]), gamma, L.ptr(rec_f), L.ptr(rec_i),
                                        L.ptr(table), L.ptr(ws), nb, L.current_stream()), "cm_segment_episodes")
    got = dict(zip(L.SEG_COLUMNS, table.cpu().tolist()))
    assert got["count"] == 0 and got["ret_sum"] == 0 and got["ret_min"] == np.inf and got["ret_max"] == -np.inf
