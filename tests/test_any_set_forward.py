"""The policy-set forward for Comm-DP nets of any - also mixed - layer sizes at the C ABI: ONE cm_policy_forward_any_multi launch
over a set of differently sized members, each on its own contiguous envs, must equal - bit for bit - one act_device
(cm_policy_forward_any) per member on its slice with env_id_offset + the slice's first env."""
import ctypes as C

import numpy as np
import pytest

from tests import any_set_members as M
from tests import any_shapes

pytestmark = pytest.mark.gpu

GUARD = 64
SEED, OFF, STEP, BASE = 11, 1000, 7, 1000
# (N, d, hops), members, envs per workgroup
CASES = [((5, 21, 1), ("m0", "m1", "m2"), 9), ((4, 21, 2), ("m0", "m1", "m2"), 12), ((24, 77, 2), ("m0", "m1", "m2"), 2),
         ((72, 53, 2), ("m0", "m1"), 1)]
IDS = [f"N{c[0][0]}_d{c[0][1]}_L{c[0][2]}" for c in CASES]

_built = {}


def _case(shape, fams, epb):
    """The case's members, inputs and per-member reference outputs {(greedy, masks): (actions, probs, attn)}: built once, shared
    by the case's four tests and left unchanged."""
    key = (shape, fams)
    if key in _built:
        return _built[key]
    import torch
    N, d, hops = shape
    assert M.epb_of(N) == epb
    sizes = [2 * epb + 1, 1, 3 * epb + 1][:len(fams)]                 # a group of one; with epb > 1 every group ends ragged
    if epb > 1:
        assert all(s % epb for s in sizes)
    S = sum(sizes)
    pols = [M.build(f, N, d, hops, seed=40 + k, rng_seed=SEED) for k, f in enumerate(fams)]
    obs, avail, adj, ch = (torch.as_tensor(x).cuda() for x in any_shapes.inputs(N, d, hops, S=S))
    assert float(avail.min()) == 0.0 and float(adj[1, N - 1].sum()) == 0.0          # the awkward masks are there
    base = torch.full((1,), BASE, dtype=torch.int32, device="cuda:0")
    refs = {}
    for greedy in (True, False):
        for masks in ("const", "explicit"):
            av, ad, c = (avail, adj, ch) if masks == "explicit" else (None, None, None)
            outs, lo = [], 0
            for k, n in enumerate(sizes):
                cut = lambda x: None if x is None else x[lo:lo + n]                   # noqa: E731
                a, p, m = pols[k].act_device(obs[lo:lo + n], cut(av), cut(ad), cut(c), greedy=greedy, policy_step=STEP,
                                             step_base=base, env_id_offset=OFF + lo)
                assert pols[k]._last_forward == "one_launch"
                outs.append((a, p, m))
                lo += n
            refs[(greedy, masks)] = tuple(torch.cat([o[i] for o in outs]).cpu().numpy() for i in range(3))
    # the inputs bite: on identical observations the members' probabilities differ
    same_obs = obs[:1].expand(len(pols), -1).contiguous()
    pr = [p.act_device(same_obs[k:k + 1], None, None, None, greedy=True, policy_step=0)[1].cpu().numpy() for k, p in enumerate(pols)]
    for k in range(1, len(pols)):
        assert not np.array_equal(pr[k], pr[0])
    _built[key] = dict(sizes=sizes, S=S, pols=pols, obs=obs, avail=avail, adj=adj, ch=ch, base=base, refs=refs)
    return _built[key]


def _bands_unwritten(flat, fill):
    for band in (flat[:GUARD], flat[-GUARD:]):
        b = band.cpu().numpy()
        assert np.isnan(b).all() if fill is None else (b == fill).all(), "guard band written"


@pytest.mark.parametrize("masks", ["const", "explicit"])
@pytest.mark.parametrize("greedy", [True, False])
@pytest.mark.parametrize("shape,fams,epb", CASES, ids=IDS)
def test_one_launch_equals_a_launch_per_member(shape, fams, epb, greedy, masks):
    import torch
    from com_marl_amd import _lib as L, nets
    N, d, hops = shape
    c = _case(shape, fams, epb)
    sizes, S, pols = c["sizes"], c["S"], c["pols"]
    A = 5
    ps = nets.PolicySet(pols, any_sizes=True)
    assert ps.set_kernel == "any" and not ps.uniform
    table, n_wg = ps.forward_table(sizes)
    assert table is not None and n_wg == sum(-(-n // epb) for n in sizes)
    assert 0 < ps.forward_lds <= M.LDS_LIMIT and ps.forward_lds == max(M.plan(N, d, f)[2] for f in fams)
    assert ps.forward_table(sizes)[0] is table                          # kept while groups and weight buffers stay
    avail, adj, ch = (c["avail"], c["adj"], c["ch"]) if masks == "explicit" else (None, None, None)
    fa, act = M.guarded(torch, (S, N), torch.int32, -7, GUARD)
    fp, probs = M.guarded(torch, (S, N, A), torch.float32, float("nan"), GUARD)
    fm, attn = M.guarded(torch, (S, N, N), torch.float32, float("nan"), GUARD)
    w = pols[-1]._net_struct()                                          # any member's: the shared dims are read
    rc = L.lib().cm_policy_forward_any_multi(
        C.byref(w), L.ptr(table), n_wg, S, ps.forward_lds, L.ptr(c["obs"]), L.ptr(avail), L.ptr(adj), L.ptr(ch), SEED, OFF, STEP,
        L.ptr(c["base"]), int(greedy), L.ptr(act), L.ptr(probs), L.ptr(attn), L.current_stream())
    assert rc == 0, (rc, L.lib().cm_last_error())
    torch.cuda.synchronize()
    ref_a, ref_p, ref_m = c["refs"][(greedy, masks)]
    np.testing.assert_array_equal(act.cpu().numpy(), ref_a)
    np.testing.assert_array_equal(probs.cpu().numpy(), ref_p)
    np.testing.assert_array_equal(attn.cpu().numpy(), ref_m)
    assert not np.isnan(ref_p).any() and not np.isnan(ref_m).any() and (ref_a >= 0).all() and (ref_a < A).all()
    _bands_unwritten(fa, -7)
    _bands_unwritten(fp, None)
    _bands_unwritten(fm, None)
    if not greedy:                                                      # sampling really draws
        assert not np.array_equal(ref_a, c["refs"][(True, masks)][0])
    if masks == "explicit":                                             # a forbidden action has probability zero and is never taken
        av = c["avail"].cpu().numpy()
        assert (ref_p[av == 0] == 0).all() and (np.take_along_axis(av, ref_a[..., None].astype(np.int64), -1) == 1).all()


def test_launch_checks_the_table_and_workgroup_count():
    import torch
    from com_marl_amd import _lib as L, nets
    shape, fams, epb = CASES[2]
    c = _case(shape, fams, epb)
    N = shape[0]
    ps = nets.PolicySet(c["pols"], any_sizes=True)
    table, n_wg = ps.forward_table(c["sizes"])
    S = c["S"]
    act = torch.full((S, N), -7, dtype=torch.int32, device="cuda:0")
    w = c["pols"][0]._net_struct()

    def launch(tab, wg, lds):
        return L.lib().cm_policy_forward_any_multi(C.byref(w), L.ptr(tab), wg, S, lds, L.ptr(c["obs"]), None, None, None, SEED, 0, 0,
                                                   None, 1, L.ptr(act), None, None, L.current_stream())

    lds = ps.forward_lds
    for tab, wg, nbytes in ((None, n_wg, lds), (table, -(-S // epb) - 1, lds), (table, S + 1, lds), (table, n_wg, 1024)):
        assert launch(tab, wg, nbytes) < 0 and L.lib().cm_last_error()
    assert launch(table, n_wg, 0) == 1 and launch(table, n_wg, M.LDS_LIMIT + 4) == 1
    torch.cuda.synchronize()
    assert (act == -7).all()


def test_a_set_with_a_member_above_the_lds_limit_is_declined():
    """m2 at N = 72, d = 53 needs 168 960 B of planes alone: no table, and the launch answers 1 having written nothing."""
    import torch
    from com_marl_amd import _lib as L, nets
    N, d, hops = 72, 53, 2
    shape, fams, epb = CASES[3]
    pols = _case(shape, fams, epb)["pols"] + [M.build("m2", N, d, hops, seed=42, rng_seed=SEED)]
    ps = nets.PolicySet(pols, any_sizes=True)
    assert ps.forward_table([3, 1, 4]) == (None, 0) and ps.forward_lds == 0
    obs = torch.rand(8, N, d, device="cuda:0")
    act = torch.full((8, N), -7, dtype=torch.int32, device="cuda:0")
    dummy = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    for w, lds in ((pols[2]._net_struct(), 129088), (pols[0]._net_struct(), M.plan(N, d, "m2")[2]), (pols[0]._net_struct(), 0)):
        rc = L.lib().cm_policy_forward_any_multi(C.byref(w), L.ptr(dummy), 8, 8, lds, L.ptr(obs), None, None, None, SEED, 0, 0, None, 1,
                                                 L.ptr(act), None, None, L.current_stream())
        assert rc == 1                                      # "not for this shape": nothing launched
    torch.cuda.synchronize()
    assert (act == -7).all()
