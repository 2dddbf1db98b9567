"""CPU side of tests/test_dense_layer_kernels_f64.py (the dense-layer kernels against float64 on every dispatch route): everything that
can be known about its cases before a kernel runs, from float64 and a float32 emulation alone (tests/f64_dense.py).

  * the case table is what it says: route() of every case is the route written beside it, the row counts are the seven allowed ones
    (144705 for at most three stream cases), and route() over CASES reaches every route of ROUTES_REQUIRED - forward tile splits OT
    1, 2, 3, 4, an odd one in 5..7 and 8; the eight + one stream builds at act 0 and 1 and the two ReLU ones; the nine ragged
    (kt, O) builds and their three ReLU ones; MAXT 1 / 2 / 4 / 8 / 16 of the generic backward and of wgrad; every fall-through to the
    generic kernel (width, 128x128, unaligned, layout1, no-relu, ragged-no-relu, lds);
  * ref64 is float64 torch autograd of act(x W^T + b) (layout 0) or act(x W) (layout 1) at 1e-12 of each tensor, for every case of
    at most 2555 rows.  The backward's saved y is a given, not the layer's own output, so autograd is run on act(z + s) with the
    constant shift s that makes the float64 output equal the given y (tanh: atanh(y) - z, and +-20 - z where y = +-1, which
    float64 tanh returns exactly; ReLU: y - z where y > 0, -1 - z where y = 0);
  * the inputs are fair: emu32 - float32 with the kernels' chunk / workgroup / merge summation - stays within HALF of every applied
    bar for every case.  A kernel ratio above a bar is then a kernel finding, not float32 noise.  (The two forward cases with
    pre-activations of 1e-2 / 1e-3 are held to the whole bar: it is tanh_exact's documented absolute bound there, and the same
    form in float32 comes to 0.6 of it);
  * negative controls, built in float64 from the reference, never by running anything wrong, and handed to the same judge():
        last_row, last_chunk (rows left out of the sums, their rows of y / dx zero); last_k_column (forward and the ragged first
        layer); no_dy2; no_act_derivative; other_layout (dW transposed into the same buffer, non-square pairs); db_first_chunk;
        overwritten (the accumulated outputs judged against ref64 when they started at 2.5).
    Each is rejected wherever it applies.  Those that COINCIDE with the right answer are asserted to coincide, by name: no_dy2 of a
    case without dy2, no_act_derivative of an identity layer, db_first_chunk of a case of at most 64 rows, other_layout of a weight
    that is a vector (K or O = 1: bwd 1 -> 32)."""
import numpy as np
import pytest
import torch

from tests import f64_dense as D

NAMES = [c.name for c in D.CASES]

ROUTES_REQUIRED = (
    [f"fwd/OT{n}" for n in (1, 2, 3, 4, 8)]
    + [f"stream/{k}x{o}/L0/act{a}" for k in D.STREAM_W for o in D.STREAM_W if (k, o) != (128, 128) for a in (0, 1)]
    + ["stream/64x64/L1/act0", "stream/64x64/L1/act1", "stream/64x32/L0/act2", "stream/128x64/L0/act2"]
    + [f"ragged/kt{kt}x{o}/act" for kt in (2, 4, 8) for o in D.STREAM_W]
    + [f"ragged/kt{kt}x128/act2" for kt in (2, 4, 8)]
    + [f"{k}/MAXT{m}" for k in ("generic", "wgrad") for m in (1, 2, 4, 8, 16)]
    + [f"generic/MAXT{m}/{why}" for m, why in ((16, "128x128"), (4, "unaligned"), (2, "layout1"), (4, "no-relu"), (2, "ragged-no-relu"),
                                              (16, "lds"), (1, "width"))])


def test_the_table_is_what_it_says():
    for c in D.CASES:
        assert D.route_of(c) == c.route, f"{c.name}: route() says {D.route_of(c)}, the table {c.route}"
        assert c.R in D.ROW_COUNTS and 1 <= c.K <= 128 and 1 <= c.O <= 128, c.name
        assert c.note
    big = [c for c in D.CASES if c.R == 144705]
    assert len(big) <= 3 and all(c.route.startswith("stream/") for c in big)


def test_every_route_is_reached():
    reached = {D.route_of(c) for c in D.CASES}
    for r in ROUTES_REQUIRED:
        assert any(x.startswith(r) for x in reached), f"no case reaches {r}"
    assert any(x.startswith(f"fwd/OT{n}") for x in reached for n in (5, 7)), "no odd forward tile split in 5..7"
    # both staging branches of every entry that stages rows, the unaligned ones by the pointer test alone
    for r in ("fwd/OT4/vec", "fwd/OT4/sca", "wgrad/MAXT4/vecvec", "wgrad/MAXT4/scasca", "wgrad/MAXT1/vecvec"):
        assert r in reached, r
    # the row counts: every one used by each family that has a grid of its own
    for fam in ("fwd", "generic", "stream", "wgrad"):
        rs = {c.R for c in D.CASES if D.group(c) == fam}
        assert {1, 65, 2555, 32833} <= rs, (fam, rs)
    assert {c.R for c in D.CASES} == set(D.ROW_COUNTS)
    assert D.stream_grid(2555) == 34 and D.stream_grid(32833) == 122 and D.stream_grid(144705) == D.N_CU


def test_route_restates_the_lds_refusal():
    assert D.stream_lds(64, 128, 0, 1, True) == 160 * 1024 and D.stream_lds(128, 64, 0, 1, True) == 128 * 1024
    assert D.stream_lds(128, 128, 0, 1, False) == 160 * 1024 and D.stream_lds(128, 128, 0, 1, True) == 192 * 1024
    assert D.route("bwd", 127, 128, act=1, dx=False, dy2=False) == "ragged/kt8x128/act1"
    assert D.route("bwd", 127, 128, act=1, dx=False, dy2=True) == "generic/MAXT16/lds"


# ---- ref64 is autograd ------------------------------------------------------------------------------------------------------------
def _autograd(c, d):
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))              # noqa: E731
    if c.entry == "wgrad":
        a, b = t(d["a"]), t(d["b"])
        m = torch.zeros(c.K, c.O, dtype=torch.float64, requires_grad=True)
        s = torch.zeros(c.K, dtype=torch.float64, requires_grad=True)      # sum_r (a_r . (M b_r) + a_r . s): d/dM = a^T b, d/ds = colsum a
        loss = ((a @ m) * b).sum() + (a * s).sum()
        gm, gs = torch.autograd.grad(loss, (m, s))
        return {"c": gm.numpy(), "colsum": gs.numpy()}
    x, w = t(d["x"]).requires_grad_(True), t(d["w"]).requires_grad_(True)
    b = (t(d["bias"]) if c.entry == "fwd" and d["bias"] is not None else torch.zeros(c.O, dtype=torch.float64)).requires_grad_(True)
    z = (x @ w.T if c.layout == 0 else x @ w) + b
    f = torch.tanh if c.act == 1 else (torch.relu if c.act == 2 else (lambda v: v))
    if c.entry == "fwd":
        return {"y": f(z).detach().numpy()}
    if c.act:
        y = t(d["y"])
        sat = 20.0 * torch.sign(y)                                          # tanh(+-20) = +-1 exactly in float64: tanh' = 0
        shift = (torch.where(y.abs() < 1, torch.atanh(y), sat) if c.act == 1
                 else torch.where(y > 0, y, torch.full_like(y, -1.0))) - z.detach()
        z = z + shift
    g = t(d["dy"]) + (t(d["dy2"]) if d["dy2"] is not None else 0.0)
    dx, dw, db = torch.autograd.grad(f(z), (x, w, b), g)
    return {"dx": dx.numpy(), "dw": dw.numpy(), "db": db.numpy()}


@pytest.mark.parametrize("name", [c.name for c in D.CASES if c.R <= 2555])
def test_ref64_is_float64_autograd(name):
    c = D.BY_NAME[name]
    ref, ag = D.reference(name), _autograd(c, D.build(name))
    for k, r in ref.items():
        assert np.abs(r - ag[k]).max() <= 1e-12 * max(np.abs(r).max(), 1e-30), (name, k)


# ---- the inputs are fair, the judge is not loose ----------------------------------------------------------------------------------
COINCIDES = {"no_dy2": lambda c: not c.dy2, "no_act_derivative": lambda c: c.act == 0, "db_first_chunk": lambda c: c.R <= D.ROWS,
             "other_layout": lambda c: min(c.K, c.O) == 1}


@pytest.mark.parametrize("name", NAMES)
def test_float32_alone_and_the_negative_controls(name):
    c, d, ref = D.BY_NAME[name], D.build(name), D.reference(name)
    emu = D.emu32(c, d)
    m = D.judge(c, ref, emu)
    print(f"{name} [{c.route}] float32 alone: " + "  ".join(f"{k} strict {s:.2e} applied {a:.2e}" for k, (s, a) in m.items()))
    # (the two small-pre-activation cases: their applied bar IS tanh_exact's documented 2e-7, which the same form in float32 comes
    # within 0.6 of - test_small_preactivations_need_the_absolute_bar - so there emu32 is held to the whole bar, not half)
    half = 1.0 if c.opts.startswith("z") else 0.5
    for k, (s, a) in m.items():
        assert a <= half * D.TAU, f"{name}: emu32 {k} at {a:.3g} of its scale, above {half} of the bar: the inputs are not fair"
        if not (k == "y" and c.act == 1):
            assert s == a, "only the forward's tanh output has an applied bar of its own"
    # 'sat': what must be exactly zero is exactly zero in the reference
    if c.opts == "sat":
        assert not ref["dw"][c.O // 2:].any() and not ref["db"][c.O // 2:].any() and not ref["dx"][:c.R // 2].any()
        assert ref["dw"][:c.O // 2].all()
    # negative controls: the reference itself (and emu32) must fail against each wrong answer - or coincide where listed
    ctl = D.controls(c)
    for what, (wrong, coincides) in ctl.items():
        assert coincides == (what in COINCIDES and COINCIDES[what](c)), (name, what)
        if coincides:
            assert all(np.array_equal(wrong[k], ref[k]) for k in wrong), f"{name}: {what} was said to coincide with the right answer"
        else:
            assert D.rejected(c, ref, wrong) and D.rejected(c, emu, wrong), f"{name}: the judge accepts '{what}'"
    # previous contents overwritten instead of added to
    acc = {k: v for k, v in ref.items() if k in D.ACCUMULATED}
    if acc:
        assert D.passes(D.judge(c, acc, {k: v + 2.5 for k, v in acc.items()}, init=2.5))
        assert not D.passes(D.judge(c, acc, acc, init=2.5)), f"{name}: the judge accepts overwritten accumulators"
    expect = {"last_row", "last_chunk"} | ({"db_first_chunk"} if c.entry == "bwd" and c.bias else set()) \
        | ({"other_layout"} if c.entry != "fwd" and c.K != c.O else set())
    if c.R <= D.FULL_RECOMPUTE_MAX_R:
        expect |= ({"no_dy2", "no_act_derivative"} if c.entry == "bwd" else set()) \
            | ({"last_k_column"} if c.entry == "fwd" or c.route.startswith("ragged") else set())
    assert set(ctl) == expect, (name, set(ctl) ^ expect)


def test_small_preactivations_need_the_absolute_bar():
    """tanh_exact's form in float32 misses the strict bar at |z| ~ 1e-3 (and sits near it at 1e-2) while its absolute error stays
    below 2e-7: the applied bar of the forward's tanh output, and why no other quantity has one."""
    for opts, lo in (("z1e-2", 1e-6), ("z1e-3", 1e-5)):
        c = next(c for c in D.CASES if c.opts == opts)
        d, ref = D.build(c.name), D.reference(c.name)
        emu = D.emu32(c, d)
        strict, applied = D.judge(c, ref, emu)["y"]
        err = np.abs(emu["y"].astype(np.float64) - ref["y"]).max()
        print(f"{c.name}: max|z| {np.abs(ref['y']).max():.2e}  float32 strict {strict:.2e} applied {applied:.2e} abs {err:.2e}")
        assert strict > lo and err <= D.TANH_ABS and applied <= D.TAU
