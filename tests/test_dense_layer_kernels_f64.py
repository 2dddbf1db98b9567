"""The dense-layer kernels on every dispatch route, called through the C ABI, against the float64 reference of tests/f64_dense.py
(its CASES / route / ref64 / emu32 / judge / controls; what holds of the cases before a kernel runs is tests/test_dense_cases_cpu.py):

  cm_linear_act_forward                                    one test per case of the forward
  cm_linear_act_backward, _ex, _det, _ex_det               one test per case, filed under the kernel route() sends it to: the generic
                                                           lin::bwd_kernel, the streaming lin2::bwd_kernel, its ragged first-layer form
  cm_linear_wgrad, _det                                    one test per case

What every case checks:
  * y / dx start as NaN with 64 guard rows of NaN behind them: every row is written, no guard row is;
  * dw / db (c / colsum_a) start at zero: judged against ref64 at TAU = 1e-5 of max|ref64| per tensor, dx and y per row as well
    (f64_dense.judge).  Strict, applied and float32-alone (emu32) ratios are printed per quantity;
  * the accumulation contract "dw +=, db +=": a second run whose accumulated outputs start at 2.5 is judged against ref64 + 2.5, the
    judge rejects it against ref64 alone ('overwritten'), and it equals the first run + 2.5
        - slab twins: exactly, fl(first + 2.5) (slab_reduce adds the index-ordered row sum to the output once);
        - atomic form, one workgroup (R <= 64): exactly, for the same reason;
        - atomic form, G > 1 workgroups: the G float atomics of an element land in any order, each rounding the running value, in
          the first run as in the second.  No running value exceeds 2.5 + T, T = sum_r |terms| of the element (f64_dense.term_sums),
          so the two runs differ by at most 2 G + 1 roundings of at most 2^-24 (2.5 + max T) each: that is the bar.  "One rounding
          of the sum" cannot be asked of unordered atomics - the first run alone moves by several between repeats; measured, in
          units of 2^-24 (2.5 + max|ref64|): up to 14.4 at 512 workgroups (wgrad 128 x 128, R = 32833);
  * each slab twin runs twice on a NaN-filled slab and is bit-equal; _det and _ex_det are bit-equal where both can name the layer;
  * 'sat' cases: dw rows / db entries of the saturated columns and dx of the saturated rows are exactly 0;
  * negative controls (f64_dense.controls): the kernel's output fails the same judge against every wrong answer that does not
    coincide with the right one.

Error paths: a slab one byte short is refused with nothing written; widths 0 and 129, w_layout 2 and a NULL dw are CM_ERR_ARG.

Worst ratios measured on the MI355X, kernel strict | kernel applied | float32 alone (emu32) strict; the bar is 1e-5:
  forward  y   1.43e-4 | 6.81e-6 | 1.43e-4   (strict: fwd R65 1x1 tanh, a one-element row 1e-3 of the tensor's size, where the
                                              absolute bar applies; identity / ReLU cases: strict = applied <= 6.7e-7; the other tanh
                                              cases at ordinary pre-activations: strict <= 5.3e-6, per row, emu32 the same)
           tanh_exact at pre-activations of 1e-2: absolute 1.36e-7, strict 8.04e-6; of 1e-3: absolute 1.36e-7, strict 8.06e-5
  generic  dx  9.22e-7 | 9.22e-7 | 9.40e-7   dw 8.50e-7 | 8.50e-7 | 8.50e-7   db 7.81e-7 | 7.81e-7 | 7.81e-7   (R32833 128x128)
  stream   dx  9.71e-7 | 9.71e-7 | 9.71e-7   dw 6.97e-7 | 6.97e-7 | 9.51e-7   db 3.65e-7 | 3.65e-7 | 6.97e-7   (R2555 64x128; R144705)
  ragged                                     dw 9.40e-7 | 9.40e-7 | 8.16e-7   db 2.95e-7 | 2.95e-7 | 6.26e-7   (R32833 21x128)
  wgrad    c   7.54e-7 | 7.54e-7 | 7.54e-7   colsum 4.51e-7 | 4.51e-7 | 4.37e-7                                 (R32833 128x128)
No applied bar but the forward's tanh output differs from its strict one; no case was found to fail."""
import functools

import numpy as np
import pytest
import torch

from tests import f64_dense as D

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
CM_ERR_ARG = -1
EPS = 2.0 ** -24


def _L():
    from com_marl_amd import _lib as L
    return L


def _p(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(a, off):
    """a float32 array on the device; off: one float into a larger allocation (4-byte aligned, not 16)"""
    if a is None:
        return None
    t = torch.from_numpy(np.array(a))
    if not off:
        return t.to(DEV).contiguous()
    buf = torch.zeros(t.numel() + 8, dtype=torch.float32, device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _guarded(R, W):
    return torch.full((R + GUARD, W), float("nan"), dtype=torch.float32, device=DEV)


def _nan_slab(nb):
    return torch.full((max(1, (int(nb) + 3) // 4),), float("nan"), dtype=torch.float32, device=DEV)


def _written(case, name, buf, R):
    assert bool(torch.isnan(buf[R:]).all()), f"{case}: {name} wrote into the guard rows behind it"
    return buf[:R]


def _report(c, what, m, emu_m):
    print(f"{c.name} [{c.route}] {what}: " + "  ".join(
        f"{k} strict {s:.2e} applied {a:.2e} f32 {emu_m[k][0]:.2e}" for k, (s, a) in m.items()))


@functools.lru_cache(maxsize=None)
def _float32_alone(name):
    c = D.BY_NAME[name]
    return D.judge(c, D.reference(name), D.emu32(c, D.build(name)))


@functools.lru_cache(maxsize=None)
def _term_sums(name):
    return D.term_sums(D.BY_NAME[name], D.build(name))


@functools.lru_cache(maxsize=None)
def _controls(name):
    return D.controls(D.BY_NAME[name])


def _judge_and_controls(c, got, what):
    ref = D.reference(c.name)
    m = D.judge(c, ref, got)
    _report(c, what, m, _float32_alone(c.name))
    for k, (s, a) in m.items():
        assert a <= D.TAU, f"{c.name} ({what}): {k} off by {a:.3g} of its scale (strict {s:.3g}; tolerance {D.TAU}) [{c.note}]"
    for name, (wrong, coincides) in _controls(c.name).items():
        if not coincides:
            assert D.rejected(c, got, wrong), f"{c.name} ({what}): negative control '{name}' passes: the check is too loose"
    if c.opts == "sat":
        h = c.O // 2
        dw = got["dw"] if c.layout == 0 else got["dw"].T
        assert not bool(dw[h:].any()) and not bool(got["db"][h:].any()) and not bool(got["dx"][:c.R // 2].any()), \
            f"{c.name} ({what}): a saturated unit's dz is not exactly 0"
    return m


def _accumulates(c, what, first, second, grid, exact):
    """second (accumulated outputs started at 2.5) against first (started at 0): see the header"""
    ref = D.reference(c.name)
    acc = {k: v for k, v in ref.items() if k in D.ACCUMULATED}
    m = D.judge(c, acc, second, init=2.5)
    for k, (s, a) in m.items():
        assert a <= D.TAU, f"{c.name} ({what}, from 2.5): {k} off by {a:.3g} of ref64 + 2.5"
    assert not D.passes(D.judge(c, acc, second)), f"{c.name} ({what}): the judge accepts overwritten accumulators"
    for k in acc:
        want = (first[k] + 2.5)                                            # float32: fl(first + 2.5)
        diff = float((second[k] - want).abs().max())
        if exact:
            assert torch.equal(second[k], want), f"{c.name} ({what}): {k} from 2.5 is not the first run + 2.5 exactly (off by {diff:.3g})"
        else:
            T = float(_term_sums(c.name)[k].max())
            one = EPS * (2.5 + float(np.abs(acc[k]).max()))
            print(f"{c.name} {what}: {k} from 2.5 differs from first + 2.5 by {diff / one:.2f} roundings of the sum ({grid} workgroups)")
            assert diff <= (2 * grid + 1) * EPS * (2.5 + T) * (1 + 1e-3), f"{c.name} ({what}): {k} from 2.5 is off the first run + 2.5 by {diff:.3g}"


# ------------------------------------------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in D.CASES if c.entry == "fwd"])
def test_forward(name):
    c, d = D.BY_NAME[name], D.build(name)
    L = _L()
    off = c.opts == "off"
    x, w, b = _dev(d["x"], off), _dev(d["w"], False), _dev(d["bias"], False)
    y = _guarded(c.R, c.O)
    L.check(L.lib().cm_linear_act_forward(c.R, c.K, c.O, _p(x), _p(w), c.layout, _p(b), c.act, _p(y), _st()), name)
    torch.cuda.synchronize()
    got = {"y": _written(name, "y", y, c.R).cpu()}
    m = _judge_and_controls(c, got, "forward")
    if c.opts.startswith("z"):
        err = float((got["y"].double() - torch.from_numpy(np.array(D.reference(name)["y"]))).abs().max())
        print(f"{name}: tanh_exact absolute error {err:.2e} (documented bound {D.TANH_ABS}), strict ratio {m['y'][0]:.2e}")
        assert err <= D.TANH_ABS


# ------------------------------------------------------------------------------------------------------------------------------
# backward
# ------------------------------------------------------------------------------------------------------------------------------
def _bwd_call(c, t, entry, init, slab=None, nb=0):
    """one call -> (rc, dict of outputs on the host); entry: '', '_ex', '_det', '_ex_det'"""
    lib = _L().lib()
    dx = _guarded(c.R, c.K) if c.dx else None
    dw = torch.full((c.O, c.K) if c.layout == 0 else (c.K, c.O), init, dtype=torch.float32, device=DEV)
    db = torch.full((c.O,), init, dtype=torch.float32, device=DEV) if c.bias else None
    head = (c.R, c.K, c.O, _p(t["x"]), _p(t["w"]), c.layout, _p(t["dy"]), _p(t["dy2"]), _p(t["y"]))
    if "_ex" in entry:
        head = head + (c.act,)
    else:
        assert c.act <= 1
    tail = (_p(dx), _p(dw), _p(db)) + ((_p(slab), nb) if "_det" in entry else ()) + (_st(),)
    rc = getattr(lib, "cm_linear_act_backward" + entry)(*head, *tail)
    torch.cuda.synchronize()
    out = {"dw": dw.cpu()}
    if c.bias:
        out["db"] = db.cpu()
    if c.dx:
        out["dx"] = dx
    return rc, out


def _bwd_case(name):
    c, d = D.BY_NAME[name], D.build(name)
    L = _L()
    lib = L.lib()
    off, offx = c.opts == "off", c.opts in ("off", "offx")
    t = dict(x=_dev(d["x"], offx), w=_dev(d["w"], False), dy=_dev(d["dy"], off), dy2=_dev(d["dy2"], off), y=_dev(d["y"], off))
    plain = "" if c.act <= 1 else "_ex"                                      # the entry without `act` names tanh by a non-NULL y
    chunks = (c.R + D.ROWS - 1) // D.ROWS
    grid = D.stream_grid(c.R) if c.route.split("/")[0] in ("stream", "ragged") else min(chunks, D.GRID_CAP)

    def take(rc, out, what):
        L.check(rc, f"{name} {what}")
        if c.dx:
            out["dx"] = _written(name, "dx", out["dx"], c.R).cpu()
        return out

    first = take(*_bwd_call(c, t, plain, 0.0), "atomic")
    _judge_and_controls(c, first, "atomic" + plain)
    second = take(*_bwd_call(c, t, "_ex", 2.5), "atomic from 2.5")
    _accumulates(c, "atomic", first, second, grid, exact=grid == 1)
    if c.dx:
        assert torch.equal(first["dx"], second["dx"]), f"{name}: dx differs between two runs"
    # slab twins
    nb = lib.cm_linear_act_backward_det_ws_bytes(c.R, c.K, c.O)
    d1 = take(*_bwd_call(c, t, "_ex_det", 0.0, _nan_slab(nb), nb), "_ex_det")
    _judge_and_controls(c, d1, "_ex_det")
    d2 = take(*_bwd_call(c, t, "_det" if c.act <= 1 else "_ex_det", 0.0, _nan_slab(nb), nb), "_det")
    for k in d1:
        assert torch.equal(d1[k], d2[k]), f"{name}: {k} of the slab twin is not bit-equal between two runs"
    d3 = take(*_bwd_call(c, t, "_ex_det", 2.5, _nan_slab(nb), nb), "_ex_det from 2.5")
    _accumulates(c, "det", d1, d3, grid, exact=True)


def _names(fam):
    return [c.name for c in D.CASES if D.group(c) == fam]


@pytest.mark.parametrize("name", _names("generic"))
def test_backward_generic(name):
    _bwd_case(name)


@pytest.mark.parametrize("name", _names("stream"))
def test_backward_stream(name):
    _bwd_case(name)


@pytest.mark.parametrize("name", _names("ragged"))
def test_backward_ragged(name):
    _bwd_case(name)


# ------------------------------------------------------------------------------------------------------------------------------
# weight gradient
# ------------------------------------------------------------------------------------------------------------------------------
def _wgrad_call(c, a, b, det, init, slab=None, nb=0):
    lib = _L().lib()
    cc = torch.full((c.K, c.O), init, dtype=torch.float32, device=DEV)
    cs = torch.full((c.K,), init, dtype=torch.float32, device=DEV) if c.bias else None
    if det:
        rc = lib.cm_linear_wgrad_det(c.R, c.K, c.O, _p(a), _p(b), _p(cc), _p(cs), _p(slab), nb, _st())
    else:
        rc = lib.cm_linear_wgrad(c.R, c.K, c.O, _p(a), _p(b), _p(cc), _p(cs), _st())
    torch.cuda.synchronize()
    _L().check(rc, c.name)
    out = {"c": cc.cpu()}
    if c.bias:
        out["colsum"] = cs.cpu()
    return out


@pytest.mark.parametrize("name", _names("wgrad"))
def test_wgrad(name):
    c, d = D.BY_NAME[name], D.build(name)
    lib = _L().lib()
    off = c.opts == "off"
    a, b = _dev(d["a"], off), _dev(d["b"], off)
    grid = min((c.R + D.ROWS - 1) // D.ROWS, D.GRID_CAP)
    first = _wgrad_call(c, a, b, False, 0.0)
    _judge_and_controls(c, first, "atomic")
    _accumulates(c, "atomic", first, _wgrad_call(c, a, b, False, 2.5), grid, exact=grid == 1)
    nb = lib.cm_linear_wgrad_det_ws_bytes(c.R, c.K, c.O)
    d1 = _wgrad_call(c, a, b, True, 0.0, _nan_slab(nb), nb)
    _judge_and_controls(c, d1, "_det")
    d2 = _wgrad_call(c, a, b, True, 0.0, _nan_slab(nb), nb)
    for k in d1:
        assert torch.equal(d1[k], d2[k]), f"{name}: {k} of the slab twin is not bit-equal between two runs"
    _accumulates(c, "det", d1, _wgrad_call(c, a, b, True, 2.5, _nan_slab(nb), nb), grid, exact=True)


# ------------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------------
def test_a_short_slab_is_refused_with_nothing_written():
    lib = _L().lib()
    R, K, O = 130, 40, 60
    z = lambda *s: torch.zeros(*s, device=DEV)                              # noqa: E731
    x, w, dy, y = z(R, K), z(O, K), z(R, O), z(R, O)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=DEV)   # noqa: E731
    nb = lib.cm_linear_act_backward_det_ws_bytes(R, K, O)
    assert nb == 3 * (K * O + O) * 4
    for entry in ("_det", "_ex_det"):
        dx, dw, db, slab = nan(R, K), nan(O, K), nan(O), _nan_slab(nb)
        head = (R, K, O, _p(x), _p(w), 0, _p(dy), None, _p(y)) + ((1,) if entry == "_ex_det" else ())
        rc = getattr(lib, "cm_linear_act_backward" + entry)(*head, _p(dx), _p(dw), _p(db), _p(slab), nb - 1, _st())
        torch.cuda.synchronize()
        assert rc == CM_ERR_ARG
        assert all(bool(torch.isnan(t).all()) for t in (dx, dw, db, slab)), entry
    nbw = lib.cm_linear_wgrad_det_ws_bytes(R, O, K)
    assert nbw == 3 * (K * O + O) * 4
    c, cs, slab = nan(O, K), nan(O), _nan_slab(nbw)
    assert lib.cm_linear_wgrad_det(R, O, K, _p(dy), _p(x), _p(c), _p(cs), _p(slab), nbw - 1, _st()) == CM_ERR_ARG
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (c, cs, slab))


def test_bad_arguments_are_refused():
    lib = _L().lib()
    R = 65
    z = lambda *s: torch.zeros(*s, device=DEV)                              # noqa: E731
    x, w, dy, y = z(R, 129), z(129, 129), z(R, 129), z(R, 129)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=DEV)   # noqa: E731
    out, dw, db = nan(R + GUARD, 129), nan(129, 129), nan(129)
    nb = 512 * (129 * 129 + 129) * 4
    slab = _nan_slab(nb)
    st = _st()
    bad = [(0, 64, 0), (64, 0, 0), (129, 64, 0), (64, 129, 0), (64, 64, 2), (64, 64, -1)]
    for K, O, lay in bad:
        assert lib.cm_linear_act_forward(R, K, O, _p(x), _p(w), lay, None, 1, _p(out), st) == CM_ERR_ARG, (K, O, lay)
        assert lib.cm_linear_act_backward(R, K, O, _p(x), _p(w), lay, _p(dy), None, _p(y), _p(out), _p(dw), _p(db), st) == CM_ERR_ARG
        assert lib.cm_linear_act_backward_ex(R, K, O, _p(x), _p(w), lay, _p(dy), None, _p(y), 1, _p(out), _p(dw), _p(db), st) == CM_ERR_ARG
        assert lib.cm_linear_act_backward_det(R, K, O, _p(x), _p(w), lay, _p(dy), None, _p(y), _p(out), _p(dw), _p(db), _p(slab), nb,
                                              st) == CM_ERR_ARG
        assert lib.cm_linear_act_backward_ex_det(R, K, O, _p(x), _p(w), lay, _p(dy), None, _p(y), 1, _p(out), _p(dw), _p(db), _p(slab),
                                                 nb, st) == CM_ERR_ARG
        if lay == 0:
            assert lib.cm_linear_wgrad(R, K, O, _p(x), _p(dy), _p(dw), _p(db), st) == CM_ERR_ARG
            assert lib.cm_linear_wgrad_det(R, K, O, _p(x), _p(dy), _p(dw), _p(db), _p(slab), nb, st) == CM_ERR_ARG
    # NULL dw / c
    assert lib.cm_linear_act_backward(R, 64, 64, _p(x), _p(w), 0, _p(dy), None, _p(y), _p(out), None, _p(db), st) == CM_ERR_ARG
    assert lib.cm_linear_act_backward_ex(R, 64, 64, _p(x), _p(w), 0, _p(dy), None, _p(y), 1, _p(out), None, _p(db), st) == CM_ERR_ARG
    assert lib.cm_linear_act_backward_det(R, 64, 64, _p(x), _p(w), 0, _p(dy), None, _p(y), _p(out), None, _p(db), _p(slab), nb,
                                          st) == CM_ERR_ARG
    assert lib.cm_linear_act_backward_ex_det(R, 64, 64, _p(x), _p(w), 0, _p(dy), None, _p(y), 1, _p(out), None, _p(db), _p(slab), nb,
                                             st) == CM_ERR_ARG
    assert lib.cm_linear_wgrad(R, 64, 64, _p(x), _p(dy), None, _p(db), st) == CM_ERR_ARG
    assert lib.cm_linear_wgrad_det(R, 64, 64, _p(x), _p(dy), None, _p(db), _p(slab), nb, st) == CM_ERR_ARG
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (out, dw, db, slab)), "a refused call wrote something"
