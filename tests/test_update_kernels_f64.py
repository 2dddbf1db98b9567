"""The PPO update's loss, scan and optimiser kernels (com-marl_amd/csrc/cm_ppo.hip and cm_optim.hip), each called through
the C ABI with the arguments the update passes (algos.py _SurrogateFn / _advantages / process_samples, nets/layers.py _GaussNLLFn /
_flat_copy, optim.py Adam.step), against a float64 reference of the same operation (torch float64 on the GPU or numpy float64
on the host: it shares no code with the kernels):

  cm_ppo_surrogate / _det                       total, count, dlogits (NULL or set), padded steps, the CM_ENT_* bits
  cm_gauss_nll_forward / _det / _backward       loss, mean square, d_per_agent, d_log_std (NULL or set), *g NULL or 2.5
  cm_discount_returns, cm_gae                   bit-equal f64 recurrence; the scan and the per-path normalisation apart
  cm_multi_adam_step / _dev, cm_adam_bias_corrections    |g|^2, the clipped gradient, both moments, the step p_old - p_new
  cm_multi_copy_t                               exact, with NaN guard margins

The reference takes the kernel's own float32 inputs (hyper-parameters included) widened to float64, so it restates the
operation and not the rounding of an earlier stage.  Outputs a kernel writes start as NaN, as does the slab of each _det twin
and Adam's norm workspace (commarl.h: "no initial contents required"); cm_gauss_nll_forward's workspace starts at zero, as the
ABI requires, and must be zero again after every launch.

Metric: max|got - ref64| <= 1e-5 * max|ref64| per tensor (TAU), and - for dlogits per step, for the advantages per path -
each row against its own max|ref64|, floored at 1e-3 of the tensor's (tests/test_backward_kernels_f64.py _metric).  Every test
prints, per judged quantity, its worst STRICT ratio (that metric), its worst APPLIED one, and the strict ratio of plain float32
torch (numpy for the scans) evaluating the same formula.

Which branch or grid boundary each shape reaches (surrogate, gauss nll, returns, gae: cm_ppo.hip; adam, copy_t: cm_optim.hip):
  surrogate  256 steps per workgroup, one wave per 64 (ppo_surrogate_kernel, sized by ppo_surrogate): S = 1 (one lane), 255
             (ragged last wave), 256 (full workgroup), 257 (second workgroup of one lane), 3 x 200 and 13 x 300 ragged (the
             kernel's s -> (path, t) across workgroups; 16 block sums into its f64 atomic / the slab of its DET form).  A = 1:
             every probability on the upper clamp (both passes); logits of +-40: probabilities under the lower clamp; all-equal
             logits: the largest entropy, under CM_ENT_SOFTPLUS; r at, inside and outside 1 +- clip with both signs of adv and
             adv = 0 (the kernel's torch.min tie split and clamp window).
  gauss nll  forward grid capped at 256 workgroups (gauss_nll_forward): S = 65536 one pass, 65537 and 262145 loop
             (gauss_nll_fwd_kernel); backward capped at 1024 (cm_gauss_nll_backward): 262145 loops (gauss_nll_bwd_kernel);
             S = 1, 255, 257: lanes past S.  log_std above / at / below min_log_std and has_min = 0 (gauss_sigma, the backward
             kernel's d_log_std); g NULL; d_log_std NULL.
  returns, gae  64 paths per workgroup (cm_discount_returns, cm_gae): P = 63, 64, 65, 130 around the boundary (p >= P of
             returns_kernel, gae_kernel); T = 1, 2, 200; lens NULL; paths of length 1 and 2 (variance 0 in gae_kernel's
             normalisation).
  adam       64 x 256 threads (multi_adam): tensors of 16383 / 16384 / 16385 elements take one pass, one pass, two passes with a
             one-element tail; 50 000 takes four with a ragged tail (the grid-stride loops of multi_norm_kernel and
             multi_adam_kernel); clip active / inactive / norm_ws NULL; _dev: cursor -1, 0, 1, n - 1, n against a table of n rows
             (multi_adam_kernel clamps the cursor).
  copy_t     64 x 256 threads (cm_multi_copy_t): 200 x 131 in each mode takes two passes (both loops of multi_copy_t_kernel);
             [1, C], [R, 1], 128 x 128, 21 x 128, 128 x 21; n = 40 fills the table (CopyTable).

Where the APPLIED metric is wider than the STRICT one, and why.  Figures: measured on the MI355X, worst over the cases named;
"float32" is plain float32 torch (numpy for the scans) evaluating the same formula from the same inputs.
  * dlogits per step row, N >= 24 (SURR_TERMS_FROM_N): r = exp(new_ll - old_ll) is formed from two log-likelihoods of size
    N |log p| (up to 205 at N = 72) whose difference is O(1), so r - and with it the whole row of the gradient - carries the
    rounding of the TERMS of that difference.  Strict ratio of the kernel / of float32 torch: N = 24: 1.28e-5 / 5.65e-6
    (S = 255), 1.63e-5 / 1.02e-5 (3 x 200); N = 72: 7.93e-5 / 2.14e-5 (3 x 200), and float32 torch 1.30e-5 at S = 1.  The
    kernel adds the N float32 logs one after the other where torch adds them pairwise: summed that way on the host, the same
    float32 logs are off by 9.7e-5 in new_ll at N = 72 (torch's sum by 2.8e-5).  A row's scale is max|ref| times
    max(1, |new_ll| + |old_ll|), and the tensor's the largest of those; applied ratio then <= 2.4e-7.  For N <= 4 the strict
    metric holds as it is (<= 3.02e-6; float32 torch <= 2.40e-6).
  * a step whose float64 r lies within the float32 rounding of new_ll - old_ll of 1 - clip or 1 + clip (the steps built to
    land on the ends) may take either side of the clamp / min: its row is judged against the nearer of the two float64
    one-sided gradients.  The band is derived (_surr_band), not measured.
  * normalised advantages: a_t - mean cancels on a path whose advantages are nearly equal, and two steps are enough for that
    (P = 130, T = 2, gamma = lam = 1: strict 3.11e-5 for the kernel and 3.11e-5 for float32 numpy, which both subtract a
    float32 mean; all other cases <= 6.5e-6, <= 1.8e-7 at T = 200).  A row's scale is the larger of its max|ref| and
    (|a_t| + |mean|) / sqrt(var + eps), the tensor's the largest of those; applied ratio then <= 1.7e-7.
  * Adam's step p_old - p_new: 1e-5 max|step64| + 2^-23 |p_old| per element, the second term being the rounding of storing p in
    float32 (derived, not measured; judging p itself would hide an error the size of lr).  Against max|step64| alone the step
    misses by up to 3.7e-3 at lr = 3e-4 (2^-24 |p| / lr) and holds 4.8e-6 at lr = 0.1; against the allowance it reaches 0.49
    of it.
Everything else holds the strict metric: surrogate total <= 1.7e-6 (float32 torch 2.9e-6); gauss loss 2.1e-7, mean square
1.4e-7, d_per_agent 2.8e-7, d_log_std 6.7e-7 (float32 torch 4.6e-6), the 1e3-residual case against log_std = -3 included: the
float32 tail of the loss holds; the GAE scan <= 8.3e-7 per path, 3.9e-7 at T = 200 (float32 numpy 8.6e-7, 8.0e-7) - forming
delta in float32 does not break it; |g|^2 3.0e-7, the clipped gradient 1.9e-7, exp_avg 7.0e-7, exp_avg_sq 1.2e-7;
cm_discount_returns, the _dev twin, the bias-correction table and cm_multi_copy_t are bit-exact.

Negative controls: each group asserts that its APPLIED metric REJECTS plausible wrong answers computed from the float64
reference.  Two wrong answers one would want the surrogate's controls to include are not wrong: (a) "one renormalisation
instead of two in the gradient" - the Jacobian-transpose of p -> p / sum(p) at sum(p) = 1 is the projection
g -> g - <g, p>, which is idempotent and is annihilated by the softmax backward p (g - <g, p>) that follows, so any number
of renormalisations gives the same gradient;
(b) "the tie of torch.min split 1 / 0 instead of 1/2 / 1/2" - sur == clp happens inside the clip range, where both branches
carry the same gradient adv r, or at adv = 0, where both carry none.  The test computes both from the float64 reference and
asserts that they COINCIDE with it (so that nobody mistakes them for a check); the two that are observable - the clamp's ends
excluded, the last step dropped from the total - are asserted to fail.
"""
import ctypes as C
import math
import time

import numpy as np
import pytest
import torch

from tests.test_backward_kernels_f64 import _check, _metric, _reject

pytestmark = pytest.mark.gpu

TAU = 1e-5
DEV = "cuda:0"
F64 = torch.float64
F32 = torch.float32
EPS = float(np.finfo(np.float32).eps)
CM_ERR_ARG = -1


def _f(x):
    """A hyper-parameter as the kernel receives it: rounded to float32, widened."""
    return float(np.float32(x))


def _lib():
    from com_marl_amd import _lib as L
    return L


def _p(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=F32, device=DEV)


def _slab(nb):
    return torch.full((max(1, (int(nb) + 3) // 4),), float("nan"), dtype=F32, device=DEV)


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _note(worst, name, got, ref, **kw):
    """Strict ratio of a float32 comparator (not asserted)."""
    s = _metric(got, ref, **kw)[0]
    worst[name] = max(worst.get(name, 0.0), s)


@pytest.fixture
def tally(request):
    """(worst, f32) of a test: {name: (strict, applied)} filled by _check, {name: strict} of the float32 comparator filled by
    _note; printed when the test ends, passed or failed."""
    worst, f32, t0 = {}, {}, time.time()
    yield worst, f32
    _record(f"{request.node.name} ({time.time() - t0:.1f}s)", worst, f32)


def _record(case, worst, f32=None):
    """One line per test: every judged quantity's worst strict / applied ratio, and the float32 comparator's strict ratio."""
    if not worst:
        return
    f32 = f32 or {}
    parts = [f"{k} {s:.2e} / {a:.2e}" + (f" / {f32[k]:.2e}" if k in f32 else "") for k, (s, a) in worst.items()]
    print(f"{case}: strict / applied" + (" / float32 strict" if f32 else "") + ": " + "; ".join(parts))


# ------------------------------------------------------------------------------------------------------------------
# 1. cm_ppo_surrogate / cm_ppo_surrogate_det
# ------------------------------------------------------------------------------------------------------------------
CLIP = 0.1
# from this team size on, a row of dlogits is scaled by the size of the terms of new_ll - old_ll (module header): the smallest
# N at which the strict metric was measured to miss, for the kernel and for plain float32 torch alike
SURR_TERMS_FROM_N = 24


def _surr_objective(lg, actions, old_ll, adv, mask, lo, hi, c, flags, renorm_grads=2):
    """-(sum over valid steps of min(r adv, clamp(r) adv) + c f(H)) as tests/test_entropy_max.py spells it, in lg's dtype.
    renorm_grads < 2 detaches the sum of the later renormalisation(s) (a negative control)."""
    p = torch.softmax(lg, -1)
    s1 = p.sum(-1, keepdim=True)
    p = p / (s1 if renorm_grads >= 1 else s1.detach())
    s2 = p.sum(-1, keepdim=True)
    p = p / (s2 if renorm_grads >= 2 else s2.detach())
    logp = torch.log(p.clamp(EPS, 1 - EPS))
    H = -(p * logp).sum(-1).mean(-1)
    if flags & 4:
        H = H.detach()
    if flags & 2:
        H = torch.nn.functional.softplus(H)
    new_ll = logp.gather(-1, actions.long().unsqueeze(-1)).squeeze(-1).sum(-1)
    r = (new_ll - old_ll).exp()
    obj = torch.min(r * adv, r.clamp(lo, hi) * adv)
    if flags & 1:
        obj = obj + c * H
    return -(obj * mask).sum(), new_ll, r, obj


def _surr_band(N, new_ll, x):
    """Bound on |float32 (new_ll - old_ll) - float64 one| for float32 inputs: N logs, each of a probability that three
    divisions and an exp have rounded (<= 8 * 2^-24 absolute in the log) and with logf's own <= 2 ulp, summed in N float32
    additions of partial sums no larger than |new_ll|, one subtraction, and expf's <= 2 ulp carried back into the exponent."""
    return 2.0 ** -24 * (8 * N + (N + 2) * new_ll.abs() + 4 + x.abs())


def _surr_inputs(P, T, N, A, lens_kind, actions_kind, seed):
    g = torch.Generator().manual_seed(seed)
    S = P * T
    if lens_kind == "full":
        lens = torch.full((P,), T, dtype=torch.int32)
    else:
        lens = torch.randint(1, T + 1, (P,), generator=g).to(torch.int32)
        lens[0], lens[-1] = T, max(1, T - 3)
        if P > 2:
            lens[1] = 1
    logits = (torch.randn(S, N, A, generator=g) * 1.5).clamp(-5, 5)        # p >= e^-10 / 8: well inside the clamp
    s = torch.arange(S)
    hot = s % 7 == 0                                                        # +-40 on agent 0: probabilities under the clamp
    logits[hot, 0, 0] = 40.0
    if A > 1:
        logits[hot, 0, A - 1] = -40.0
    logits[s % 7 == 1] = 0.0                                                # all-equal logits: entropy log A, the largest
    if actions_kind == "last":
        actions = torch.full((S, N), A - 1, dtype=torch.int32)
    else:
        actions = torch.randint(0, A, (S, N), generator=g).to(torch.int32)
    adv = torch.randn(S, generator=g)
    adv[s % 5 == 3] = 0.0
    mask = (torch.arange(T)[None, :] < lens[:, None]).reshape(S)
    last = int(mask.nonzero()[-1])
    adv[last] = 1.5                                                         # the step the "last step dropped" control drops
    logits, actions, adv, lens, mask = (t.to(DEV) for t in (logits, actions, adv, lens, mask))
    # old_ll from the float32 new_ll (plain float32 torch), so that r lands on the ends, on 1, inside and outside
    lo, hi = _f(np.float32(1) - np.float32(CLIP)), _f(np.float32(1) + np.float32(CLIP))
    with torch.no_grad():
        _, new32, _, _ = _surr_objective(logits, actions, torch.zeros(S, device=DEV), adv, mask.float(), lo, hi, 0.0, 0)
    kind = (s % 8).to(DEV)
    noise = (torch.randn(S, generator=g) * 0.2).to(DEV)
    shift = torch.zeros(S, device=DEV)
    shift[kind == 0] = math.log(hi)
    shift[kind == 1] = math.log(lo)
    shift[kind == 3] = 0.03
    shift[kind == 4] = 0.5
    shift[kind == 5] = -0.5
    shift = torch.where(kind >= 6, noise, shift)
    old_ll = (new32 - shift).contiguous()
    return dict(logits=logits.contiguous(), actions=actions.contiguous(), old_ll=old_ll, adv=adv.contiguous(), lens=lens, mask=mask,
                lo=lo, hi=hi, last=last)


def _surr_call(P, T, N, A, c, inp, ent_coeff, flags, det, with_grad, slab=None):
    L = _lib()
    lib = L.lib()
    S = P * T
    total = torch.full((1,), float("nan"), dtype=F64, device=DEV)
    count = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    dl = _nan(S, N, A) if with_grad else None
    args = (P, T, N, A, _p(inp["logits"]), _p(inp["actions"]), _p(inp["old_ll"]), _p(inp["adv"]), _p(inp["lens"]), c, ent_coeff, flags,
            _p(total), _p(count), _p(dl))
    if det:
        nb = lib.cm_ppo_surrogate_det_ws_bytes(P, T)
        slab = _slab(nb)
        rc = lib.cm_ppo_surrogate_det(*args, _p(slab), nb, _st())
    else:
        rc = lib.cm_ppo_surrogate(*args, _st())
    L.check(rc, "cm_ppo_surrogate")
    torch.cuda.synchronize()
    return total, count, dl


SURR_CASES = [
    # P, T, N, A, add_entropy, lens, actions
    (1, 1, 4, 5, 1, "full", "random"),
    (1, 1, 72, 8, 7, "full", "random"),
    (1, 255, 1, 1, 1, "full", "random"),
    (1, 255, 24, 2, 5, "full", "random"),
    (1, 256, 3, 2, 3, "full", "random"),
    (1, 256, 4, 8, 0, "full", "last"),
    (1, 257, 4, 5, 5, "full", "random"),
    (1, 257, 4, 1, 7, "full", "random"),
    (3, 200, 24, 8, 7, "ragged", "random"),
    (3, 200, 72, 5, 1, "ragged", "random"),
    (3, 200, 4, 5, 3, "full", "last"),
    (3, 200, 1, 2, 0, "ragged", "random"),
    (13, 300, 4, 5, 3, "ragged", "random"),
    (13, 300, 3, 8, 1, "ragged", "last"),
]


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("P,T,N,A,flags,lens_kind,actions_kind", SURR_CASES,
                         ids=[f"P{c[0]}-T{c[1]}-N{c[2]}-A{c[3]}-e{c[4]}-{c[5]}-{c[6]}" for c in SURR_CASES])
def test_surrogate(P, T, N, A, flags, lens_kind, actions_kind, det, tally):
    S, ent_coeff = P * T, _f(0.3)
    case = f"surrogate P={P} T={T} N={N} A={A} ent={flags} {lens_kind} {actions_kind} {'det' if det else 'atomic'}"
    inp = _surr_inputs(P, T, N, A, lens_kind, actions_kind, seed=100 * S + 10 * N + A + flags)
    mask, lo, hi = inp["mask"], inp["lo"], inp["hi"]
    total, count, dl = _surr_call(P, T, N, A, _f(CLIP), inp, ent_coeff, flags, det, True)
    total0, count0, _ = _surr_call(P, T, N, A, _f(CLIP), inp, ent_coeff, flags, det, False)

    # float64 autograd of the objective, the weight w = d total / d new_ll of each step and G = d new_ll / d logits
    lg = inp["logits"].double().requires_grad_(True)
    adv64, old64, m64 = inp["adv"].double(), inp["old_ll"].double(), mask.double()
    want, new_ll, r, obj = _surr_objective(lg, inp["actions"], old64, adv64, m64, lo, hi, ent_coeff, flags)
    ref, w = torch.autograd.grad(want, (lg, new_ll), retain_graph=True)
    G, = torch.autograd.grad(new_ll.sum(), lg, retain_graph=True)
    want, new_ll, r, obj = want.detach(), new_ll.detach(), r.detach(), obj.detach()

    # steps within float32 rounding of an end of the clip range: either one-sided gradient (module header)
    x = new_ll - old64
    band = _surr_band(N, new_ll, x)
    at_hi, at_lo = (x - math.log(hi)).abs() <= band, (x - math.log(lo)).abs() <= band
    w_in = -m64 * adv64 * r                                                # inside the range, ends included: the gradient passes
    w_out = torch.where(at_hi, torch.where(adv64 > 0, torch.zeros_like(w_in), w_in),
                        torch.where(adv64 < 0, torch.zeros_like(w_in), w_in))
    at_end = at_hi | at_lo
    cand_in = torch.where(at_end[:, None, None], ref + (w_in - w)[:, None, None] * G, ref)
    cand_out = torch.where(at_end[:, None, None], ref + (w_out - w)[:, None, None] * G, ref)
    nearer_in = (dl.double() - cand_in).abs().amax((1, 2)) <= (dl.double() - cand_out).abs().amax((1, 2))
    ref_rows = torch.where(nearer_in[:, None, None], cand_in, cand_out)

    worst, f32 = tally
    kw = dict(rows=S)
    if N >= SURR_TERMS_FROM_N:
        terms = ref_rows.abs().amax((1, 2)) * (new_ll.abs() + old64.abs()).clamp(min=1.0)
        kw["row_terms"] = terms[:, None, None].expand_as(ref_rows)
        kw["tensor_terms"] = terms
    assert int(count) == int(mask.sum()) == int(count0), f"{case}: count {int(count)} != {int(mask.sum())}"
    _check(case, "total", total, want.reshape(1), worst)
    _check(case, "dlogits", dl, ref_rows, worst, **kw)
    assert bool((dl[~mask] == 0).all()), f"{case}: a padded step has a gradient"
    # dlogits NULL: the same total.  Block sums are the same numbers; the default adds them with f64 atomics in an order that is
    # free once there are more than two of them (a + b is commutative, a + b + c is not associative)
    blocks = (S + 255) // 256
    if det or blocks <= 2:
        assert torch.equal(total, total0), f"{case}: total changes with dlogits NULL ({float(total)!r} vs {float(total0)!r})"
    else:
        slack = blocks * 2.0 ** -52 * float((obj * m64).abs().sum())
        assert abs(float(total) - float(total0)) <= slack, f"{case}: total changes with dlogits NULL beyond the summation order"
    if det:
        total2, count2, dl2 = _surr_call(P, T, N, A, _f(CLIP), inp, ent_coeff, flags, True, True)
        assert torch.equal(total, total2) and torch.equal(dl, dl2) and int(count2) == int(count), f"{case}: the twin is not reproducible"

    # plain float32 torch of the same formula (the arithmetic a float32 implementation has)
    lg32 = inp["logits"].clone().requires_grad_(True)
    w32, _, _, _ = _surr_objective(lg32, inp["actions"], inp["old_ll"], inp["adv"], mask.float(), lo, hi, ent_coeff, flags)
    g32, = torch.autograd.grad(w32, lg32)
    n32 = (g32.double() - cand_in).abs().amax((1, 2)) <= (g32.double() - cand_out).abs().amax((1, 2))
    _note(f32, "total", w32.detach().reshape(1), want.reshape(1))
    _note(f32, "dlogits", g32, torch.where(n32[:, None, None], cand_in, cand_out), rows=S)

    # negative controls
    _reject(case, "the last step dropped from the total", [(total, (want + obj[inp["last"]]).reshape(1), {})])
    ends = at_end & mask & (adv64 != 0) & (G.abs().amax((1, 2)) > 0)
    if A > 1:
        assert bool(ends.any()), f"{case}: no step on an end of the clip range"
        w_excl = torch.where(ends, 0.5 * w_in, w)                           # tie sur == clp with the clamp's gradient cut at its ends
        _reject(case, "the clamp's ends excluded from the gradient", [(dl, ref + (w_excl - w)[:, None, None] * G, kw)])
    # the two wrong answers that are not wrong (module header): they coincide with the reference
    sur, clp = r * adv64, r.clamp(lo, hi) * adv64
    cg = ((r >= lo) & (r <= hi)).double()
    w_10 = -m64 * adv64 * r * ((sur <= clp).double() + cg * (sur > clp).double())
    assert _metric(ref + (w_10 - w)[:, None, None] * G, ref, rows=S)[0] <= 1e-12, f"{case}: the tie split is observable after all"
    want1, _, _, _ = _surr_objective(lg, inp["actions"], old64, adv64, m64, lo, hi, ent_coeff, flags, renorm_grads=1)
    ref1, = torch.autograd.grad(want1, lg)
    assert _metric(ref1, ref, rows=S)[0] <= 1e-9, f"{case}: the number of renormalisations in the gradient is observable after all"


def test_surrogate_empty_batch_and_short_slab():
    L = _lib()
    lib = L.lib()
    for det in (False, True):
        total = torch.full((1,), float("nan"), dtype=F64, device=DEV)
        count = torch.full((1,), -7, dtype=torch.int64, device=DEV)
        args = (0, 12, 4, 5, None, None, None, None, None, _f(CLIP), 0.0, 1, _p(total), _p(count), None)
        slab = _slab(0)                                                     # (a slab of no bytes is still a pointer: _lib.slab)
        rc = lib.cm_ppo_surrogate_det(*args, _p(slab), 0, _st()) if det else lib.cm_ppo_surrogate(*args, _st())
        L.check(rc, "cm_ppo_surrogate on an empty batch")
        torch.cuda.synchronize()
        assert float(total) == 0.0 and int(count) == 0
    P, T, N, A = 3, 200, 4, 5
    inp = _surr_inputs(P, T, N, A, "ragged", "random", seed=5)
    total = torch.full((1,), float("nan"), dtype=F64, device=DEV)
    count = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    nb = lib.cm_ppo_surrogate_det_ws_bytes(P, T)
    assert nb == 8 * ((P * T + 255) // 256)
    slab = _slab(nb)
    rc = lib.cm_ppo_surrogate_det(P, T, N, A, _p(inp["logits"]), _p(inp["actions"]), _p(inp["old_ll"]), _p(inp["adv"]), _p(inp["lens"]),
                                  _f(CLIP), 0.0, 1, _p(total), _p(count), None, _p(slab), nb - 1, _st())
    torch.cuda.synchronize()
    assert rc == CM_ERR_ARG
    assert bool(torch.isnan(total).all()) and int(count) == -7 and bool(torch.isnan(slab).all())      # refused before anything ran


# ------------------------------------------------------------------------------------------------------------------
# 2. cm_gauss_nll_forward / _det / _backward
# ------------------------------------------------------------------------------------------------------------------
def _gauss_ref(pa, ret, log_std, min_ls, has_min, g, dtype):
    """loss * g, mean square, d_per_agent, d_log_std of -Normal(sum_i per_agent, exp(clamp(log_std))).log_prob(returns).mean()."""
    pa_, ls_ = pa.detach().to(dtype).clone().requires_grad_(True), log_std.detach().to(dtype).clone().requires_grad_(True)
    v = pa_.sum(-1)
    ls = ls_.clamp(min=min_ls) if has_min else ls_
    loss = -torch.distributions.Normal(v, ls.exp(), validate_args=False).log_prob(ret.to(dtype)).mean()
    d_pa, d_ls = torch.autograd.grad(loss * g, (pa_, ls_), allow_unused=True)
    if d_ls is None:
        d_ls = torch.zeros_like(ls_)
    return loss.detach(), ((ret.to(dtype) - v.detach()) ** 2).mean(), d_pa, d_ls


def _gauss_call(S, N, pa, ret, log_std, min_ls, has_min, g_dev, want_dls, det):
    L = _lib()
    lib = L.lib()
    out = _nan(2)
    if det:
        nb = lib.cm_gauss_nll_forward_det_ws_bytes(S)
        rc = lib.cm_gauss_nll_forward_det(S, N, _p(pa), _p(ret), _p(log_std), min_ls, has_min, _p(out), _p(_slab(nb)), nb, _st())
        L.check(rc, "cm_gauss_nll_forward_det")
        torch.cuda.synchronize()
    else:
        ws = torch.zeros(2, dtype=F64, device=DEV)                           # CM_GAUSS_WS_BYTES, zero before the first use
        for launch in range(2):
            out.fill_(float("nan"))
            L.check(lib.cm_gauss_nll_forward(S, N, _p(pa), _p(ret), _p(log_std), min_ls, has_min, _p(out), _p(ws), _st()),
                    "cm_gauss_nll_forward")
            torch.cuda.synchronize()
            assert bool((ws.view(torch.int64) == 0).all()), f"the workspace is not zero after launch {launch + 1}"
    d_pa, d_ls = _nan(S, N), (_nan(1) if want_dls else None)
    L.check(lib.cm_gauss_nll_backward(S, N, _p(pa), _p(ret), _p(log_std), min_ls, has_min, _p(out), _p(g_dev), _p(d_pa), _p(d_ls), _st()),
            "cm_gauss_nll_backward")
    torch.cuda.synchronize()
    return out, d_pa, d_ls


MIN_LS = _f(-2.0)
GAUSS_SETTINGS = [
    # log_std, min_log_std, has_min, g, d_log_std wanted, residual scale, what
    (0.3, _f(math.log(1e-6)), 1, None, True, 1.0, "above the minimum, g NULL"),
    (MIN_LS, MIN_LS, 1, 2.5, True, 1.0, "exactly at the minimum: the gradient passes"),
    (-3.0, MIN_LS, 1, 2.5, True, 1.0, "below the minimum: no gradient"),
    (-0.7, 0.0, 0, None, False, 1.0, "has_min = 0, d_log_std NULL"),
    (-3.0, _f(math.log(1e-6)), 1, 2.5, True, 1e3, "returns - values of size 1e3 against log_std = -3"),
]
GAUSS_SHAPES = [(1, 1), (1, 4), (255, 24), (257, 4), (257, 1), (65536, 4), (65537, 4), (65537, 1), (262145, 4), (4099, 24)]


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("S,N", GAUSS_SHAPES, ids=[f"S{s}-N{n}" for s, n in GAUSS_SHAPES])
def test_gauss_nll(S, N, det, tally):
    worst, f32 = tally
    gen = torch.Generator().manual_seed(31 * S + N)
    pa = torch.randn(S, N, generator=gen).to(DEV)
    noise = torch.randn(S, generator=gen).to(DEV)
    for si, (ls, min_ls, has_min, g, want_dls, resid, what) in enumerate(GAUSS_SETTINGS):
        case = f"gauss S={S} N={N} {'det' if det else 'atomic'} [{what}]"
        ret = (pa.double().sum(-1) * 0.5 + noise.double() * 2.0 * resid).float().contiguous()
        log_std = torch.tensor([ls], dtype=F32, device=DEV)
        g_dev = None if g is None else torch.tensor([g], dtype=F32, device=DEV)
        gv = 1.0 if g is None else g
        out, d_pa, d_ls = _gauss_call(S, N, pa, ret, log_std, min_ls, has_min, g_dev, want_dls, det)
        loss, msq, r_pa, r_ls = _gauss_ref(pa, ret, log_std, min_ls, has_min, gv, F64)
        _check(case, "loss", out[0:1], loss.reshape(1), worst)
        _check(case, "mean square", out[1:2], msq.reshape(1), worst)
        _check(case, "d_per_agent", d_pa, r_pa, worst)
        if want_dls:
            _check(case, "d_log_std", d_ls, r_ls, worst)
            if has_min and ls < min_ls:
                assert float(d_ls) == 0.0, f"{case}: a gradient below the clamp"
        if det:
            out2, d_pa2, _ = _gauss_call(S, N, pa, ret, log_std, min_ls, has_min, g_dev, want_dls, True)
            assert torch.equal(out, out2) and torch.equal(d_pa, d_pa2), f"{case}: the twin is not reproducible"
        l32, m32, p32, s32 = _gauss_ref(pa, ret, log_std, min_ls, has_min, gv, F32)
        _note(f32, "loss", l32.reshape(1), loss.reshape(1))
        _note(f32, "mean square", m32.reshape(1), msq.reshape(1))
        _note(f32, "d_per_agent", p32, r_pa)
        _note(f32, "d_log_std", s32, r_ls)

        # negative controls, from the float64 reference
        d2 = (ret.double() - pa.double().sum(-1)) ** 2
        var = math.exp(2.0 * (max(_f(ls), min_ls) if has_min else _f(ls)))
        tail = math.log(math.exp(max(_f(ls), min_ls) if has_min else _f(ls))) + 0.5 * math.log(2 * math.pi)
        w_msq = d2[:-1].sum() / S
        w_pa = r_pa.clone()
        w_pa[-1] = 0
        _reject(case, "the last element of S dropped",
                [(out[1:2], w_msq.reshape(1), {}), (out[0:1], (w_msq / (2 * var) + tail).reshape(1), {}), (d_pa, w_pa, {})])
        if 1 < S and 1.0 / (S - 1) > 1.5 * TAU:             # (a mean over S - 1 is off by 1 / (S - 1) of itself: beyond that S, within TAU)
            w_msq = d2.sum() / (S - 1)
            _reject(case, "a mean over S - 1 elements", [(out[1:2], w_msq.reshape(1), {})])
        if want_dls and has_min and ls < min_ls:
            _reject(case, "a gradient that passes below the clamp", [(d_ls, (gv * (1 - msq / var)).reshape(1), {})])


def test_gauss_nll_refuses_a_short_slab():
    lib = _lib().lib()
    S, N = 700, 4
    pa, ret, ls, out = torch.zeros(S, N, device=DEV), torch.zeros(S, device=DEV), torch.zeros(1, device=DEV), _nan(2)
    nb = lib.cm_gauss_nll_forward_det_ws_bytes(S)
    assert nb == 8 * 3 and lib.cm_gauss_nll_forward_det_ws_bytes(262145) == 8 * 256
    rc = lib.cm_gauss_nll_forward_det(S, N, _p(pa), _p(ret), _p(ls), 0.0, 0, _p(out), _p(_slab(nb)), nb - 1, _st())
    torch.cuda.synchronize()
    assert rc == CM_ERR_ARG and bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------------------------------
# 3. cm_discount_returns and cm_gae
# ------------------------------------------------------------------------------------------------------------------
SCAN_P = [1, 63, 64, 65, 130]
SCAN_T = [1, 2, 200]
LENS_KINDS = ["ragged", "full", "null"]


def _scan_lens(P, T, kind, gen):
    """-> (int32 lens on the host as the reference sees them, the tensor passed to the kernel or None)."""
    if kind == "ragged":
        lens = torch.randint(1, T + 1, (P,), generator=gen).to(torch.int32)
        lens[0] = 1                                                          # a path of one step
        if P > 1:
            lens[1] = min(2, T)
        if P > 2:
            lens[2] = T
    else:
        lens = torch.full((P,), T, dtype=torch.int32)
    return lens.numpy(), (None if kind == "null" else lens.to(DEV))


def _returns_np(rew, lens, gamma):
    """tensor_utils.discount_cumsum per path in float64, cast once; zero past lens."""
    P, T = rew.shape
    y, out = np.zeros(P), np.zeros((P, T), np.float32)
    for t in range(T - 1, -1, -1):
        valid = t < lens
        y = np.where(valid, rew[:, t] + gamma * y, y)
        out[:, t] = np.where(valid, y, 0.0).astype(np.float32)
    return out


@pytest.mark.parametrize("lens_kind", LENS_KINDS)
@pytest.mark.parametrize("T", SCAN_T)
@pytest.mark.parametrize("P", SCAN_P)
def test_discount_returns_is_the_float64_recurrence_cast_once(P, T, lens_kind):
    L = _lib()
    gen = torch.Generator().manual_seed(1000 * P + T)
    lens, lens_dev = _scan_lens(P, T, lens_kind, gen)
    rew = torch.randn(P, T, generator=gen, dtype=F64)
    out = _nan(P, T)
    rew_dev = rew.to(DEV)
    L.check(L.lib().cm_discount_returns(P, T, _p(rew_dev), _p(lens_dev), 0.99, _p(out), _st()), "cm_discount_returns")
    torch.cuda.synchronize()
    want = _returns_np(rew.numpy(), lens, 0.99)
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), \
        f"returns P={P} T={T} {lens_kind}: {int((got != want).sum())} elements differ, worst {np.abs(got - want).max():.3g}"
    assert bool((got[np.arange(T)[None, :] >= lens[:, None]] == 0).all())


def _gae_np(rew, val, gamma, lam, dtype, v_at_t=False):
    """compute_advantages over the padded length (V past the end = 0) in `dtype`."""
    P, T = rew.shape
    r, v = rew.astype(dtype), val.astype(dtype)
    g, gl = dtype(gamma), dtype(gamma) * dtype(lam)
    acc, vnext, out = np.zeros(P, dtype), np.zeros(P, dtype), np.zeros((P, T), dtype)
    for t in range(T - 1, -1, -1):
        delta = r[:, t] + g * (v[:, t] if v_at_t else vnext) - v[:, t]
        acc = delta + gl * acc
        out[:, t] = acc
        vnext = v[:, t]
    return out


def _normalize_terms(a, lens, eps):
    """Size of the terms of (a_t - mean) / sqrt(var + eps): (|a_t| + |mean|) / sqrt(var + eps)."""
    a = a.astype(np.float64)
    out = np.zeros_like(a)
    for p in range(a.shape[0]):
        n = int(lens[p])
        m = a[p, :n].mean()
        out[p] = (np.abs(a[p]) + abs(m)) / np.sqrt(((a[p, :n] - m) ** 2).mean() + eps)
    return out


def _normalize_np(a, lens, eps, unbiased=False, over_T=False):
    """centralized_ma_ppo.py:422-426 per path in float64: mean / biased variance over the first lens[p] steps, applied to the row."""
    P, T = a.shape
    a = a.astype(np.float64)
    out = np.zeros_like(a)
    for p in range(P):
        n = T if over_T else int(lens[p])
        m = a[p, :n].mean()
        var = ((a[p, :n] - m) ** 2).sum() / ((n - 1) if unbiased else n)
        out[p] = (a[p] - m) / np.sqrt(var + eps)
    return out


@pytest.mark.parametrize("gamma,lam", [(0.99, 0.97), (1.0, 1.0)], ids=["g099-l097", "g1-l1"])
@pytest.mark.parametrize("T", SCAN_T)
@pytest.mark.parametrize("P", SCAN_P)
def test_gae(P, T, gamma, lam, tally):
    L = _lib()
    lib = L.lib()
    worst, f32 = tally
    g32, l32, eps = _f(gamma), _f(lam), _f(1e-8)
    for lens_kind in LENS_KINDS:
        case = f"gae P={P} T={T} gamma={gamma} lam={lam} lens {lens_kind}"
        gen = torch.Generator().manual_seed(77 * P + T + len(lens_kind))
        lens, lens_dev = _scan_lens(P, T, lens_kind, gen)
        valid = torch.arange(T)[None, :] < torch.as_tensor(lens)[:, None]
        rew = (torch.randn(P, T, generator=gen) * valid).contiguous()       # zero padding, as process_samples pads
        val = torch.randn(P, T, generator=gen).contiguous()
        rew_dev, val_dev = rew.to(DEV), val.to(DEV)
        a0, a1 = _nan(P, T), _nan(P, T)
        L.check(lib.cm_gae(P, T, _p(rew_dev), _p(val_dev), _p(lens_dev), g32, l32, 0, eps, _p(a0), _st()), "cm_gae")
        L.check(lib.cm_gae(P, T, _p(rew_dev), _p(val_dev), _p(lens_dev), g32, l32, 1, eps, _p(a1), _st()), "cm_gae")
        torch.cuda.synchronize()
        r_np, v_np = rew.numpy(), val.numpy()
        # the scan
        want0 = _gae_np(r_np, v_np, g32, l32, np.float64)
        kw = dict(rows=P)
        _check(case, "adv", a0, torch.as_tensor(want0), worst, **kw)
        _note(f32, "adv", torch.as_tensor(_gae_np(r_np, v_np, g32, l32, np.float32)), torch.as_tensor(want0), rows=P)
        wrong = _gae_np(r_np, v_np, g32, l32, np.float64, v_at_t=True)
        _reject(case, "V taken at t instead of at t + 1", [(a0, torch.as_tensor(wrong), kw)])
        # the normalisation, as an operation on the float32 advantages the kernel itself produced
        a0_np = a0.cpu().numpy()
        want1 = _normalize_np(a0_np, lens, eps)
        a1_np, one = a1.cpu().numpy(), lens == 1
        a32 = a0_np.copy()
        for p in range(P):                                                  # the same formula in float32 numpy
            n = int(lens[p])
            m = a32[p, :n].mean(dtype=np.float32)
            a32[p] = (a32[p] - m) / np.sqrt(((a32[p, :n] - m) ** 2).mean(dtype=np.float32) + np.float32(eps))
        if (~one).any():
            _note(f32, "normalised adv", torch.as_tensor(a32[~one]), torch.as_tensor(want1[~one]), rows=int((~one).sum()))
        # a_t - mean cancels on a path whose advantages are nearly equal (two steps are enough): the scales take the terms
        # (header).  Paths of one step apart: with variance 0 the rest of their row is (a - a_0) / sqrt(eps), 1e4 times the others
        nterms = torch.as_tensor(_normalize_terms(a0_np, lens, eps))
        for nm, sel in (("normalised adv", ~one), ("normalised adv, paths of one step", one)):
            if sel.any():
                _check(case, nm, torch.as_tensor(a1_np[sel]), torch.as_tensor(want1[sel]), worst, rows=int(sel.sum()),
                       row_terms=nterms[sel], tensor_terms=nterms[sel])
        if lens_kind == "ragged" or T == 1:
            assert one.any()
        assert bool((a1_np[one, 0] == 0).all()), f"{case}: a path of one step is not normalised to exactly 0"
        many = lens > 1
        if many.any():
            wrong = _normalize_np(a0_np[many], lens[many], eps, unbiased=True)
            _reject(case, "unbiased variance", [(torch.as_tensor(a1_np[many]), torch.as_tensor(wrong),
                                                 dict(rows=int(many.sum()), row_terms=nterms[many], tensor_terms=nterms[many]))])
        short = many & (lens < T)
        if short.any():
            wrong = _normalize_np(a0_np[short], lens[short], eps, over_T=True)
            _reject(case, "statistics over T instead of over lens",
                    [(torch.as_tensor(a1_np[short]), torch.as_tensor(wrong),
                      dict(rows=int(short.sum()), row_terms=nterms[short], tensor_terms=nterms[short]))])


# ------------------------------------------------------------------------------------------------------------------
# 4. cm_multi_adam_step, cm_multi_adam_step_dev, cm_adam_bias_corrections
# ------------------------------------------------------------------------------------------------------------------
B1, B2, ADAM_EPS = _f(0.9), _f(0.999), _f(1e-5)
ADAM_SETS = {
    "one": [1],
    "eight": [128 * 21, 128, 64 * 128, 64, 64 * 64, 5 * 32, 5, 1],          # test_hip_ppo_parity.py's set
    "forty": [16383, 16384, 16385, 50000] + [(37 * k * k + 11 * k) % 3001 + 1 for k in range(36)],
}
BIG = 3                                                                      # index of the 50 000-element tensor in "forty"


def _adam_ref(ps, gs, ms, vs, lr, step, max_norm, dtype=F64):
    """The formula of the Adam header comment of cm_optim.hip in `dtype` -> |g|^2, clipped gradients, exp_avg, exp_avg_sq, steps p_old - p_new."""
    gsq = sum((g.to(dtype) ** 2).sum() for g in gs)
    coef = 1.0
    if max_norm is not None:
        coef = min(1.0, max_norm / (float(gsq.sqrt()) + _f(1e-6)))
    bc1, bc2 = 1.0 - B1 ** step, 1.0 - B2 ** step
    gc, m2, v2, st = [], [], [], []
    for g, m, v in zip(gs, ms, vs):
        g_ = g.to(dtype) * coef
        m_ = m.to(dtype) * B1 + (1.0 - B1) * g_
        v_ = v.to(dtype) * B2 + (1.0 - B2) * g_ * g_
        gc.append(g_), m2.append(m_), v2.append(v_)
        st.append((lr / bc1) * m_ / (v_.sqrt() / math.sqrt(bc2) + ADAM_EPS))
    return gsq, gc, m2, v2, st


def _step_metric(p_old, p_new, step64):
    """-> (strict, applied) of the step p_old - p_new: strict against max|step64|; applied per element against
    1e-5 * max|step64| + 2^-23 |p_old| (the rounding of storing p in float32), scaled so that it compares with TAU."""
    err = ((p_old.double() - p_new.double()) - step64).abs()
    top = max(float(step64.abs().max()), 1e-30)
    allow = TAU * top + 2.0 ** -23 * p_old.double().abs()
    return float(err.max()) / top, TAU * float((err / allow).max())


def _reject_steps(case, what, p_old, p_new, wrong_steps):
    r = max(_step_metric(a, b, w)[1] for a, b, w in zip(p_old, p_new, wrong_steps))
    assert r > TAU, f"{case}: negative control '{what}' passes the step's allowance (ratio {r:.3g}): the check is too loose"


def _adam_call(ps, gs, ms, vs, lr, step, max_norm, norm_ws, dev=None):
    """dev = (table, cursor, rows): cm_multi_adam_step_dev."""
    L = _lib()
    lib = L.lib()
    n = len(ps)
    sizes = (C.c_int64 * n)(*[p.numel() for p in ps])
    head = (n, _ptrs(ps), _ptrs(gs), _ptrs(ms), _ptrs(vs), sizes, _p(norm_ws), 0.0 if max_norm is None else max_norm, lr, B1, B2, ADAM_EPS)
    if dev is None:
        rc = lib.cm_multi_adam_step(*head, step, _st())
    else:
        rc = lib.cm_multi_adam_step_dev(*head, _p(dev[0]), _p(dev[1]), dev[2], _st())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("lr", [3e-4, 0.1])
@pytest.mark.parametrize("clip", ["active", "inactive", "null"])
@pytest.mark.parametrize("which", list(ADAM_SETS))
def test_multi_adam_step(which, clip, lr, tally):
    L = _lib()
    sizes = ADAM_SETS[which]
    lr32 = _f(lr)
    max_norm = {"active": _f(0.5), "inactive": _f(1e9), "null": None}[clip]
    gen = torch.Generator().manual_seed(len(sizes) + int(lr * 1e4))
    ps = [torch.randn(s, generator=gen).to(DEV) for s in sizes]
    ms, vs = [torch.zeros(s, device=DEV) for s in sizes], [torch.zeros(s, device=DEV) for s in sizes]
    worst, f32 = tally
    for step in (1, 2, 3):                                                  # the kernel's own float32 state is carried forward
        case = f"adam {which} clip {clip} lr={lr} step {step}"
        g0 = [(torch.randn(s, generator=gen) * (0.1 + step)).to(DEV) for s in sizes]
        if which == "one":                                                  # (one element: keep |g| above max_norm, so that the clip acts)
            g0 = [g + 2 * torch.sign(g) for g in g0]
        gs = [g.clone() for g in g0]
        p_old, m_old, v_old = [p.clone() for p in ps], [m.clone() for m in ms], [v.clone() for v in vs]
        norm_ws = None if max_norm is None else _nan(65)                    # CM_ADAM_NORM_FLOATS, no initial contents required
        L.check(_adam_call(ps, gs, ms, vs, lr32, step, max_norm, norm_ws), "cm_multi_adam_step")
        gsq, gc, m2, v2, st = _adam_ref(p_old, g0, m_old, v_old, lr32, step, max_norm)
        _, gc32, m32, v32, st32 = _adam_ref(p_old, g0, m_old, v_old, lr32, step, max_norm, F32)
        if max_norm is None:
            assert all(torch.equal(a, b) for a, b in zip(gs, g0)), f"{case}: the gradient changed without a clip"
        else:
            _check(case, "|g|^2", norm_ws[0:1], gsq.reshape(1), worst)
            if clip == "active":
                assert float(gsq.sqrt()) > max_norm
        for k in range(len(sizes)):
            if max_norm is not None:
                _check(f"{case} tensor {k}", "clipped grad", gs[k], gc[k], worst)
            _check(f"{case} tensor {k}", "exp_avg", ms[k], m2[k], worst)
            _check(f"{case} tensor {k}", "exp_avg_sq", vs[k], v2[k], worst)
            strict, applied = _step_metric(p_old[k], ps[k], st[k])
            s0, a0 = worst.get("step", (0.0, 0.0))
            worst["step"] = (max(s0, strict), max(a0, applied))
            assert applied <= TAU, f"{case}: step of tensor {k} off by {applied / TAU:.3g} of its allowance (strict {strict:.3g})"
            _note(f32, "exp_avg", m32[k], m2[k])
            _note(f32, "exp_avg_sq", v32[k], v2[k])
            f32["step"] = max(f32.get("step", 0.0), float((st32[k].double() - st[k]).abs().max()) / max(float(st[k].abs().max()), 1e-30))
        # negative controls (the step metric, tensor by tensor: at least one must fail)
        _reject_steps(case, "the bias correction of step t + 1", p_old, ps, _adam_ref(p_old, g0, m_old, v_old, lr32, step + 1, max_norm)[4])
        if step > 1:
            _reject_steps(case, "the bias correction of step t - 1", p_old, ps,
                          _adam_ref(p_old, g0, m_old, v_old, lr32, step - 1, max_norm)[4])
        if clip == "active":
            noclip = _adam_ref(p_old, g0, m_old, v_old, lr32, step, None)
            _reject(case, "no clip", [(gs[k], noclip[1][k], {}) for k in range(len(sizes))] +
                    [(ms[k], noclip[2][k], {}) for k in range(len(sizes))])
        if which == "forty":
            w = [s.clone() for s in st]
            w[BIG][16384:] = 0
            _reject_steps(case, "the 50 000-element tensor left unchanged past 16384", p_old, ps, w)
            wm = m2[BIG].clone()
            wm[16384:] = m_old[BIG][16384:].double()
            _reject(case, "the 50 000-element tensor left unchanged past 16384", [(ms[BIG], wm, {})])


def test_multi_adam_refuses_41_tensors():
    ts = [torch.zeros(4, device=DEV) for _ in range(41)]
    assert _adam_call(ts, ts, ts, ts, _f(3e-4), 1, None, None) == CM_ERR_ARG
    tab, cur = torch.ones(2, 2, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    assert _adam_call(ts, ts, ts, ts, _f(3e-4), 0, None, None, dev=(tab, cur, 2)) == CM_ERR_ARG


def test_adam_bias_correction_table_and_device_cursor():
    """cm_adam_bias_corrections against float64 rounded once; cm_multi_adam_step_dev with cursor c bit-equal to the eager step
    first + c on copies of the same buffers (commarl.h: "the replayed steps are bit-identical to eager ones"), the cursor
    clamped to the table at both ends."""
    L = _lib()
    lib = L.lib()
    first, n = 7, 5
    host = torch.full((n, 2), float("nan"), dtype=F32)
    lib.cm_adam_bias_corrections(B1, B2, first, n, host.data_ptr())
    for i in range(n):
        t = first + i
        assert float(host[i, 0]) == float(np.float32(1.0 - B1 ** t)), f"1 - beta1^{t}"
        assert float(host[i, 1]) == float(np.float32(math.sqrt(1.0 - B2 ** t))), f"sqrt(1 - beta2^{t})"
    table = host.to(DEV)
    sizes = ADAM_SETS["eight"] + [50000]
    gen = torch.Generator().manual_seed(11)
    base = [[torch.randn(s, generator=gen).to(DEV) for s in sizes] for _ in range(3)]       # p, g, m
    base.append([torch.rand(s, generator=gen).to(DEV) * 0.1 for s in sizes])               # v >= 0
    lr32, max_norm = _f(3e-4), _f(0.5)
    for cursor, row in ((0, 0), (1, 1), (n - 1, n - 1), (-1, 0), (n, n - 1)):
        a = [[t.clone() for t in ts] for ts in base]
        b = [[t.clone() for t in ts] for ts in base]
        ws_a, ws_b = _nan(65), _nan(65)
        cur = torch.tensor([cursor], dtype=torch.int32, device=DEV)
        L.check(_adam_call(a[0], a[1], a[2], a[3], lr32, 0, max_norm, ws_a, dev=(table, cur, n)), "cm_multi_adam_step_dev")
        L.check(_adam_call(b[0], b[1], b[2], b[3], lr32, first + row, max_norm, ws_b), "cm_multi_adam_step")
        assert int(cur) == cursor                                           # the caller advances the cursor, not the kernel
        assert torch.equal(ws_a, ws_b), f"cursor {cursor}: norm workspace"
        for what, xa, xb in zip(("params", "grads", "exp_avg", "exp_avg_sq"), a, b):
            for k, (ta, tb) in enumerate(zip(xa, xb)):
                assert torch.equal(ta, tb), f"cursor {cursor}: {what}[{k}] differs from the eager step {first + row}"
        if row + 1 < n:                                                     # the neighbouring row's step is a different one
            c = [[t.clone() for t in ts] for ts in base]
            L.check(_adam_call(c[0], c[1], c[2], c[3], lr32, first + row + 1, max_norm, _nan(65)), "cm_multi_adam_step")
            assert not torch.equal(c[0][-1], a[0][-1])


# ------------------------------------------------------------------------------------------------------------------
# 5. cm_multi_copy_t
# ------------------------------------------------------------------------------------------------------------------
GUARD = 32


def _copy_call(srcs, dsts, rows, cols, tr):
    n = len(srcs)
    i32 = lambda xs: (C.c_int32 * len(xs))(*xs)                             # noqa: E731
    rc = _lib().lib().cm_multi_copy_t(n, _ptrs(srcs), (C.c_void_p * n)(*dsts), i32(rows), i32(cols), i32(tr), _st())
    torch.cuda.synchronize()
    return rc


def test_multi_copy_t_is_exact_and_stays_in_bounds():
    L = _lib()
    shapes = [(1, 77, 1), (1, 77, 0), (93, 1, 1), (93, 1, 0), (128, 128, 1), (128, 128, 0), (21, 128, 1), (128, 21, 1), (21, 128, 0),
              (200, 131, 1), (200, 131, 0), (131, 200, 1), (1, 1, 1), (1, 1, 0), (1, 16385, 0), (127, 129, 1)]
    k = 0
    while len(shapes) < 40:                                                 # fill the table: n = 40
        k += 1
        shapes.append(((7 * k) % 23 + 1, (11 * k) % 37 + 1, k % 2))
    gen = torch.Generator().manual_seed(5)
    srcs = [torch.randn(r, c, generator=gen).to(DEV) for r, c, _ in shapes]
    bufs = [_nan(r * c + 2 * GUARD) for r, c, _ in shapes]
    dsts = [b.data_ptr() + 4 * GUARD for b in bufs]
    L.check(_copy_call(srcs, dsts, [s[0] for s in shapes], [s[1] for s in shapes], [s[2] for s in shapes]), "cm_multi_copy_t")
    for (r, c, t), src, buf in zip(shapes, srcs, bufs):
        body = buf[GUARD:GUARD + r * c]
        want = src.t().contiguous().reshape(-1) if t else src.reshape(-1)
        assert torch.equal(body, want), f"[{r}, {c}] transpose={t}: {int((body != want).sum())} of {r * c} elements wrong"
        assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + r * c:]).all()), \
            f"[{r}, {c}] transpose={t}: wrote outside"


def test_multi_copy_t_refusals_and_no_op():
    lib = _lib().lib()
    src, dst = torch.ones(3, 4, device=DEV), _nan(12)
    assert _copy_call([src] * 41, [dst.data_ptr()] * 41, [3] * 41, [4] * 41, [0] * 41) == CM_ERR_ARG
    assert _copy_call([src, None], [dst.data_ptr()] * 2, [3, 3], [4, 4], [0, 0]) == CM_ERR_ARG
    assert _copy_call([src], [None], [3], [4], [1]) == CM_ERR_ARG
    assert _copy_call([src], [dst.data_ptr()], [0], [4], [0]) == CM_ERR_ARG
    assert lib.cm_multi_copy_t(0, None, None, None, None, None, _st()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(dst).all())                                     # nothing above wrote
