"""Fixed-length rollout segments (csrc/cm_segments.hip, CentralizedMAPPO(segment_steps=...)), the part that needs no GPU: the
declarations and bindings, the argument checks (which answer before anything is launched), the constructor's switch with its
environment fall-back and its refusal, the float64 reference against the textbook formulas, and the unit's register metadata."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests import segments_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("cm_segment_targets", "cm_adv_normalize_ws_bytes", "cm_adv_normalize", "cm_segment_episodes_ws_bytes", "cm_segment_episodes")


def test_symbols_are_exported_bound_and_declared():
    from com_marl_amd import _lib
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "commarl.h")).read()
    for n in SYMBOLS:
        assert n in _lib.EXPORTED and hasattr(lib, n), n
        assert re.search(r"\b" + n + r"\(", header), n
    assert not any(n.startswith(("cm_segment", "cm_adv_normalize")) and n.endswith("_det") for n in _lib.EXPORTED)   # no twin
    assert not set(SYMBOLS) & set(_lib.TWINS)
    assert lib.cm_abi_version() == 3 and "#define CM_ABI_VERSION 3" in header
    assert f"#define CM_SEG_COLS {_lib.SEG_COLS}" in header and _lib.SEG_COLS == 13
    for c, name in enumerate(_lib.SEG_COLUMNS[:8]):
        macro = {"count": "COUNT", "success": "SUCCESS"}.get(name, name.upper())
        assert f"#define CM_SEG_{macro} {c}\n" in header, name
    assert "#define CM_SEG_DETAILS 8\n" in header and _lib.SEG_COLUMNS[8:] == tuple(f"details_{k}" for k in range(5))
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert f'({len(_lib.EXPORTED)} `extern "C"` entry points)' in readme


def test_argument_errors_answer_before_any_launch():
    from com_marl_amd import _lib
    lib = _lib.lib()
    p = C.c_void_p(4096)                                             # plausible, never dereferenced

    def targets(T=5, rew=p, dones=p, base=p, vl=p, adv=p, ret=p):
        return lib.cm_segment_targets(3, T, rew, dones, 1, 3, base, vl, 0.99, 0.97, adv, ret, None)
    assert lib.cm_segment_targets(0, 0, None, None, 0, 0, None, None, 0.99, 0.97, None, None, None) == -1
    assert b"cm_segment_targets" in lib.cm_last_error() and b"null" in lib.cm_last_error()
    for kw in (dict(rew=None), dict(dones=None), dict(base=None), dict(vl=None), dict(adv=None), dict(ret=None)):
        assert targets(**kw) == -1 and b"null" in lib.cm_last_error(), kw
    for T in (0, -1):
        assert targets(T=T) == -1 and b"T >= 1" in lib.cm_last_error(), T

    need = lib.cm_adv_normalize_ws_bytes()
    assert need == 2 * 256 * 8
    assert lib.cm_adv_normalize(10, None, 1e-8, p, need, None) == -1 and b"null" in lib.cm_last_error()
    assert lib.cm_adv_normalize(10, p, 1e-8, None, need, None) == -1 and b"null workspace" in lib.cm_last_error()
    assert lib.cm_adv_normalize(10, p, 1e-8, p, need - 1, None) == -1 and b"required" in lib.cm_last_error()
    assert lib.cm_adv_normalize(-1, p, 1e-8, p, need, None) == -1
    assert lib.cm_adv_normalize(0, p, 1e-8, p, need, None) == 0                    # nothing to do, nothing launched

    assert lib.cm_segment_episodes_ws_bytes(1) == 16 * 8 and lib.cm_segment_episodes_ws_bytes(256) == 16 * 8
    assert lib.cm_segment_episodes_ws_bytes(257) == 2 * 16 * 8 and lib.cm_segment_episodes_ws_bytes(4096) == 16 * 16 * 8
    nb = lib.cm_segment_episodes_ws_bytes(300)

    def episodes(n=7, B=300, rew=p, table=p, ws=p, nb=nb):
        return lib.cm_segment_episodes(n, B, rew, p, p, p, 0.99, p, p, table, ws, nb, None)
    for kw, text in ((dict(n=0), b"n_steps"), (dict(B=0), b"B >= 1"), (dict(rew=None), b"null"), (dict(table=None), b"null"),
                     (dict(ws=None), b"null workspace"), (dict(nb=nb - 1), b"required")):
        assert episodes(**kw) == -1, kw
        assert text in lib.cm_last_error(), (kw, lib.cm_last_error())


def _cpu_algo(**kw):
    import torch
    from com_marl_amd import envs, nets
    from com_marl_amd.algos import CentralizedMAPPO
    N, d = 2, 6
    spec = envs.EnvSpec(envs._Box(np.zeros(d * N), np.ones(d * N)), envs._Discrete(5))
    torch.manual_seed(0)
    pol = nets.CommCategoricalMLPPolicy(spec, n_agents=N, device="cpu")
    crit = nets.CommBaseCritic(spec, n_agents=N, device="cpu")
    return CentralizedMAPPO(env_spec=spec, policy=pol, baseline=crit, **kw)


def test_switch_and_its_environment_fallback(monkeypatch):
    import pickle
    from com_marl_amd.algos import CentralizedMAPPO
    assert inspect.signature(CentralizedMAPPO.__init__).parameters["segment_steps"].default is None
    doc = CentralizedMAPPO.__init__.__doc__
    assert "COMMARL_SEGMENT_STEPS" in doc and "per-path normalisation" in doc          # what center_adv means here is documented
    monkeypatch.delenv("COMMARL_SEGMENT_STEPS", raising=False)
    assert _cpu_algo()._segment_steps is None
    assert _cpu_algo(segment_steps=32)._segment_steps == 32
    assert _cpu_algo(segment_steps=np.int64(1))._segment_steps == 1
    monkeypatch.setenv("COMMARL_SEGMENT_STEPS", "128")
    a = _cpu_algo()
    assert a._segment_steps == 128 and isinstance(a._segment_steps, int)
    assert _cpu_algo(segment_steps=7)._segment_steps == 7                               # explicit wins
    assert pickle.loads(pickle.dumps(a))._segment_steps == 128
    monkeypatch.setenv("COMMARL_SEGMENT_STEPS", "")
    assert _cpu_algo()._segment_steps is None


@pytest.mark.parametrize("bad", [0, -3, 2.5, 8.0, "x", "1.5", True, [8]])
def test_constructor_refuses_a_bad_segment_steps(bad, monkeypatch):
    from com_marl_amd.algos import CentralizedMAPPO
    monkeypatch.delenv("COMMARL_SEGMENT_STEPS", raising=False)
    with pytest.raises(ValueError, match="segment_steps"):
        CentralizedMAPPO(None, None, None, segment_steps=bad)        # (refused before anything else is looked at)
    if isinstance(bad, (int, float, str)) and not isinstance(bad, bool):
        monkeypatch.setenv("COMMARL_SEGMENT_STEPS", str(bad))
        with pytest.raises(ValueError, match="segment_steps"):
            CentralizedMAPPO(None, None, None)


def test_maximum_entropy_is_refused_with_its_reason(monkeypatch):
    monkeypatch.delenv("COMMARL_SEGMENT_STEPS", raising=False)
    kw = dict(entropy_method="max", center_adv=False, stop_entropy_gradient=True, policy_ent_coeff=0.01)
    assert _cpu_algo(**kw)._segment_steps is None                                       # the combination alone is fine
    with pytest.raises(NotImplementedError, match="cm_entropy_gae"):
        _cpu_algo(segment_steps=16, **kw)
    monkeypatch.setenv("COMMARL_SEGMENT_STEPS", "16")
    with pytest.raises(NotImplementedError, match="done-aware"):
        _cpu_algo(**kw)


def test_sampler_refusals_need_no_gpu():
    """n_steps, a PolicySet and the tape mode are refused before an engine exists."""
    from com_marl_amd import _lib as L, nets
    from com_marl_amd.sampler import CentralizedMAOnPolicyVectorizedSampler as S

    class _Cfg:
        rng_mode = L.RNG_PHILOX

    class _Batch:
        B, N, cfg = 4, 2, _Cfg()

    class _Env:
        batch = _Batch()

    class _Algo:
        policy, discount = object(), 0.99
    smp = S(_Algo(), _Env())
    for bad in (0, -1, 2.5, "x", None):
        with pytest.raises(ValueError, match="n_steps"):
            smp.obtain_segments(0, bad)
    _Algo.policy = nets.PolicySet.__new__(nets.PolicySet)                               # (never initialised: the type decides)
    with pytest.raises(ValueError, match="PolicySet"):
        smp.obtain_segments(0, 8)
    _Algo.policy = object()
    _Cfg.rng_mode = L.RNG_TAPE
    with pytest.raises(L.CommarlError, match="tape"):
        smp.obtain_segments(0, 8)
    assert smp.engine is None


# ---------------------------------------------------------------------------------------------------------------------------
# the float64 reference, piece by piece against the textbook formulas
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,T", [(70, 37), (1, 1), (3, 2)])
def test_reference_is_the_textbook_formulas_piece_by_piece(P, T):
    rng = np.random.default_rng(100 * P + T)
    gamma, lam = 0.99, 0.97
    r, v, vl = rng.normal(size=(P, T)), rng.normal(size=(P, T)), rng.normal(size=P) + 3.0
    d = R.draw_dones(P, T, rng)
    if P == 70:
        assert not d[0].any() and d[1].sum() == 1 and d[1, -1] and d[2, 0] and d[3, 1] and d[3, 2]
    adv, ret, terms = R.segment_targets(r, d, v, vl, gamma, gamma * lam, gamma)
    n_pieces = 0
    for p in range(P):
        ps = R.pieces(d[p])
        assert ps[0][0] == 0 and ps[-1][1] == T - 1 and all(a[1] + 1 == b[0] for a, b in zip(ps, ps[1:]))
        for first, last in ps:
            v_end = 0.0 if d[p, last] else vl[p]                        # a terminal state is worth nothing, the cut one v_last
            assert last == T - 1 or d[p, last]
            sl = slice(first, last + 1)
            np.testing.assert_allclose(adv[p, sl], R.textbook_gae(r[p, sl], v[p, sl], v_end, gamma, lam), rtol=1e-12, atol=1e-13)
            np.testing.assert_allclose(ret[p, sl], R.textbook_returns(r[p, sl], v_end, gamma), rtol=1e-12, atol=1e-13)
            n_pieces += 1
    assert n_pieces >= P and (terms >= np.abs(adv) - 1e-12).all()
    # a row that ends in a done does not see v_last at all
    adv2, ret2, _ = R.segment_targets(r, d, v, vl + 5.0, gamma, gamma * lam, gamma)
    ends = d[:, -1]
    assert np.array_equal(adv[ends], adv2[ends]) and np.array_equal(ret[ends], ret2[ends])
    if (~ends).any():
        assert not np.array_equal(adv[~ends], adv2[~ends])


def test_reference_coefficients_normalisation_and_episodes():
    g, gl, gr = R.kernel_coefficients(0.99, 0.97)
    assert g == float(np.float32(0.99)) and gr == 0.99 and gl == float(np.float32(np.float32(0.99) * np.float32(0.97)))
    x = np.random.default_rng(1).normal(2.0, 3.0, 500)
    y = R.adv_normalize(x, 1e-8)
    assert abs(y.mean()) < 1e-12 and abs(y.std() - 1.0) < 1e-8
    # episodes: two envs, 5 steps, cut into 2 + 3: the carry makes the halves add up to the whole
    rng = np.random.default_rng(2)
    rew, det = rng.normal(size=(5, 2)), rng.integers(0, 4, (5, 2, 6))
    done = np.zeros((5, 2), bool)
    done[2, 0] = done[4, 0] = done[3, 1] = True
    succ = rng.integers(0, 2, (5, 2))
    whole, _ = R.episodes(rew, done, det, succ, 0.9)
    a, carry = R.episodes(rew[:2], done[:2], det[:2], succ[:2], 0.9)
    b, _ = R.episodes(rew[2:], done[2:], det[2:], succ[2:], 0.9, carry)
    assert a == [] and len(b) == len(whole) == 3
    tw, tb = R.episode_table(whole), R.episode_table(b)
    assert tw.keys() == tb.keys() and all(abs(tw[k] - tb[k]) <= 1e-12 * max(1.0, abs(tw[k])) for k in tw)
    e0 = whole[0]
    assert e0["n"] == 3 and abs(e0["ret"] - rew[:3, 0].sum()) < 1e-12
    assert abs(e0["disc"] - (rew[0, 0] + 0.9 * rew[1, 0] + 0.81 * rew[2, 0])) < 1e-12
    assert (e0["det"] == det[:3, 0, :5].sum(0)).all() and e0["success"] == succ[2, 0]
    assert R.episode_table([])["count"] == 0 and R.episode_table([])["ret_min"] == np.inf


def test_kernels_of_the_unit_use_no_scratch_and_spill_nothing():
    from tests import isa
    ks = isa.kernels(isa.listing("cm_segments"))
    names = sorted(k.name for k in ks)
    assert len(ks) == 6, names
    for part in ("segment_targets_kernel", "adv_sum_kernel", "adv_sq_kernel", "adv_apply_kernel", "segment_episodes_kernel",
                 "segment_episodes_finish_kernel"):
        assert any(part in n for n in names), (part, names)
    for k in ks:
        assert k.private_segment_fixed_size == 0, (k.name, k.private_segment_fixed_size)
        assert k.vgpr_spill_count == 0, (k.name, k.vgpr_spill_count)
        assert not any(re.match(r"(global|flat)_atomic", ln) for ln in k.lines), k.name      # no atomics: one order of every sum
