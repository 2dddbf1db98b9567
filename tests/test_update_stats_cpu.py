"""Per-step PPO update statistics and the KL early stop (csrc/cm_ppo_stats.hip, cm_multi_adam_step_gated), the part that needs
no GPU: declarations and bindings, the argument checks (which answer before anything is launched), the constructor's switches
and their environment fall-backs, and the new unit's register metadata."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("cm_ppo_update_stats_ws_bytes", "cm_ppo_update_stats", "cm_multi_adam_step_gated")


def test_symbols_are_exported_bound_and_declared():
    from com_marl_amd import _lib
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "commarl.h")).read()
    for n in SYMBOLS:
        assert n in _lib.EXPORTED and hasattr(lib, n), n
        assert re.search(r"\b" + n + r"\(", header), n
        assert not n.endswith("_det")
    assert lib.cm_abi_version() == 3 and "#define CM_ABI_VERSION 3" in header
    # the row's columns: the header's indices are _lib.UPD_COLUMNS' order
    assert f"#define CM_UPD_COLS {_lib.UPD_COLS}" in header and _lib.UPD_COLS == 8
    for c, name in enumerate(_lib.UPD_COLUMNS):
        assert f"#define CM_UPD_{name.upper()} {c}\n" in header, name
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert f'({len(_lib.EXPORTED)} `extern "C"` entry points)' in readme


def test_argument_errors_answer_before_any_launch():
    from com_marl_amd import _lib
    lib = _lib.lib()
    p = C.c_void_p(4096)                                             # plausible, never dereferenced
    need = lib.cm_ppo_update_stats_ws_bytes(10, 15)
    assert need == 7 * 8 and lib.cm_ppo_update_stats_ws_bytes(300, 250) == 7 * 8 * 256       # one f64 per plane and workgroup
    assert lib.cm_ppo_update_stats_ws_bytes(1 << 16, 1 << 10) == 7 * 8 * 256                 # at most 256 workgroups

    def call(A=5, N=4, rows=p, cursor=p, ws=p, nb=need, logits=p):
        return lib.cm_ppo_update_stats(10, 15, N, A, logits, p, p, p, 0.1, 0.0, rows, 256, cursor, None, ws, nb, None)
    for kw, text in ((dict(A=9), b"n_actions"), (dict(A=0), b"n_actions"), (dict(N=0), b"n_agents"), (dict(rows=None), b"null"),
                     (dict(cursor=None), b"null"), (dict(logits=None), b"null"), (dict(ws=None), b"null workspace"),
                     (dict(nb=need - 1), b"required")):
        assert call(**kw) == -1, kw
        assert text in lib.cm_last_error(), (kw, lib.cm_last_error())
    # the gated Adam: its gate is required
    n = 1
    arr = (C.c_void_p * n)(4096)
    sizes = (C.c_int64 * n)(16)
    assert lib.cm_multi_adam_step_gated(n, arr, arr, arr, arr, sizes, None, 0.0, 1e-3, 0.9, 0.999, 1e-8, p, p, 256, None, None) == -1
    assert b"null gate" in lib.cm_last_error()
    assert lib.cm_multi_adam_step_gated(n, arr, arr, arr, arr, sizes, None, 0.0, 1e-3, 0.9, 0.999, 1e-8, None, p, 256, p, None) == -1
    assert b"bias-correction table" in lib.cm_last_error()


@pytest.mark.parametrize("bad", [0, 0.0, -0.01, float("nan"), float("inf"), "x"])
def test_constructor_refuses_a_bad_target_kl(bad, monkeypatch):
    from com_marl_amd.algos import CentralizedMAPPO
    monkeypatch.delenv("COMMARL_TARGET_KL", raising=False)
    with pytest.raises(ValueError, match="target_kl"):
        CentralizedMAPPO(None, None, None, target_kl=bad)            # (refused before anything else is looked at)
    monkeypatch.setenv("COMMARL_TARGET_KL", str(bad))
    with pytest.raises(ValueError, match="target_kl"):
        CentralizedMAPPO(None, None, None)


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


def test_switches_and_their_environment_fallbacks(monkeypatch):
    import inspect
    import pickle
    from com_marl_amd.algos import CentralizedMAPPO
    sig = inspect.signature(CentralizedMAPPO.__init__).parameters
    assert sig["update_stats"].default is None and sig["target_kl"].default is None
    assert "1.5" in CentralizedMAPPO.__init__.__doc__                  # the stop factor is documented
    monkeypatch.delenv("COMMARL_UPDATE_STATS", raising=False)
    monkeypatch.delenv("COMMARL_TARGET_KL", raising=False)
    a = _cpu_algo()
    assert a._update_stats is False and a._target_kl is None and a.update_rows is None
    a = _cpu_algo(update_stats=True)
    assert a._update_stats is True and a._target_kl is None
    a = _cpu_algo(update_stats=False, target_kl=0.02)                  # target_kl implies update_stats
    assert a._update_stats is True and a._target_kl == 0.02
    monkeypatch.setenv("COMMARL_UPDATE_STATS", "1")
    a = _cpu_algo()
    assert a._update_stats is True and a._target_kl is None
    assert _cpu_algo(update_stats=False)._update_stats is False        # explicit wins
    monkeypatch.setenv("COMMARL_UPDATE_STATS", "0")
    monkeypatch.setenv("COMMARL_TARGET_KL", "0.015")
    a = _cpu_algo()
    assert a._update_stats is True and math.isclose(a._target_kl, 0.015)
    assert _cpu_algo(target_kl=0.5)._target_kl == 0.5
    # the device tables are no part of a snapshot
    a._upd_state = object()
    st = a.__getstate__()
    assert "_upd_state" not in st and st["_target_kl"] == a._target_kl
    del a._upd_state
    b = pickle.loads(pickle.dumps(a))
    assert b._update_stats is True and b._target_kl == a._target_kl


def test_adam_device_step_session_bookkeeping():
    """optim.Adam's device-step session on CPU parameters (arming and booking are host work: no launch, and
    cm_adam_bias_corrections is host code): a never-stepped optimiser behind a gate, an ungated session after it, the refusals."""
    import torch
    from com_marl_amd.optim import Adam
    cap = Adam.DEV_STEP_CAPACITY
    ps = [torch.nn.Parameter(torch.randn(3, 2)), torch.nn.Parameter(torch.randn(5))]
    opt = Adam(ps, lr=1e-3, betas=(0.9, 0.999))
    for bad in (0, cap + 1):
        with pytest.raises(AssertionError):
            opt.begin_device_steps(bad)
    with pytest.raises(AssertionError):
        opt.begin_device_steps(5, gate=torch.zeros(1, dtype=torch.int64))
    assert opt._dev_steps is None and not any(opt.state[p] for p in ps)             # a refusal arms nothing

    def table(first, n):
        """Rows first .. first + n - 1 in float64, rounded once to float32 (the betas cross the C ABI as floats)."""
        b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
        want = np.zeros((cap, 2), np.float32)
        for i in range(n):
            want[i] = 1.0 - b1 ** (first + i), math.sqrt(1.0 - b2 ** (first + i))
        return want

    # never stepped, behind a gate: zero moments, the first step number is 1
    versions = [p._version for p in ps]
    opt.begin_device_steps(5, gate=torch.zeros(1, dtype=torch.int32))
    ds = opt._dev_steps
    for p in ps:
        st = opt.state[p]
        assert st["step"] == 0 and st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape
        assert not st["exp_avg"].any() and not st["exp_avg_sq"].any()
    assert ds["table"].dtype == torch.float32 and ds["table"].numpy().tobytes() == table(1, 5).tobytes()
    assert int(ds["cursor"].item()) == 0
    opt.end_device_steps(3)
    assert opt._dev_steps is None
    assert [int(opt.state[p]["step"]) for p in ps] == [3, 3]
    assert all(p._version > v for p, v in zip(ps, versions))

    # ungated, after a session: the table starts at step 4, in the same table and cursor tensors
    opt.begin_device_steps(2)
    ds2 = opt._dev_steps
    assert ds2.get("gate") is None
    assert ds2["table"].data_ptr() == ds["table"].data_ptr() and ds2["cursor"].data_ptr() == ds["cursor"].data_ptr()
    assert ds2["table"].numpy().tobytes() == table(4, 2).tobytes() and int(ds2["cursor"].item()) == 0
    opt.end_device_steps(2)
    assert opt._dev_steps is None and [int(opt.state[p]["step"]) for p in ps] == [5, 5]


def test_kernels_of_the_unit_use_no_scratch_and_spill_nothing():
    from tests import isa
    ks = isa.kernels(isa.listing("cm_ppo_stats"))
    names = sorted(k.name for k in ks)
    assert len(ks) == 2 and any("ppo_update_stats_kernel" in n for n in names) and any("finish_kernel" in n for n in names), names
    for k in ks:
        assert k.private_segment_fixed_size == 0, (k.name, k.private_segment_fixed_size)
        assert k.vgpr_spill_count == 0, (k.name, k.vgpr_spill_count)
