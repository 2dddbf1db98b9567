"""Per-env comm conditions on the env step (cm_env_set_conditions, csrc/cm_env_cond.hip), driven through cm_env_step alone by one
random action tensor per case: every slice of a conditions batch must write exactly what the uniform-condition kernels write for
a batch built with that condition (tests/conditions_common.py) - no exclusions, no tolerance."""
import ctypes as C

import numpy as np
import pytest

from tests import conditions_common as cc

pytestmark = pytest.mark.gpu

PP4 = ("pp", cc.base_params("pp", 10, 1, 4, 4))
PP4_CONDS = [dict(Rcom=9, pl=0), dict(Rcom=2, pl=0.3), dict(Rcom=1, pl=0.9), dict(Rcom=3, pl=0)]
CO24 = cc.base_params("co", 20, 2, 24, 0)
PP72 = ("pp", cc.base_params("pp", 30, 2, 72, 72))
PP9 = ("pp", cc.base_params("pp", 10, 1, 9, 4))
PP9_CONDS = [dict(Rcom=9, pl=0.1), dict(Rcom=2, pl=0.3), dict(Rcom=1, pl=0.9), dict(Rcom=4, pl=0.5)]

# (scenario, params), channel kind, conditions, E, paired ids, steps, max_steps
CASES = {
    "pp4_iid": (PP4, "IID", PP4_CONDS, 5, False, 12, 5),
    "pp4_iid_paired": (PP4, "IID", PP4_CONDS, 5, True, 12, 5),
    "co24_ge_random_init": (("co", dict(CO24, GE_INIT=2)), "GE",
                            [dict(Rcom=3, Pgb=0.05, Pbg=0.3), dict(Rcom=6, Pgb=0.4, Pbg=0.1), dict(Rcom=19, Pgb=0.9, Pbg=0.9)],
                            3, False, 12, 5),
    "co24_ge_per_step": (("co", dict(CO24, loss_apply=0)), "GE", [dict(Pgb=0.05, Pbg=0.3), dict(Pgb=0.6, Pbg=0.1)], 2, False, 12, 5),
    "pp72_iid": (PP72, "IID", [dict(Rcom=5, pl=0.3), dict(Rcom=29, pl=0.6)], 2, False, 12, 5),
    "pp9_narrow64": (PP9, "IID", PP9_CONDS, 385, False, 4, 2),
    "pp9_lanes32": (PP9, "IID", PP9_CONDS, 2048, False, 3, 2),
}


def _run_case(name):
    (scen, params), channel, conds, E, paired, T, max_steps = CASES[name]
    Cn = len(conds)
    B, off = Cn * E, 11
    kw = dict(rng_ids=off + np.arange(B) % E) if paired else {}
    env = cc.make_batch(scen, params, B, off, channel, max_steps, conditions=conds, **kw)
    assert env.conditions == conds and not env.adj_const and env.channelType == channel
    np.testing.assert_array_equal(env.condition_of, np.repeat(np.arange(Cn), E))
    acts = cc.random_actions(T, B, env.N, seed=len(name))
    got = cc.drive(env, acts)
    return env, conds, E, off, paired, acts, got, (scen, params, channel, max_steps)


@pytest.mark.parametrize("name", list(CASES))
def test_slices_equal_uniform_batches(name):
    env, conds, E, off, paired, acts, got, (scen, params, channel, max_steps) = _run_case(name)
    B, N = env.B, env.N
    # ---- the inputs bite ----
    done = np.stack([s["done"] for s in got[1:]])
    assert done.any(0).all(), "every env must auto-reset at least once"
    deg = np.stack([s["dist_adj"] for s in got]).sum(-1).mean((0, 2)).reshape(len(conds), E).mean(1)     # mean degree per condition
    full = [c.get("Rcom", params["teRcom"]) + 1 >= params["grid_size"] for c in conds]
    for c, d in enumerate(deg):
        if full[c]:
            assert d == N
    rc = [N * 100 if full[c] else conds[c].get("Rcom", params["teRcom"]) for c in range(len(conds))]
    for a in range(len(conds)):
        for b in range(a + 1, len(conds)):
            if rc[a] != rc[b]:
                assert deg[a] != deg[b], (deg, rc)
    ch = np.stack([s["channels"] for s in got])                                     # [T+1, B, L, N, N]
    for c, cond in enumerate(conds):
        if cond.get("pl") == 0.9:
            # the issue asks for a channel mean below 0.3; the diagonal is always delivered and alone is 1/N of the mean (0.25
            # at N = 4), so the bound is put on the links that can be lost, whose expected mean is 0.1
            m = cc.offdiag_mean(ch[:, c * E:(c + 1) * E])
            print(f"{name}: pl 0.9 slice, off-diagonal channel mean {m:.4f}")
            assert m < 0.3
    # ---- every slice against its uniform batch ----
    refs = {}
    for lo, hi, c, first_id in cc.slices_of(env.condition_of, env.rng_ids):
        assert (hi - lo, first_id) == (E, off if paired else off + lo)
        w = cc.uniform_batch(scen, params, conds[c], hi - lo, first_id, channel, max_steps)
        assert w.channelType == channel and w.ch_const == env.ch_const
        assert w.adj_const == full[c]
        ref = cc.drive(w, acts[:, lo:hi])
        cc.assert_slice_equal(got, lo, hi, ref, f"{name}: condition {c}")
        if w.adj_const:
            assert all((s["dist_adj"][lo:hi] == 1).all() for s in got)
        refs[c] = (lo, hi, ref)
    # ---- control: a slice is NOT what another condition's uniform batch writes ----
    lo, hi, _ = refs[0]
    w = cc.uniform_batch(scen, params, conds[1], E, off + lo, channel, max_steps)      # slice 0's ids and actions, condition 1
    assert cc.slices_differ(got, lo, hi, cc.drive(w, acts[:, lo:hi]))


def test_dispatch_reaches_every_kernel_form():
    """The shapes above land where the table says: 16 lanes per env, the wide form, 64 lanes narrow, 32 lanes - by the rule
    of cm_env_create / launch() (largest team <= 8: 16 lanes; <= 32 agents and >= 8192 envs: 32; else 64; wide when 64 lanes and at
    most 1536 envs)."""
    def lanes(big, B):
        return 16 if big <= 8 else (32 if big <= 32 and B >= 8192 else 64)
    shape = {n: (max(c[0][1]["n_agents"], c[0][1]["n_preys"] if c[0][0] == "pp" else 0), len(c[2]) * c[3]) for n, c in CASES.items()}
    assert lanes(*shape["pp4_iid"]) == 16 and shape["pp4_iid"][1] == 20      # E = 5: condition borders inside a wave, ragged last one
    for n in ("co24_ge_random_init", "co24_ge_per_step", "pp72_iid"):
        assert lanes(*shape[n]) == 64 and shape[n][1] <= 1536
    assert lanes(*shape["pp9_narrow64"]) == 64 and shape["pp9_narrow64"][1] == 1540 > 1536
    assert lanes(*shape["pp9_lanes32"]) == 32 and shape["pp9_lanes32"][1] == 8192


def _pp4(conds, B=8, off=11, **kw):
    scen, params = PP4
    return cc.make_batch(scen, params, B, off, "IID", conditions=conds, **kw)


def test_set_conditions_changes_the_next_step_and_nothing_else():
    X, Y = PP4_CONDS[:2], PP4_CONDS[2:]
    acts = cc.random_actions(3, 8, 4, seed=7)
    a = _pp4(X)
    before = cc.drive(a, acts[:1])[-1]
    a.set_conditions(Y)
    assert a.conditions == Y
    after = cc.snapshot(a)
    for name, v in before.items():
        if name != "path_len":
            np.testing.assert_array_equal(after[name], v, err_msg=name)      # no state, no output touched by the call itself
    a.step_device(acts[1])
    a.check_status()
    got = cc.snapshot(a)
    # reference: a batch under Y from the start, put into a's state before the step
    r = _pp4(Y)
    r.reset_all()
    r.set_state(**{k[len("state."):]: v for k, v in before.items() if k.startswith("state.")})
    r.step_device(acts[1])
    r.check_status()
    want = cc.snapshot(r)
    for name in want:
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)
    # control: without the call the step writes something else
    k = _pp4(X)
    kept = cc.drive(k, acts[:2])[-1]
    assert any(not np.array_equal(kept[n], got[n]) for n in want)
    # condition_of / rng_ids can be replaced too; None keeps them
    a.set_conditions(Y, condition_of=np.array([1, 0] * 4))
    np.testing.assert_array_equal(a.condition_of, [1, 0] * 4)
    np.testing.assert_array_equal(a.rng_ids, 11 + np.arange(8))


def test_captured_graph_replays_with_the_new_values():
    import torch
    from com_marl_amd import _lib as L
    X, Y = PP4_CONDS[:2], PP4_CONDS[2:]
    acts = cc.random_actions(3, 8, 4, seed=9)
    g_env, e_env = _pp4(X), _pp4(X)
    for env in (g_env, e_env):                                               # the scratch step outside the capture
        env.reset_all()
        env.step_device(acts[0])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with L.capture_guard():
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            g_env.step_device(acts[1])
            g_env.step_device(acts[2])
    snaps = []
    for conds in (None, Y):
        if conds is not None:
            g_env.set_conditions(conds)
            e_env.set_conditions(conds)
        g.replay()
        e_env.step_device(acts[1])
        e_env.step_device(acts[2])
        g_env.check_status()
        e_env.check_status()
        got, want = cc.snapshot(g_env), cc.snapshot(e_env)
        for name in want:
            np.testing.assert_array_equal(got[name], want[name], err_msg=f"{name} (conditions {conds})")
        snaps.append(got)
    # the second replay did run under Y: an eager twin that stays under X ends elsewhere
    k = _pp4(X)
    k.reset_all()
    for a in (acts[0], acts[1], acts[2], acts[1], acts[2]):
        k.step_device(a)
    k.check_status()
    kept = cc.snapshot(k)
    assert any(not np.array_equal(kept[n], snaps[1][n]) for n in kept)


def test_refusals():
    from com_marl_amd import _lib as L, envs as E
    scen, params = PP4
    lib = L.lib()
    with pytest.raises(L.CommarlError, match="tape"):
        E.GridEnvBatch(scen, params, 4, device="cuda:0", seed=3, channel="IID", rng_mode="tape", conditions=PP4_CONDS[:2])
    # the first table comes too late after a reset
    u = cc.make_batch(scen, params, 4, 0, "IID")
    assert lib.cm_env_has_conditions(u._h) == 0
    table = E.condition_table(scen, params, PP4_CONDS[:2], np.array([0, 0, 1, 1]), channel="IID")
    u.reset_all()
    assert lib.cm_env_set_conditions(u._h, table.ctypes.data, None) == -1
    assert b"before the handle's first reset" in lib.cm_last_error()
    assert lib.cm_env_has_conditions(u._h) == 0 and lib.cm_env_adj_is_const(u._h) == 0    # (Rcom 3 on map 10: a range graph anyway)
    with pytest.raises(L.CommarlError, match="without conditions"):
        u.set_conditions(PP4_CONDS[:2])
    # a fully connected handle: the first table turns adj_const off
    f = cc.make_batch(scen, dict(params, teRcom=9), 4, 0, "IID")
    assert lib.cm_env_adj_is_const(f._h) == 1 and lib.cm_env_channels_are_const(f._h) == 0
    assert lib.cm_env_set_conditions(f._h, None, None) == -1 and b"null table" in lib.cm_last_error()
    for field, value, text in (("ploss", 1.5, b"ploss"), ("ploss", -0.25, b"ploss"), ("ploss", float("nan"), b"ploss"),
                               ("rcom", -1, b"rcom"), ("reserved", (0, 1, 0), b"reserved")):
        bad = table.copy()
        bad[field][2] = value
        assert lib.cm_env_set_conditions(f._h, bad.ctypes.data, None) == -1, field
        assert text in lib.cm_last_error() and b"env 2" in lib.cm_last_error()
        assert lib.cm_env_has_conditions(f._h) == 0 and lib.cm_env_adj_is_const(f._h) == 1
    assert lib.cm_env_set_conditions(f._h, table.ctypes.data, None) == 0
    assert lib.cm_env_has_conditions(f._h) == 1
    assert lib.cm_env_adj_is_const(f._h) == 0 and lib.cm_env_channels_are_const(f._h) == 0
    # probabilities the channel kind does not read are ignored; an FC handle keeps its constant channel
    fc = cc.make_batch(scen, params, 4, 0, None)
    assert fc.channelType == "FC"
    odd = table.copy()
    odd["ploss"] = 7.0
    assert lib.cm_env_set_conditions(fc._h, odd.ctypes.data, None) == 0
    assert lib.cm_env_channels_are_const(fc._h) == 1
    # python side
    with pytest.raises(ValueError, match="evenly"):
        cc.make_batch(scen, params, 5, 0, "IID", conditions=PP4_CONDS[:2])
    with pytest.raises(ValueError, match="entries"):
        cc.make_batch(scen, params, 4, 0, "IID", conditions=PP4_CONDS[:2], condition_of=np.array([0, 1]))


def test_fused_entry_points_decline():
    """cm_rollout_step / cm_rollout_chunk answer 1 - nothing done - for a handle with a table, at the shape where they run the
    fused kernels for a uniform handle; the engine then stays on two launches per step and never asks again."""
    import torch
    from com_marl_amd import envs as E, nets
    from com_marl_amd.rollout import RolloutEngine
    scen, params = PP4
    H = 4
    made = []
    for conds in (None, PP4_CONDS[:2]):
        env = cc.make_batch(scen, dict(params, teRcom=3, tepl=0.3), 32, 0, "IID", **(dict(conditions=conds) if conds else {}))
        spec = E.EnvSpec(E._Box(np.zeros(env.d * env.N), np.ones(env.d * env.N)), E._Discrete(5))
        torch.manual_seed(1)
        pol = nets.CommCategoricalMLPPolicy(spec, n_agents=env.N, n_gcn_layers=env.Lh, device="cuda:0")
        pol.set_rng(3)
        pol.sync_weights()
        eng = RolloutEngine(env, pol, H)
        eng.reset()
        made.append((env, pol, eng))
    (u_env, u_pol, u_eng), (c_env, c_pol, c_eng) = made
    assert u_eng.steps_fused(0, 2) is True                               # control: this shape has the fused kernels
    calls = []
    for name in ("step_fused", "chunk_fused"):
        real = getattr(c_pol, name)
        setattr(c_pol, name, lambda *a, _real=real, _name=name, **k: (calls.append(_name), _real(*a, **k))[1])
    assert c_eng.steps_fused(0, 2) is False
    assert calls == ["chunk_fused"] and c_eng._fused is False
    c_eng.step(0)
    c_eng.step(1)
    assert c_eng.steps_fused(0, 2) is False
    assert calls == ["chunk_fused"]                                      # not asked again after the 1
    c_eng2 = RolloutEngine(c_env, c_pol, H)
    c_eng2.reset()
    c_eng2.step(0)
    c_eng2.step(1)
    assert calls == ["chunk_fused", "step_fused"] and c_eng2._fused is False
    torch.cuda.synchronize()
    c_env.check_status()
