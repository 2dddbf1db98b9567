"""The rollout kernels' own env code - cm_env_pp10_dev.h inside rollout_w_kernel SHAPE 1 and its carried multi-step launch,
cm_rollout_wc.hip (per-env conditions), cm_rollout_wm.hip (a policy set), cm_fused.hip (the one-launch step of larger teams) -
started in the late game.  These kernels take their actions from the policy on the device, so no script can drive them; the
engines are loaded with a mid-hunt state instead (purposeful_teams.dense_start: every env holds one or two live preys with the
team around them), the state through set_state, agent_cond included, and what the oracle emitted at that step into slot 0 -
tests/test_purposeful_teams_env.py shows that emission equal to the kernels', bit for bit.

Per case: two chunks of 16 steps as persistent launches (fused_map20: 32 one-launch steps) against the same 32 steps as
two-launch steps on a second engine loaded the same way - every trajectory buffer and the final get_state() bit for bit - and
the 32 recorded action slots replayed through the oracle from the same snapshot: obs, reward64, done, success, prey_alive (and
dist_adj / channels where the engine records them) exact.  Floors, on the oracle replay: at least 8 episodes of the window end
by success, and its captures per env-step are at least 4 times those of a window of the same length from a reset under the same
policy (taken over 4096 envs - 512 of the larger teams - so that it is a rate and not a handful of captures; both rates are
printed)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import purposeful_teams as P

pytestmark = pytest.mark.gpu

H, CHUNK = P.DENSE_WINDOW, 16
BUFS = ("obs", "actions", "probs", "attn", "reward", "reward64", "done", "details", "prey_alive", "success", "path_len", "dist_adj",
        "channels")
POLICY_SEED = 5


BASE_ENVS = 4096          # the from-reset rate is taken over this many envs: over 64 it is 18 captures, give or take 5


def _env(name, lo=0, hi=None, **kw):
    """The GridEnvBatch of DENSE[name] (envs lo .. hi-1 of it: a member's share of a policy set, with its Philox env ids; hi
    beyond the case's batch: the larger batch of the from-reset rate, a condition table split in halves)."""
    from com_marl_amd import envs as E
    from tests import hip_adapters
    c = P.DENSE[name]
    hi = c["cfg"]["n_envs"] if hi is None else hi
    if c.get("conditions") and hi > c["cfg"]["n_envs"]:
        c = dict(c, condition_of=np.repeat(np.arange(2), hi // 2))
    cfg = O.make_cfg(**dict(c["cfg"], n_envs=hi - lo), rng_mode=O.RNG_PHILOX, seed=P.SEED, env_id_offset=lo)
    scen, p, ch = hip_adapters.params_from_cfg(cfg)
    if c.get("conditions"):
        kw.update(conditions=c["conditions"], condition_of=np.asarray(c["condition_of"]))
    return E.GridEnvBatch(scen, p, cfg.n_envs, device="cuda:0", seed=cfg.seed, env_id_offset=lo, max_steps=cfg.max_steps,
                          max_path_length=cfg.max_path_length, channel=ch, **kw)


def _policy(env, seed=POLICY_SEED):
    import torch
    from com_marl_amd import envs as E, nets
    spec = E.EnvSpec(E._Box(np.zeros(env.d * env.N), np.ones(env.d * env.N)), E._Discrete(5))
    torch.manual_seed(seed)
    pol = nets.CommCategoricalMLPPolicy(spec, n_agents=env.N, device="cuda:0")
    pol.set_rng(POLICY_SEED)
    return pol


def _load(eng, snap, lo=0, hi=None):
    """reset(), then the snapshot's state into the env batch and its emission into slot 0."""
    import torch
    eng.reset()
    rows = slice(lo, hi)
    eng.env.set_state(**{k: snap[k][rows] for k in P.DENSE_STATE if k != "ge_state"})
    for k in P.DENSE_OUTS:
        if getattr(eng, k) is not None:
            getattr(eng, k)[0].copy_(torch.as_tensor(np.array(snap[k][rows])))


def _play(eng, persistent):
    import torch
    if persistent:
        for t0 in range(0, H, CHUNK):
            assert eng.steps_fused(t0, CHUNK), "the library reported no persistent launch for this shape"
    else:
        for t in range(H):
            eng.step(t)
    torch.cuda.synchronize()
    eng.env.check_status()
    out = {k: getattr(eng, k).cpu().numpy() for k in BUFS if getattr(eng, k) is not None}
    out["state"] = eng.env.get_state()
    return out


def _assert_same(a, b, cols=slice(None)):
    assert sorted(a) == sorted(b)
    for k in sorted(b):
        if k == "state":
            for kk in sorted(b[k]):
                np.testing.assert_array_equal(a[k][kk][cols], b[k][kk], err_msg=f"state.{kk}")
        else:
            np.testing.assert_array_equal(a[k][:, cols], b[k], err_msg=k)


def _rate_from_reset(eng, persistent):
    """Captures per env-step of the window's length from a reset, under the policy of `eng` (an engine of BASE_ENVS envs)."""
    eng.reset()
    return int(_play(eng, persistent)["details"][:, :, 0].sum()) / (H * eng.env.B)


def _replay_and_floors(name, snap, run, rate0):
    """The recorded actions through the oracle from the snapshot; then the floors on what the oracle saw."""
    assert (snap["agent_cond"] == 1).all()
    live = snap["prey_alive"].sum(1)
    assert 2 * int(((live >= 1) & (live <= 2)).sum()) >= len(live)                   # at least half: here every env
    eo = P.make_oracle(name)
    eo.reset()
    eo.load_state(**{k: snap[k] for k in P.DENSE_STATE})
    np.testing.assert_array_equal(run["obs"][0], snap["obs"])
    captures = wins = 0
    for t in range(H):
        eo.step(run["actions"][t], n_threads=8)
        w = f"slot {t}"
        np.testing.assert_array_equal(run["obs"][t + 1], eo.obs, err_msg=w)
        np.testing.assert_array_equal(run["reward64"][t], eo.reward, err_msg=w)
        np.testing.assert_array_equal(run["done"][t], eo.done, err_msg=w)
        np.testing.assert_array_equal(run["success"][t], eo.success, err_msg=w)
        np.testing.assert_array_equal(run["prey_alive"][t], eo.prey_alive_info[:, :eo.M], err_msg=w)
        np.testing.assert_array_equal(run["details"][t], eo.details, err_msg=w)
        for k in ("dist_adj", "channels"):
            if k in run:
                np.testing.assert_array_equal(run[k][t + 1], getattr(eo, k), err_msg=w)
        captures += int(eo.details[:, 0].sum())
        wins += int((eo.done.astype(bool) & ~eo.prey_alive_info[:, :eo.M].astype(bool).any(1)).sum())
    rate = captures / (H * eo.B)
    print(f"\n{name}: {wins} success-ended episodes; captures per env-step {rate:.4f} from the dense start, {rate0:.4f} from a reset")
    assert wins >= 8
    assert rate >= 4 * rate0


def _engine(name, fused, persistent, n_envs=None, **env_kw):
    from com_marl_amd.rollout import RolloutEngine
    env = _env(name, 0, n_envs, **env_kw)
    return RolloutEngine(env, _policy(env), H, fused=fused, persistent=persistent)


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need the MI355X")
    return torch


@pytest.mark.parametrize("name", ["headline_full", "headline_ragged", "cond_full", "cond_ragged"])
def test_persistent_chunks_from_a_dense_start(name, gpu):
    """rollout_w_kernel SHAPE 1 / its condition twin, full workgroups (B = 64) and the ragged build (B = 209)."""
    snap = P.dense_start(name)
    cond = bool(P.DENSE[name].get("conditions"))
    kw = dict(fused_conditions=True) if cond else {}
    fast = _engine(name, True, True, **kw)
    slow = _engine(name, False, False)
    assert fast._persistent and not slow._persistent
    _load(fast, snap)
    _load(slow, snap)
    a, b = _play(fast, True), _play(slow, False)
    assert slow._fused is False
    _assert_same(a, b)
    _replay_and_floors(name, snap, a, _rate_from_reset(_engine(name, True, True, BASE_ENVS, **kw), True))


def test_policy_set_chunks_from_a_dense_start(gpu):
    """cm_rollout_wm: two members with 32 envs each (whole workgroups of 16) in one launch per chunk, against each member's
    own two-launch engine on its share of the snapshot.  The engine accepts set_state for a policy set: the env batch is the
    same GridEnvBatch."""
    from com_marl_amd import nets
    from com_marl_amd.rollout import RolloutEngine
    name, sizes = "set_of_two", [32, 32]
    snap = P.dense_start(name)
    env = _env(name)
    pols = [_policy(env, POLICY_SEED + k) for k in range(2)]
    eng = RolloutEngine(env, nets.PolicySet(pols), H, groups=sizes)
    assert eng.multi_form == "wave"
    eng.policy.sync_weights()
    _load(eng, snap)
    a = _play(eng, True)
    assert eng.multi_form == "wave"
    for k, (lo, hi) in enumerate(eng.groups):
        env_k = _env(name, lo, hi)
        ref = RolloutEngine(env_k, _policy(env_k, POLICY_SEED + k), H, fused=False, persistent=False)
        _load(ref, snap, lo, hi)
        _assert_same(a, _play(ref, False), cols=slice(lo, hi))
    big = RolloutEngine(_env(name, 0, BASE_ENVS), eng.policy, H, groups=[BASE_ENVS // 2] * 2)
    _replay_and_floors(name, snap, a, _rate_from_reset(big, True))


def test_fused_step_from_a_dense_start(gpu):
    """cm_fused.hip: Predator-Prey map 20, 24 agents with sensing range 2 hunting 2 preys, 13 envs - one launch per step
    against two."""
    name = "fused_map20"
    snap = P.dense_start(name)
    fast, slow = _engine(name, True, False), _engine(name, False, False)
    _load(fast, snap)
    _load(slow, snap)
    a, b = _play(fast, False), _play(slow, False)
    assert fast._fused is True and slow._fused is False
    _assert_same(a, b)
    _replay_and_floors(name, snap, a, _rate_from_reset(_engine(name, True, False, BASE_ENVS // 8), False))
