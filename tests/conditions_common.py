"""Shared by the per-env comm condition tests: the comparison against the uniform-condition kernels.

For condition c a fresh uniform batch W_c is built - same scenario, seed and channel kind, params carrying c's Rcom / pl / Pgb /
Pbg, as many envs as the slice and env_id_offset = the slice's first rng_id - and everything the env writes must be equal, bit for
bit, between the conditions batch's slice and W_c."""
import numpy as np

SEED = 3
OUTS = ("obs", "reward", "reward64", "done", "details", "prey_alive", "success_t", "dist_adj", "channels")
COND_TO_PARAM = dict(Rcom="teRcom", pl="tepl", Pgb="Pgb", Pbg="Pbg")


def base_params(scen, map_, sen, N, M, **over):
    """mode 'test': the env reads teRcom / tepl, the settings the reference's test runs sweep."""
    pp = scen == "pp"
    p = dict(load=2, max_env_steps=5, capture_reward=10 if pp else 2, step_cost=0.1 if pp else 0, rm=0,
             penalty=0 if pp else 1, revisit_penalty=0.5, lazy_penalty=1, grid_size=map_, Rsen=sen, n_agents=N, n_preys=M,
             n_gcn_layers=2, mode="test", teRcom=3, tepl=0.0, obstComplex="Easy", add_clock=0)
    p.update(over)
    return p


def with_condition(params, cond):
    p = dict(params)
    p.update({COND_TO_PARAM[k]: v for k, v in cond.items()})
    return p


def make_batch(scen, params, B, off, channel, max_steps=5, **kw):
    from com_marl_amd import envs as E
    return E.GridEnvBatch(scen, params, B, device="cuda:0", seed=SEED, env_id_offset=off, channel=channel, max_steps=max_steps,
                          max_path_length=max_steps, **kw)


def uniform_batch(scen, params, cond, n, off, channel, max_steps=5):
    """W_c: the parent commit's way to run condition c."""
    return make_batch(scen, with_condition(params, cond), n, off, channel, max_steps)


def random_actions(T, B, N, seed=0):
    import torch
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 5, (T, B, N), generator=g, dtype=torch.int32).to("cuda:0")


def snapshot(env, path_len=None):
    """Everything the env wrote, on the host: the output buffers, path_len when stepped, and get_state()."""
    s = {k: getattr(env, k).cpu().numpy() for k in OUTS}
    if path_len is not None:
        s["path_len"] = path_len.cpu().numpy()
    s.update({"state." + k: v for k, v in env.get_state().items()})
    return s


def drive(env, actions):
    """reset + one cm_env_step per row of `actions` -> the snapshots after the reset and after every step."""
    import torch
    pl = torch.zeros(env.B, dtype=torch.int32, device=env.device)
    env.reset_all()
    snaps = [snapshot(env)]
    for a in actions:
        env.step_device(a.contiguous(), out=dict(path_len=pl))
        snaps.append(snapshot(env, pl))
    env.check_status()
    return snaps


def assert_slice_equal(got, lo, hi, ref, what):
    assert len(got) == len(ref)
    for t, (g, r) in enumerate(zip(got, ref)):
        assert set(g) == set(r)
        for name in r:
            np.testing.assert_array_equal(g[name][lo:hi], r[name], err_msg=f"{what}, snapshot {t}, {name}")


def slices_differ(got, lo, hi, ref):
    return any(not np.array_equal(g[name][lo:hi], r[name]) for g, r in zip(got, ref) for name in r)


def slices_of(condition_of, rng_ids):
    """Maximal runs of envs with one condition and consecutive rng_ids: each is one W_c."""
    out, lo, B = [], 0, len(condition_of)
    for b in range(1, B + 1):
        if b == B or condition_of[b] != condition_of[lo] or rng_ids[b] != rng_ids[b - 1] + 1:
            out.append((lo, b, int(condition_of[lo]), int(rng_ids[lo])))
            lo = b
    return out


def offdiag_mean(channels):
    """Mean of the links i != j of channels [..., N, N] (the diagonal is always delivered, env_communication.py:212)."""
    N = channels.shape[-1]
    mask = ~np.eye(N, dtype=bool)
    return float(channels[..., mask].mean())
