"""PathBatch.gather_index / padded (sampler.py): the one gather of the time-major engine buffers into the padded [P, T, ...] batch
that process_samples and _log_performance share - against a plain numpy loop, over a stand-in engine that holds CPU tensors."""
import types

import numpy as np
import pytest
import torch

from com_marl_amd.sampler import PathBatch

H, B, N, D = 6, 3, 2, 3                                     # horizon (step slots), envs, agents, per-agent observation
# (env, first slot, length): one step long; ending in the last slot H - 1; two of the same env
PATHS = [(0, 2, 1), (1, 1, 5), (2, 0, 3), (2, 3, 2)]


def _batch():
    rng = np.random.RandomState(7)
    eng = types.SimpleNamespace(
        generation=0,
        obs=torch.as_tensor(rng.rand(H + 1, B, N, D).astype(np.float32)) + 1,      # (+1: no genuine zero to take for padding)
        dist_adj=torch.as_tensor((rng.rand(H + 1, B, N, N) > 0.5).astype(np.float32)) * 0.5,
        reward64=torch.as_tensor(rng.randn(H, B)))
    env, start, length = (torch.tensor(c, dtype=torch.int64) for c in zip(*PATHS))
    return eng, PathBatch(eng, env, start, length, N)


def _loop(buf, pad):
    buf = buf.numpy()
    T = max(n for _, _, n in PATHS)
    out = np.full((len(PATHS), T) + buf.shape[2:], pad, dtype=buf.dtype)
    for p, (b, s, n) in enumerate(PATHS):
        for tau in range(n):
            out[p, tau] = buf[s + tau, b]
    return out


@pytest.mark.parametrize("name,pad", [("obs", 0), ("dist_adj", 1), ("reward64", 0)])
def test_padded_matches_a_numpy_loop(name, pad):
    eng, batch = _batch()
    got = batch.padded(name, pad)
    want = _loop(getattr(eng, name), pad)
    assert got.dtype == getattr(eng, name).dtype and tuple(got.shape) == want.shape
    np.testing.assert_array_equal(got.numpy(), want)
    assert batch.host_buffers == []                           # a device-side gather: no engine buffer came to the host


def test_index_is_built_once_and_stays_inside_the_buffers():
    eng, batch = _batch()
    P, T, valid, t_idx, b_idx = idx = batch.gather_index()
    assert (P, T) == (4, 5) and valid.shape == t_idx.shape == b_idx.shape == (4, 5)
    np.testing.assert_array_equal(valid.sum(1).numpy(), [n for _, _, n in PATHS])
    assert int(t_idx.max()) == H - 1 and int(t_idx.min()) >= 0   # the clamp: slot H - 1 exists in the H-slot buffers too
    for name, pad in (("obs", 0), ("reward64", 0), ("dist_adj", 1)):
        batch.padded(name, pad)
    assert batch.gather_index() is idx and batch.gather_index()[3] is t_idx


def test_a_later_rollout_makes_the_batch_stale():
    eng, batch = _batch()
    batch.padded("reward64", 0)
    eng.generation += 1                                       # what RolloutEngine.reset() does
    with pytest.raises(RuntimeError, match="earlier rollout"):
        batch.padded("reward64", 0)
    with pytest.raises(RuntimeError, match="earlier rollout"):
        batch.gather_index()
