"""The host-side round of the evaluation (evaluate._first_episodes) against a stub engine that records its calls: which
launches a round asks for with the chunk attempt off, accepted and declined, in which order, and what it reads off the
trajectory buffers (the first end of every env, the mean degree only where the engine records an adjacency)."""
import numpy as np
import torch

from com_marl_amd import evaluate
from com_marl_amd.rollout import RolloutEngine

T, B, N = 5, 3, 4


class _Engine:
    """What a round touches of a RolloutEngine, on the CPU.  Env 0 ends at t = 1 and t = 3, env 1 never, env 2 at t = 4."""
    play = getattr(RolloutEngine, "play", None)           # the engine's own round player, on the stub's launches

    def __init__(self, accept, adjacency=True):
        self.calls, self.accept = [], accept
        H = T + 1                                                              # one slot more than a round plays
        g = torch.Generator().manual_seed(0)
        self.path_len = torch.zeros(H, B, dtype=torch.int32)
        self.path_len[1, 0], self.path_len[3, 0], self.path_len[4, 2], self.path_len[T, 1] = 2, 2, 5, 9
        self.reward64 = torch.rand(H, B, generator=g, dtype=torch.float64)
        self.details = torch.randint(0, 9, (H, B, 6), generator=g, dtype=torch.int32)
        self.success = torch.randint(0, 2, (H, B), generator=g, dtype=torch.int32)
        self.done = (self.path_len > 0).to(torch.uint8)
        self.dist_adj = (torch.rand(H + 1, B, N, N, generator=g) < 0.5).float() if adjacency else None
        self.batch = self                                                       # base.batch.check_status()

    def reset(self):
        self.calls.append("reset")

    def steps_fused(self, t0, n, greedy=False, tail=False):
        self.calls.append(("steps_fused", t0, n, greedy, tail))
        return self.accept

    def fork(self):
        self.calls.append("fork")

    def step(self, t, greedy=False):
        self.calls.append(("step", t, greedy))

    def join(self):
        self.calls.append("join")

    def bump(self, n):
        self.calls.append(("bump", n))

    def check_status(self):
        self.calls.append("check_status")


def _round(eng, greedy, chunk):
    """One round with the chunk attempt on or off (off is the default: not passed)."""
    return evaluate._first_episodes(eng, eng, T, greedy, **(dict(chunk=True) if chunk else {}))


def _stepped(greedy):
    return ["fork"] + [("step", t, greedy) for t in range(T)] + ["join"]


def test_chunk_off_steps_one_by_one_and_never_asks_for_the_chunk():
    for greedy in (True, False):
        eng = _Engine(accept=True)
        _round(eng, greedy, chunk=False)
        assert eng.calls == ["reset"] + _stepped(greedy) + [("bump", T), "check_status"]


def test_chunk_on_and_accepted_takes_no_step():
    eng = _Engine(accept=True)
    _round(eng, True, chunk=True)
    assert eng.calls == ["reset", ("steps_fused", 0, T, True, False), ("bump", T), "check_status"]


def test_chunk_on_and_declined_asks_once_then_steps():
    for greedy in (True, False):
        eng = _Engine(accept=False)
        _round(eng, greedy, chunk=True)
        assert eng.calls == ["reset", ("steps_fused", 0, T, greedy, False)] + _stepped(greedy) + [("bump", T), "check_status"]


def test_first_end_of_every_env_and_the_host_arrays():
    for chunk in (False, True):
        eng = _Engine(accept=True)
        h = _round(eng, True, chunk)
        np.testing.assert_array_equal(h["first"], [1, T - 1, 4])               # ends at t = 1 and t = 3: the first; never: T - 1
        assert h["first"].dtype == np.int64
        for name, buf in (("reward", eng.reward64), ("details", eng.details), ("success", eng.success), ("done", eng.done)):
            np.testing.assert_array_equal(h[name], buf[:T].numpy())
        assert h["deg"].shape == (T + 1, B)
        np.testing.assert_array_equal(h["deg"], eng.dist_adj[:T + 1].sum(-1).mean(-1).numpy())
        assert set(h) == {"first", "reward", "details", "success", "done", "deg"}


def test_no_degree_without_a_recorded_adjacency():
    for chunk in (False, True):
        h = _round(_Engine(accept=True, adjacency=False), True, chunk)
        assert set(h) == {"first", "reward", "details", "success", "done"}
