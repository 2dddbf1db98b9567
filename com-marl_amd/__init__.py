"""com_marl_amd - MI355X-native batched rollout + GNN-PPO hot path of Com-MARL.

Host-side mirror of the reference's operator interface (same class names, ctor kwargs and
argument meaning) over the C ABI of libcommarl_hip.so (include/commarl.h).  The HIP library
is mandatory: nothing here falls back to a CPU implementation.
"""
from . import _lib
from ._lib import CommarlError, lib  # noqa: F401

__all__ = ["lib", "CommarlError", "envs", "nets", "sampler", "algos", "set_deterministic", "deterministic"]

_deterministic = None


def set_deterministic(on):
    """Deterministic update mode: True / False force it; None (the default) follows COMMARL_DETERMINISTIC=1 or
    torch.are_deterministic_algorithms_enabled().  In this mode every cross-workgroup sum of the PPO update is merged in a
    fixed order, so a training run repeats bit for bit on the same GPU type with the same seeds and shapes."""
    global _deterministic
    if on is not None and not isinstance(on, bool):
        raise TypeError("set_deterministic takes True, False or None")
    _deterministic = on


def deterministic():
    """Whether the update runs in deterministic mode now (read at every launch choice, like the other COMMARL_* knobs)."""
    if _deterministic is not None:
        return _deterministic
    import os
    if os.environ.get("COMMARL_DETERMINISTIC", "") == "1":
        return True
    import torch
    return torch.are_deterministic_algorithms_enabled()


def __getattr__(name):
    import importlib
    if name in ("envs", "nets", "sampler", "algos", "dist", "dropin"):
        return importlib.import_module(f"{__name__}.{name}")
    raise AttributeError(name)
