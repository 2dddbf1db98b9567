"""CPU-side checks of the multi-policy rollout (cm_rollout_chunk_multi): the kernel compiles for gfx950 without private memory,
spills or flat / scratch addressing, and the entry point is part of the C ABI without a version bump."""
import os
import re

import pytest

from tests import isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_multi_policy_rollout_kernels_use_no_flat_or_scratch_addressing():
    """Every rollout_wm_kernel instantiation (cm_rollout_wm.hip) is held to what test_cabi holds rollout_w_kernel to: no
    private segment, no VGPR spill, no flat / scratch instruction, one workgroup barrier (behind the weight staging)."""
    ks = isa.kernels(isa.listing("cm_rollout_wm"), "rollout_wm_kernel")
    assert len(ks) == 16, len(ks)   # 1 / 2 hops x (plain, env prefetch, carried, carried map10) x (full / ragged workgroups)
    for k in ks:
        assert k.private_segment_fixed_size == 0, k.name
        assert k.vgpr_spill_count == 0, k.name
        assert not k.has_flat_or_scratch, k.name
        assert k.barriers == 1, k.name


def test_chunk_multi_is_declared_and_exported_at_abi_3():
    from com_marl_amd import _lib
    src = open(os.path.join(ROOT, "include", "commarl.h")).read()
    assert re.search(r"\bint\s+cm_rollout_chunk_multi\s*\(", src)
    assert "cm_policy_set" in src
    assert "cm_rollout_chunk_multi" in _lib.EXPORTED
    lib = _lib.lib()
    assert hasattr(lib, "cm_rollout_chunk_multi")
    assert lib.cm_abi_version() == 3
    import ctypes as C
    assert C.sizeof(_lib.PolicySetT) == 2 * 4 + 2 * 8


def test_policy_set_refuses_mixed_architectures_without_gpu():
    """The architecture rule is a host-side check: CPU nets show it (the rollout itself needs the GPU)."""
    import numpy as np
    import torch
    from com_marl_amd import envs as E, nets
    spec = E.EnvSpec(E._Box(np.zeros(21 * 4), np.ones(21 * 4)), E._Discrete(5))
    spec6 = E.EnvSpec(E._Box(np.zeros(21 * 6), np.ones(21 * 6)), E._Discrete(5))
    a = nets.CommCategoricalMLPPolicy(spec, n_agents=4)
    nets.PolicySet([a, nets.CommCategoricalMLPPolicy(spec, n_agents=4)])
    with pytest.raises(ValueError, match="hops"):
        nets.PolicySet([a, nets.CommCategoricalMLPPolicy(spec, n_agents=4, n_gcn_layers=1)])
    with pytest.raises(ValueError, match="team size"):
        nets.PolicySet([a, nets.CommCategoricalMLPPolicy(spec6, n_agents=6)])
    with pytest.raises(ValueError, match="class"):
        nets.PolicySet([a, nets.DecCategoricalMLPPolicy(spec, n_agents=4)])
    d = nets.DecCategoricalMLPPolicy(spec, n_agents=4)
    with pytest.raises(ValueError, match="nonlinearity"):
        nets.PolicySet([d, nets.DecCategoricalMLPPolicy(spec, n_agents=4, hidden_nonlinearity=torch.relu)])
    with pytest.raises(ValueError):
        nets.PolicySet([])
