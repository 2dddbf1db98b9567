"""CPU-side checks of the multi-policy rollout (cm_rollout_chunk_multi): the kernel compiles for gfx950 without private memory,
spills or flat / scratch addressing, and the entry point is part of the C ABI without a version bump."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_multi_policy_rollout_kernels_use_no_flat_or_scratch_addressing(tmp_path):
    """Every rollout_wm_kernel instantiation (cm_rollout_wm.hip) is held to what test_cabi holds rollout_w_kernel to: no
    private segment, no VGPR spill, no flat / scratch instruction, one workgroup barrier (behind the weight staging)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "com-marl_amd", "csrc", "cm_rollout_wm.hip")
    out = tmp_path / "cm_rollout_wm.s"
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-mllvm",
                           "-amdgpu-mfma-vgpr-form", "-fno-slp-vectorize", "-S", "--cuda-device-only", "-w", "-o", str(out), src])
    asm = out.read_text()
    seen = 0
    for blk in re.split(r"\n\s+- \.agpr_count:", asm)[1:]:                 # one metadata block per kernel
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if "rollout_wm_kernel" not in name:
            continue
        seen += 1
        assert re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1) == "0", name
        assert re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1) == "0", name
    assert seen == 16, seen     # 1 / 2 hops x (plain, env prefetch, carried, carried map10) x (full / ragged workgroups)
    bodies = list(re.finditer(r"^(_ZN2cm17rollout_wm_kernel\S+):[^\n]*\n(.*?)\n\.Lfunc_end", asm, re.M | re.S))
    assert len(bodies) == seen
    for m in bodies:
        assert not re.search(r"^\s+(flat_(load|store|atomic)|scratch_)", m.group(2), re.M), m.group(1)
        assert len(re.findall(r"^\s+s_barrier", m.group(2), re.M)) == 1, m.group(1)


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
