"""Per-env comm conditions in the wave-owned rollout (csrc/cm_rollout_wc.hip), the part that needs no GPU: the C-ABI symbol that
switches it on, the unit's compile flags, and the gfx950 ISA of every twin beside the rollout_w_kernel / rollout_wm_kernel build of
the same template arguments."""
import ctypes as C
import itertools
import os
import re

import pytest

from tests import isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# what a lane keeps of its env's record through the launch: rc2, ploss, pgb, pbg and the Philox id offset (EnvCondVals)
RECORD_VGPRS = 5
# hops, env prefetch, full workgroups; the two-hop plain builds are not shipped: no handle reaches them (cm_rollout_wc.hip)
BUILDS = [b for b in itertools.product((1, 2), (True, False), (True, False)) if b[:2] != (2, False)]


def test_symbol_is_declared_exported_and_bound():
    from com_marl_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "commarl.h")).read(), flags=re.S)
    assert re.search(r"\bint cm_env_fuse_conditions\s*\(\s*cm_env_t h,\s*int32_t on\s*\)", src)
    assert "cm_env_fuse_conditions" in _lib.EXPORTED
    lib = _lib.lib()
    assert lib.cm_env_fuse_conditions.restype is C.c_int
    assert lib.cm_abi_version() == 3                                      # a symbol was only added
    assert lib.cm_env_fuse_conditions(None, 1) == -1
    assert b"cm_env_fuse_conditions: null handle" in lib.cm_last_error()


def test_wrappers_take_the_keyword():
    import inspect
    from com_marl_amd import envs
    assert inspect.signature(envs.GridEnvBatch.__init__).parameters["fused_conditions"].default is False
    assert inspect.signature(envs._WrapperBase.__init__).parameters["fused_conditions"].default is False
    assert inspect.signature(envs.GridEnvBatch.fuse_conditions).parameters["on"].default is True
    assert callable(envs.PredatorPreyWrapper.fuse_conditions) and callable(envs.CoverageWrapper.fuse_conditions)


def test_unit_is_built_without_slp_vectorisation():
    assert "cm_rollout_wc" in isa.units()
    cmd = isa.compile_command("cm_rollout_wc", "/dev/null")
    assert "-fno-slp-vectorize" in cmd, cmd
    mk = open(os.path.join(isa.csrc(), "Makefile")).read()
    dbg = re.search(r"^DBG_SRC\s*:=\s*(.*)$", mk, re.M).group(1).split()
    assert "cm_rollout_wc.hip" in dbg                                     # the unit includes cm_env_dev.h: CM_BOUNDS changes it
    assert re.search(r"_build/dbg/cm_rollout_wc\.o[^\n]*: HIPFLAGS \+= -fno-slp-vectorize", mk)


def _flat_or_scratch(k):
    return sum(1 for ln in k.lines if isa.FLAT_OR_SCRATCH.match(ln))


def _vgprs(k):
    return k._meta_int("vgpr_count")


def _b(x):
    return "Lb1" if x else "Lb0"


def test_the_unit_holds_the_twelve_twins_and_nothing_else():
    asm = isa.listing("cm_rollout_wc")
    names = sorted(k.name for k in isa.kernels(asm))
    want = sorted(f"_ZN2cm{len(n)}{n}ILi{L}E{_b(pre)}E{_b(full)}EE" for n in ("rollout_wc_kernel", "rollout_wcm_kernel")
                  for L, pre, full in BUILDS)
    assert [n[:len(w)] for n, w in zip(names, want)] == want and len(names) == len(want), names


@pytest.mark.parametrize("hops, pre, full", BUILDS, ids=[f"{L}hop-{'pre' if p else 'plain'}-{'full' if f else 'ragged'}" for L, p, f in BUILDS])
def test_twins_cost_no_more_than_the_record(hops, pre, full):
    """Beside the sibling of the same template arguments (non-carried, SHAPE 0, no tape): no more flat / scratch instructions, no
    larger private segment, no spilled VGPR, and at most the record's five VGPRs more.  The sibling's values are read from its
    own listing."""
    wc = isa.listing("cm_rollout_wc")
    args = f"ILi{hops}E{_b(pre)}E{_b(full)}E"
    pairs = [(isa.kernel(wc, "_ZN2cm17rollout_wc_kernel" + args + "E"),
              isa.kernel(isa.listing("cm_rollout_w"), "_ZN2cm16rollout_w_kernel" + args + "Lb0ELb0ELi0EE")),
             (isa.kernel(wc, "_ZN2cm18rollout_wcm_kernel" + args + "E"),
              isa.kernel(isa.listing("cm_rollout_wm"), "_ZN2cm17rollout_wm_kernel" + args + "Lb0ELi0EE"))]
    for twin, sib in pairs:
        print(f"{twin.name}: VGPRs {_vgprs(twin)} (sibling {_vgprs(sib)}), SGPR spills {twin._meta_int('sgpr_spill_count')} "
              f"({sib._meta_int('sgpr_spill_count')}), scratch {twin.private_segment_fixed_size} ({sib.private_segment_fixed_size}), "
              f"lines {len(twin.lines)} ({len(sib.lines)})")
        assert _flat_or_scratch(twin) <= _flat_or_scratch(sib), twin.name
        assert twin.private_segment_fixed_size <= sib.private_segment_fixed_size, twin.name
        assert twin.vgpr_spill_count <= sib.vgpr_spill_count, twin.name
        assert _vgprs(twin) <= _vgprs(sib) + RECORD_VGPRS, twin.name
        assert twin.barriers == sib.barriers == 1, twin.name               # the one behind the weight staging
