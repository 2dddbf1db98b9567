"""Per-env comm conditions, the part that needs no GPU: the record's layout, the two new C-ABI symbols and their argument
errors, the numpy mirror (envs.condition_table, evaluate.sweep_layout) and the gfx950 ISA of csrc/cm_env_cond.hip."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PP = dict(load=2, max_env_steps=20, capture_reward=10, step_cost=0.1, rm=0, penalty=0, grid_size=10, Rsen=1, n_agents=4,
          n_preys=4, n_gcn_layers=2, mode="test", teRcom=3, tepl=0.25, seed=5)


def test_record_is_32_bytes_in_the_header_and_in_ctypes():
    from com_marl_amd import _lib, envs
    src = open(os.path.join(ROOT, "include", "commarl.h")).read()
    body = re.search(r"typedef struct cm_env_cond \{(.*?)\} cm_env_cond;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip() for f in body.split(";") if f.strip()]
    assert fields == ["int32_t rcom", "float   ploss, pgb, pbg", "int32_t rng_id", "int32_t reserved[3]"]
    assert 4 + 3 * 4 + 4 + 3 * 4 == 32
    assert C.sizeof(_lib.EnvCond) == 32
    assert envs.COND_DTYPE.itemsize == 32
    assert [envs.COND_DTYPE.fields[n][1] for n in ("rcom", "ploss", "pgb", "pbg", "rng_id", "reserved")] == [0, 4, 8, 12, 16, 20]
    assert [getattr(_lib.EnvCond, n).offset for n in ("rcom", "ploss", "pgb", "pbg", "rng_id", "reserved")] == [0, 4, 8, 12, 16, 20]


def test_symbols_are_declared_exported_and_bound():
    from com_marl_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "commarl.h")).read(), flags=re.S)
    lib = _lib.lib()
    for name in ("cm_env_set_conditions", "cm_env_has_conditions"):
        assert re.search(r"\bint " + name + r"\s*\(", src), name
        assert name in _lib.EXPORTED
        assert getattr(lib, name).restype is C.c_int
    assert lib.cm_abi_version() == 3                                      # symbols were only added


def test_argument_errors_without_gpu():
    from com_marl_amd import _lib
    lib = _lib.lib()
    table = (_lib.EnvCond * 2)()
    assert lib.cm_env_set_conditions(None, table, None) == -1
    assert b"null handle" in lib.cm_last_error()
    assert lib.cm_env_set_conditions(None, None, None) == -1
    assert lib.cm_env_has_conditions(None) == -1
    assert b"null" in lib.cm_last_error()


# ---- envs.condition_table ------------------------------------------------------------------------------------------------
def test_condition_table_defaults_and_values():
    from com_marl_amd import envs
    conds = [dict(), dict(Rcom=2, pl=0.5), dict(pl=1.0)]
    of = np.array([0, 1, 2, 1, 0])
    t = envs.condition_table("pp", PP, conds, of, env_id_offset=100)
    assert t.dtype == envs.COND_DTYPE and t.shape == (5,) and t.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(t["rcom"], [3, 2, 3, 2, 3])            # a missing key: what make_cfg takes from params
    np.testing.assert_array_equal(t["ploss"], np.float32([0.25, 0.5, 1.0, 0.5, 0.25]))
    np.testing.assert_array_equal(t["pgb"], np.float32([0.0196] * 5))
    np.testing.assert_array_equal(t["pbg"], np.float32([0.282] * 5))
    np.testing.assert_array_equal(t["rng_id"], 100 + np.arange(5))       # the id the env has without a table
    assert not t["reserved"].any()
    t = envs.condition_table("pp", PP, conds, of, rng_ids=[7, 7, 8, 8, 9], env_id_offset=100)
    np.testing.assert_array_equal(t["rng_id"], [7, 7, 8, 8, 9])
    # train mode reads the tr* keys
    tr = dict(PP, mode="train", trRcom=4, trpl=0.125)
    t = envs.condition_table("pp", tr, [dict()], np.zeros(3, int))
    np.testing.assert_array_equal(t["rcom"], [4, 4, 4])
    np.testing.assert_array_equal(t["ploss"], np.float32([0.125] * 3))
    # GE: Pgb / Pbg per condition
    t = envs.condition_table("co", dict(PP, grid_size=20), [dict(Pgb=0.1), dict(Rcom=5, Pbg=0.9)], np.array([1, 0]), channel="GE")
    np.testing.assert_array_equal(t["rcom"], [5, 3])
    np.testing.assert_array_equal(t["pgb"], np.float32([0.0196, 0.1]))
    np.testing.assert_array_equal(t["pbg"], np.float32([0.9, 0.282]))


def test_conditions_channel_rule():
    from com_marl_amd import envs
    assert envs.conditions_channel([dict(pl=0), dict(pl=0.3)]) == "IID"
    assert envs.conditions_channel([dict(pl=0), dict(pl=1), dict(Rcom=2)]) is None        # make_cfg derives it from params
    assert envs.conditions_channel([dict(pl=0.3)], "GE") == "GE"
    # params with pl = 0 give FC; one lossy condition makes the batch IID
    fc = dict(PP, tepl=0)
    assert envs.make_cfg("pp", fc, 2)[1] == "FC"
    t = envs.condition_table("pp", fc, [dict(), dict(pl=0.3)], np.array([0, 1]))
    np.testing.assert_array_equal(t["ploss"], np.float32([0.0, 0.3]))


@pytest.mark.parametrize("conds, of, kw, text", [
    ([dict(Rcom=1)], [0, 1], {}, "outside"),                              # index outside the list
    ([dict(Rcom=1)], [-1], {}, "outside"),
    ([], [0], {}, "at least one"),
    ([dict(pl=0.5)], [0], dict(channel="GE"), "not IID"),                 # pl given, channel not IID
    ([dict(pl=0.0)], [0], dict(params=dict(PP, tepl=0)), "not IID"),      # ... the derived FC kind included
    ([dict(Pgb=0.1)], [0], {}, "not GE"),                                 # Pgb / Pbg given, channel not GE
    ([dict(Pbg=0.1)], [0], dict(channel="IID"), "not GE"),
    ([dict(pl=1.5)], [0], {}, "outside [0, 1]"),
    ([dict(pl=-0.1)], [0], dict(channel="IID"), "outside [0, 1]"),
    ([dict(Pgb=2.0)], [0], dict(channel="GE"), "outside [0, 1]"),
    ([dict(Pbg=-1.0)], [0], dict(channel="GE"), "outside [0, 1]"),
    ([dict(Rcom=-1)], [0], {}, "Rcom"),
    ([dict(Rcom=1.5)], [0], {}, "Rcom"),
    ([dict(rcom=1)], [0], {}, "unknown"),
    ([dict(Rcom=1)], [0.0], {}, "int array"),
    ([dict(Rcom=1)], [0, 0], dict(rng_ids=[1]), "rng_ids"),
    ([dict(Rcom=1)], [0], dict(rng_ids=[2 ** 31]), "32-bit"),
])
def test_condition_table_refusals(conds, of, kw, text):
    from com_marl_amd import envs
    kw = dict(kw)
    params = kw.pop("params", PP)
    with pytest.raises(ValueError, match=re.escape(text)):
        envs.condition_table("pp", params, conds, np.asarray(of), **kw)


# ---- evaluate.sweep_layout -----------------------------------------------------------------------------------------------
def test_sweep_layout():
    from com_marl_amd import evaluate
    K, C_, E = 2, 3, 4
    B = K * C_ * E
    of, ids = evaluate.sweep_layout(B, K, C_, 50, True)
    assert of.shape == ids.shape == (B,)
    for k in range(K):
        for c in range(C_):
            for e in range(E):
                b = (k * C_ + c) * E + e
                assert of[b] == c and ids[b] == 50 + e                   # paired: every cell sees the same streams
    of2, ids2 = evaluate.sweep_layout(B, K, C_, 50, False)
    np.testing.assert_array_equal(of2, of)
    np.testing.assert_array_equal(ids2, 50 + np.arange(B))
    of1, ids1 = evaluate.sweep_layout(6, 1, 3)
    np.testing.assert_array_equal(of1, [0, 0, 1, 1, 2, 2])
    np.testing.assert_array_equal(ids1, [0, 1, 0, 1, 0, 1])
    for bad in ((25, 2, 3), (24, 0, 3), (24, 2, 0), (0, 1, 1)):
        with pytest.raises(ValueError):
            evaluate.sweep_layout(*bad)


# ---- the kernels ---------------------------------------------------------------------------------------------------------
def test_cond_kernels_use_no_flat_or_scratch_addressing():
    """DESIGN §10 for the twins: the by-value copy of EnvDev with five per-env fields is taken apart by the compiler - no
    private segment, no flat / scratch instruction, no spilled register in any of PP / CO x 16 / 32 / 64 lanes + the two wide
    forms."""
    asm = isa.listing("cm_env_cond")
    ks = isa.kernels(asm, "env_cond_kernel")
    assert len(ks) >= 8, [k.name for k in ks]
    assert len(isa.kernels(asm, "env_cond_kernel_wide")) == 2
    assert len(isa.kernels(asm)) == len(ks)                               # the unit holds nothing else
    for k in ks:
        assert not k.has_flat_or_scratch, k.name
        assert k.private_segment_fixed_size == 0, k.name
        assert k.vgpr_spill_count == 0, k.name
