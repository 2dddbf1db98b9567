"""The bootstrap of the evaluation scores without a device: the numpy reference the GPU tests compare against (tests/boot_ref.py)
is pinned first - its Philox against the oracle's and the Random123 known answers, its outputs against what must hold of any
bootstrap - then the refusals of ci= / n_boot= / boot_seed= / contrast= and of envs.bootstrap that are raised before anything is
built, the layout of the new sections, and the gfx950 ISA of csrc/cm_boot.hip (needs hipcc)."""
import numpy as np
import pytest
import torch

from tests import boot_ref as R
from tests import isa


# ---- the reference itself ---------------------------------------------------------------------------------------------------------
def test_numpy_philox_equals_the_oracles():
    from oracle import oracle as O
    rng = np.random.default_rng(11)
    ctr = rng.integers(0, 1 << 32, (300, 4), dtype=np.uint64)
    key = rng.integers(0, 1 << 32, (300, 2), dtype=np.uint64)
    ctr[:8] = [[r, q, R.SITE_BOOT, 0] for r in (0, 1, 4095) for q in (0, 1, 25)][:8]          # the counters the stream uses
    got = np.stack(R.philox4x32_10(*ctr.T, *key.T), axis=-1)
    for i in range(len(ctr)):
        assert tuple(int(x) for x in got[i]) == tuple(int(x) for x in O.philox(ctr[i], key[i])), (ctr[i], key[i])


def test_numpy_philox_known_answers():
    """The Random123 vectors tests/test_oracle_golden.py pins the oracle with."""
    kat = [
        ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
        ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
        ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
         (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
    ]
    for ctr, key, want in kat:
        assert tuple(int(x) for x in R.philox4x32_10(*ctr, *key)) == want


def test_index_stream_is_in_range_shared_and_roughly_uniform():
    idx = R.indices(101, 257, seed=5)
    assert idx.shape == (257, 101) and idx.min() >= 0 and idx.max() <= 100
    np.testing.assert_array_equal(idx[:100], R.indices(101, 100, seed=5))                  # resample r does not depend on R
    assert (R.indices(101, 257, seed=6) != idx).mean() > 0.9                                # the seed re-keys the stream
    # the words do not depend on n: the same draw scaled to another n
    w50 = R.indices(50, 64, seed=5)
    assert (np.abs(w50 / 50.0 - R.indices(100, 64, seed=5)[:, :50] / 100.0) <= 1 / 50.0).all()
    counts = np.bincount(R.indices(10, 4096, seed=1).ravel(), minlength=10)
    assert (np.abs(counts - 4096.0) < 6 * np.sqrt(4096 * 0.9)).all(), counts


@pytest.mark.parametrize("seed", [0, 7, (1 << 64) - 1])
def test_one_episode_gives_degenerate_intervals(seed):
    """n = 1: every resample is the one row - lo == hi == the value, and se == 0.  (The doubles here are multiples of 2^-20 below
    1: the sum of up to 4096 equal values, and so np.std's mean, is exact; for arbitrary doubles the mean of equal values may
    round, and se is then some ulps of the value - bounded below.)"""
    rng = np.random.default_rng(3)
    t = R.mixed_table(rng, 5, 1, 9)
    t[:, :, 0::4] = rng.integers(0, 1 << 20, t[:, :, 0::4].shape) / float(1 << 20)
    for n_boot, level in ((2, 0.5), (257, 0.9), (2000, 0.95)):
        out = R.bootstrap(t, level, n_boot, seed)
        assert (out[:, :, 0] == t[:, 0, :]).all() and (out[:, :, 1] == t[:, 0, :]).all()
        assert (out[:, :, 2] == 0).all()
    t = rng.normal(size=(5, 1, 6)) * 100.0                                                   # arbitrary doubles
    out = R.bootstrap(t, 0.95, 2000, seed)
    assert (out[:, :, 0] == t[:, 0, :]).all() and (out[:, :, 1] == t[:, 0, :]).all()
    assert (out[:, :, 2] <= 1e-12 * np.maximum(1.0, np.abs(t[:, 0, :]))).all()


@pytest.mark.parametrize("seed", [0, 1, 12345])
def test_interval_of_fifty_rows_holds_the_column_mean(seed):
    rng = np.random.default_rng(4)
    for cols in (4, 6, 9):
        t = R.mixed_table(rng, 5, 50, cols)
        out = R.bootstrap(t, 0.95, 2000, seed)
        mean = t.mean(1)
        assert (out[:, :, 0] <= mean).all() and (mean <= out[:, :, 1]).all()
        spread = t.std(1, ddof=1) / np.sqrt(50)                                              # the textbook standard error
        varying = spread > 0
        assert (np.abs(out[:, :, 2][varying] / spread[varying] - 1) < 0.15).all()
        assert (out[:, :, 2][~varying] == 0).all() and (out[:, :, 0][~varying] == 2.5).all()


def test_contrast_of_the_reference_is_paired():
    rng = np.random.default_rng(5)
    base = rng.normal(size=(1, 50, 4)) * 5.0
    t = np.concatenate([base, base + 0.25 + 0.01 * rng.normal(size=base.shape), base], axis=0)   # cell 1 = cell 0 + ~0.25; cell 2 = cell 0
    out, v = R.quantiles(R.means(t, 500, 9), *R.ranks(0.9, 500), "columns", ref_cell=[0, 0, 0])
    assert (out[0] == [0.0, 0.0, 0.0, 0.5]).all() and (out[2] == [0.0, 0.0, 0.0, 0.5]).all() and (v[0] == 0).all()
    assert (out[1, :, 0] > 0.2).all() and (out[1, :, 1] < 0.3).all() and (out[1, :, 3] == 1.0).all()   # far tighter than either cell's own
    own = R.bootstrap(t, 0.9, 500, 9)
    assert ((own[1, :, 1] - own[1, :, 0]) > 10 * (out[1, :, 1] - out[1, :, 0])).all()


def test_ranks():
    from com_marl_amd import envs
    for level, n_boot in ((0.95, 2000), (0.9, 257), (0.5, 2), (0.999, 3), (0.01, 4096), (0.9, 100)):
        assert envs.boot_ranks(level, n_boot) == R.ranks(level, n_boot)
        lo, hi = R.ranks(level, n_boot)
        assert 0 <= lo <= hi < n_boot and hi == n_boot - 1 - lo
    assert R.ranks(0.95, 2000) == (50, 1949) and R.ranks(0.999, 3) == (0, 2) and R.ranks(0.01, 4096) == (2027, 2068)
    assert R.ranks(0.01, 2) == (0, 1) and R.ranks(0.01, 3) == (1, 1)                        # capped at the median: lo <= hi


# ---- the refusals that need no device -------------------------------------------------------------------------------------------
class _Batch:
    conditions = [dict(Rcom=9, pl=0), dict(Rcom=2, pl=0.3), dict(Rcom=1, pl=0.9)]


class _Env:
    batch = _Batch()


def _raises(fn, match, *a, **kw):
    with pytest.raises(ValueError, match=match):
        fn(*a, **kw)


@pytest.mark.parametrize("who", ["eval_summary", "eval_sweep"])
def test_refusals_of_the_keywords_before_anything_is_built(who):
    from com_marl_amd import evaluate
    fn = getattr(evaluate, who)
    env, pols = _Env(), [object(), object()]
    for bad in (0, 1, -0.5, 1.5, float("nan"), "0.9", True):
        _raises(fn, r"ci=", env, pols, ci=bad)
    for bad in (1, 0, 4097, -3, 2.5, None):
        _raises(fn, r"n_boot=", env, pols, ci=0.9, n_boot=bad)
    for bad in (-1, 1 << 64, 0.5, None):
        _raises(fn, r"boot_seed=", env, pols, ci=0.9, boot_seed=bad)
    _raises(fn, r"n_boot= is read with ci= only", env, pols, n_boot=100)
    _raises(fn, r"boot_seed= is read with ci= only", env, pols, boot_seed=1)


def test_refusals_of_contrast():
    from com_marl_amd import evaluate
    env, pols = _Env(), [object(), object()]
    sweep = evaluate.eval_sweep
    _raises(sweep, r"contrast= is read with ci= only", env, pols, contrast=dict(condition=0))
    _raises(sweep, r"contrast= needs paired=True", env, pols, ci=0.9, paired=False, contrast=dict(condition=0))
    for bad in (dict(), dict(condition=0, policy=0), dict(cell=0), [0], 0):
        _raises(sweep, r"contrast= takes", env, pols, ci=0.9, contrast=bad)
    for bad in (dict(condition=3), dict(condition=-1), dict(policy=2), dict(policy=0.0), dict(condition=None)):
        _raises(sweep, r"contrast=dict\(.*index", env, pols, ci=0.9, contrast=bad)
    _raises(sweep, r"contrast=dict\(policy=1", env, object(), ci=0.9, contrast=dict(policy=1))     # a single policy: K = 1
    # eval_summary: its policies play unpaired envs
    _raises(evaluate.eval_summary, r"contrast= is eval_sweep's", env, pols, ci=0.9, contrast=dict(policy=0))
    _raises(evaluate.eval_summary, r"contrast= is eval_sweep's", env, pols, contrast=dict(policy=0))


def test_contrast_cells():
    from com_marl_amd.evaluate import _contrast_cells
    assert _contrast_cells("x", None, 2, 3) is None
    assert _contrast_cells("x", dict(condition=1), 2, 3) == [1, 1, 1, 4, 4, 4]
    assert _contrast_cells("x", dict(policy=1), 2, 3) == [3, 4, 5, 3, 4, 5]


def test_refusals_of_envs_bootstrap():
    from com_marl_amd import envs
    t = torch.zeros(3, 5, 4, dtype=torch.float64)
    _raises(envs.bootstrap, r"level=", t, 1.0)
    _raises(envs.bootstrap, r"n_boot=", t, 0.9, n_boot=1)
    _raises(envs.bootstrap, r"n_boot=", t, 0.9, n_boot=4097)
    _raises(envs.bootstrap, r"seed=", t, 0.9, seed=-1)
    _raises(envs.bootstrap, r"kind=", t, 0.9, kind="value")                                  # 4 columns are not the value family's 6
    _raises(envs.bootstrap, r"kind=", t, 0.9, kind="median")
    _raises(envs.bootstrap, r"kind=", torch.zeros(3, 5, 5, dtype=torch.float64), 0.9)
    for bad in ([0, 1, 3], [0, -1, 0], [0, 1]):
        _raises(envs.bootstrap, r"ref_cell=", t, 0.9, ref_cell=bad)
    assert [envs.boot_keys(k, c) for k, c in (("columns", 4), ("columns", 6), ("columns", 9), ("comm", 4), ("value", 6))] == [4, 6, 9, 5, 7]


def test_layout_keeps_its_sections_and_appends_the_bootstrap_blocks():
    from com_marl_amd.evaluate import FAMILIES, _cut, _host_tables, _layout
    fams = list(FAMILIES.values())
    for curves in (False, True):
        plain = _layout(4, 7, fams, curves)
        assert _layout(4, 7, fams, curves, ()) == plain
        both = _layout(4, 7, fams, curves, ("boot", "contrast"))
        assert both[:len(plain)] == plain
        assert both[len(plain):] == [(f"{name}_{b}", (4, keys, 4)) for b in ("boot", "contrast")
                                     for name, keys in (("summary", 9), ("comm", 5), ("attn", 6), ("listen", 6), ("value", 7))]
        flat = np.arange(sum(int(np.prod(s)) for _, s in both), dtype=np.float64)
        host, raw = _host_tables(flat, both), _cut(flat, both)
        for name, shape in both:                                                             # only curve tables are transposed
            if name.endswith("curves"):
                np.testing.assert_array_equal(host[name], raw[name].transpose(0, 2, 1))
            else:
                assert host[name].shape == shape and np.shares_memory(host[name], flat)
    for switch, fam in FAMILIES.items():                                                     # the device keys are the host keys, in order
        names = list(fam.keys(np.ones((fam.cols, 1))))
        assert names == R.key_names(fam.kind, fam.cols) or fam.kind == "columns"
        assert len(names) == (5 if fam.kind == "comm" else 7 if fam.kind == "value" else fam.cols)


# ---- the unit's ISA ---------------------------------------------------------------------------------------------------------------
def test_no_kernel_of_cm_boot_uses_scratch_or_spills():
    ks = isa.kernels(isa.listing("cm_boot"))
    names = [k.name for k in ks]
    assert len([n for n in names if "boot_means_kernel" in n]) == 3 * 2, names               # cols 4, 6, 9 x staged / global
    assert len([n for n in names if "boot_quantiles_kernel" in n]) == 1, names
    assert len(ks) == 7, names
    for k in ks:
        assert k.private_segment_fixed_size == 0, (k.name, k.private_segment_fixed_size)
        assert k.vgpr_spill_count == 0, (k.name, k.vgpr_spill_count)
        assert not any(ln.startswith("scratch_") for ln in k.lines), k.name
