"""cm_boot_means and cm_boot_quantiles (csrc/cm_boot.hip) through ctypes and envs.bootstrap, against the numpy reference
(tests/boot_ref.py) on tables whose columns cycle through random doubles, small integers (many ties), 0/1 and a constant.

The resampled means are the same sequential f64 sums on both sides: compared with ==.  So are lo, hi and p_gt of keys that are
columns or differences of columns.  delivery, value_rmse and value_ev take a division or a root per value, correctly rounded on
both sides - == is expected, 8 ulps of max(1, |x|) allowed (boot_ref.check_out).  se is two sums of at most 4096 terms in another
order than np.std's: rtol 1e-9, atol 1e-12 max(1, max |v|) - far below the difference between the divisors R - 1 and R.
Launches are repeated and compared bit for bit, and the outputs sit between sentinel guard rows."""
import numpy as np
import pytest

from tests import boot_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -77.0
GUARD = 16                                                      # guard doubles in front of and behind each output
STAGE_BYTES = 32 * 1024                                         # the staging budget of cm_boot_means (include/commarl.h)
KINDS = {"columns": 0, "comm": 1, "value": 2}
DERIVED = {"columns": (), "comm": (4,), "value": (3, 4)}        # the keys that take a division or a root


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch


def _guarded(torch, numel):
    return torch.full((numel + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda")


def _inner(buf, shape):
    host = buf.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[-GUARD:] == SENTINEL).all(), "guard doubles written"
    return host[GUARD:-GUARD].reshape(shape)


def _means(torch, table, n_boot, seed):
    """One cm_boot_means launch on a device table -> (the guarded device buffer, its host view [cells, R, cols])."""
    from com_marl_amd import _lib as L
    cells, n, cols = table.shape
    buf = _guarded(torch, cells * n_boot * cols)
    L.check(L.lib().cm_boot_means(cells, n, cols, L.ptr(table), n_boot, seed & 0xFFFFFFFF, seed >> 32, L.ptr(buf[GUARD:]),
                                  L.current_stream()), "cm_boot_means")
    return buf, _inner(buf, (cells, n_boot, cols))


def _quantiles(torch, means_buf, cells, n_boot, cols, kind, ref, lo, hi):
    from com_marl_amd import _lib as L, envs
    keys = envs.boot_keys(kind, cols)
    buf = _guarded(torch, cells * keys * 4)
    L.check(L.lib().cm_boot_quantiles(KINDS[kind], cells, n_boot, cols, L.ptr(means_buf[GUARD:]), L.ptr(ref), lo, hi,
                                      L.ptr(buf[GUARD:]), L.current_stream()), "cm_boot_quantiles")
    return _inner(buf, (cells, keys, 4))


def _table(kind, cells, n, cols, seed):
    rng = np.random.default_rng(seed)
    t = R.mixed_table(rng, cells, n, cols)
    if kind == "comm":                                          # range_degree the small integers: resamples with nobody in range
        t[:, :, [0, 1]] = t[:, :, [1, 0]]
    if kind == "value" and seed % 2:                            # moments that belong together: E[G^2] >= E[G]^2, a real explained variance
        v, g = rng.normal(size=(2, cells, n)) * 4.0
        t[:, :, 0], t[:, :, 1], t[:, :, 2], t[:, :, 3] = v, g, (v - g) ** 2, g * g
    return t


# (cols, cells, n, R, (lo_rank, hi_rank) or the level, kind, ref_cell or None, seed): every cols, cells 1 and 5, n 1 / 3 / 12 / 101
# and 456 - 9 columns just above the staging budget (455 rows fit) -, every R, lo_rank = 0, lo_rank == hi_rank, every kind, and
# reference tables with self-references
CASES = [
    (4, 1, 1, 2, (0, 1), "columns", None, 0),
    (4, 5, 3, 3, (1, 1), "comm", [0, 0, 2, 1, 4], 1),
    (6, 5, 12, 100, (0, 99), "value", None, 2),
    (6, 1, 101, 257, 0.9, "columns", None, 3),
    (9, 5, 101, 2000, 0.95, "columns", [1, 1, 1, 3, 0], (1 << 64) - 1),
    (9, 1, 456, 4096, 0.95, "columns", None, 5),
    (6, 5, 12, 257, 0.5, "value", [4, 1, 0, 3, 3], 7),
    (4, 5, 101, 100, (0, 50), "comm", None, 8),
]


@pytest.mark.parametrize("case", CASES, ids=[f"c{c[0]}-g{c[1]}-n{c[2]}-R{c[3]}-{c[5]}{'-ref' if c[6] else ''}" for c in CASES])
def test_entry_points_equal_the_reference(gpu, case):
    cols, cells, n, n_boot, rk, kind, ref, seed = case
    lo, hi = rk if isinstance(rk, tuple) else R.ranks(rk, n_boot)
    assert (n * cols * 8 > STAGE_BYTES) == (n == 456) and (n - 1) * cols * 8 <= STAGE_BYTES
    host = _table(kind, cells, n, cols, seed)
    table = gpu.from_numpy(host).cuda()
    want_means = R.means(host, n_boot, seed)
    buf, got_means = _means(gpu, table, n_boot, seed)
    np.testing.assert_array_equal(got_means, want_means)
    np.testing.assert_array_equal(_means(gpu, table, n_boot, seed)[1], got_means)                # two launches: the same bits
    ref_dev = None if ref is None else gpu.tensor(ref, dtype=gpu.int32, device="cuda")
    want, v = R.quantiles(want_means, lo, hi, kind, ref)
    got = _quantiles(gpu, buf, cells, n_boot, cols, kind, ref_dev, lo, hi)
    R.check_out(got, want, v, DERIVED[kind], str(case))
    print(f"{case}: max |got - want| lo/hi {np.abs(got[..., :2] - want[..., :2]).max():.3e}, se {np.abs(got[..., 2] - want[..., 2]).max():.3e}, "
          f"p_gt {np.abs(got[..., 3] - want[..., 3]).max():.3e}")
    np.testing.assert_array_equal(_quantiles(gpu, buf, cells, n_boot, cols, kind, ref_dev, lo, hi), got)
    for g in ([g for g, r in enumerate(ref) if r == g] if ref else []):                         # a cell against itself
        assert (got[g] == [0.0, 0.0, 0.0, 0.5]).all(), got[g]
    if n == 1 and ref is None and kind == "columns":
        assert (got[:, :, 0] == host[:, 0, :]).all() and (got[:, :, 1] == host[:, 0, :]).all()


@pytest.mark.parametrize("cols,n", [(4, 101), (6, 12), (9, 455)])
def test_staged_and_global_routes_give_the_same_bits(gpu, monkeypatch, cols, n):
    host = _table("columns", 3, n, cols, 21)
    table = gpu.from_numpy(host).cuda()
    monkeypatch.delenv("COMMARL_BOOT_STAGE_BYTES", raising=False)
    staged = _means(gpu, table, 300, 9)[1]
    monkeypatch.setenv("COMMARL_BOOT_STAGE_BYTES", "0")         # nothing fits: the global-memory route
    flat = _means(gpu, table, 300, 9)[1]
    monkeypatch.setenv("COMMARL_BOOT_STAGE_BYTES", str(n * cols * 8))   # exactly this table: staged again
    again = _means(gpu, table, 300, 9)[1]
    np.testing.assert_array_equal(staged, flat)
    np.testing.assert_array_equal(staged, again)
    np.testing.assert_array_equal(staged, R.means(host, 300, 9))


def test_envs_bootstrap(gpu):
    from com_marl_amd import envs
    host = _table("comm", 5, 50, 4, 31)
    table = gpu.from_numpy(host).cuda()
    for kind, ref in (("columns", None), ("comm", None), ("comm", [2, 2, 2, 0, 4])):
        got = envs.bootstrap(table, 0.9, n_boot=257, seed=4, kind=kind, ref_cell=ref)
        assert got.is_cuda and got.dtype == gpu.float64 and tuple(got.shape) == (5, envs.boot_keys(kind, 4), 4)
        m = R.means(host, 257, 4)
        want, v = R.quantiles(m, *R.ranks(0.9, 257), kind, ref)
        R.check_out(got.cpu().numpy(), want, v, DERIVED[kind], kind)
    assert gpu.equal(envs.bootstrap(table, 0.9, 257, 4), envs.bootstrap(table, 0.9, 257, 4))
    assert not gpu.equal(envs.bootstrap(table, 0.9, 257, 4), envs.bootstrap(table, 0.9, 257, 5))   # the seed re-keys the resamples


def test_refusals_launch_nothing(gpu):
    from com_marl_amd import _lib as L
    lib = L.lib()
    table = gpu.zeros(2, 5, 4, dtype=gpu.float64, device="cuda")
    means = _guarded(gpu, 2 * 10 * 4)
    out = _guarded(gpu, 2 * 5 * 4)
    ref = gpu.zeros(2, dtype=gpu.int32, device="cuda")
    st = L.current_stream()
    t, m, o = L.ptr(table), L.ptr(means[GUARD:]), L.ptr(out[GUARD:])
    bad_means = [(0, 5, 4, t, 10, m), (2, 0, 4, t, 10, m), (2, 5, 5, t, 10, m), (2, 5, 8, t, 10, m), (2, 5, 4, t, 1, m), (2, 5, 4, t, 4097, m),
                 (2, 5, 4, None, 10, m), (2, 5, 4, t, 10, None), (-1, 5, 4, t, 10, m), (2, -5, 4, t, 10, m)]
    for cells, n, cols, tab, n_boot, dst in bad_means:
        assert lib.cm_boot_means(cells, n, cols, tab, n_boot, 0, 0, dst, st) == -1, (cells, n, cols, n_boot)
        assert b"cm_boot_means" in lib.cm_last_error()
    # (kind, cells, R, cols, means, lo_rank, hi_rank, out)
    bad_quant = [(3, 2, 10, 4, m, 0, 9, o), (-1, 2, 10, 4, m, 0, 9, o), (0, 2, 10, 5, m, 0, 9, o), (1, 2, 10, 6, m, 0, 9, o),
                 (2, 2, 10, 4, m, 0, 9, o), (0, 0, 10, 4, m, 0, 9, o), (0, 2, 1, 4, m, 0, 0, o), (0, 2, 4097, 4, m, 0, 9, o),
                 (0, 2, 10, 4, m, -1, 9, o), (0, 2, 10, 4, m, 5, 4, o), (0, 2, 10, 4, m, 0, 10, o), (0, 2, 10, 4, None, 0, 9, o),
                 (0, 2, 10, 4, m, 0, 9, None)]
    for kind, cells, n_boot, cols, src, lo, hi, dst in bad_quant:
        for r in (None, L.ptr(ref)):
            assert lib.cm_boot_quantiles(kind, cells, n_boot, cols, src, r, lo, hi, dst, st) == -1, (kind, cells, n_boot, cols, lo, hi)
            assert b"cm_boot_quantiles" in lib.cm_last_error()
    gpu.cuda.synchronize()
    assert (means.cpu().numpy() == SENTINEL).all() and (out.cpu().numpy() == SENTINEL).all(), "a refused call wrote"
    # and the same arguments made right are accepted
    assert lib.cm_boot_means(2, 5, 4, t, 10, 0, 0, m, st) == 0 and lib.cm_boot_quantiles(1, 2, 10, 4, m, L.ptr(ref), 0, 9, o, st) == 0
    assert (_inner(out, (2, 5, 4))[0] == [0.0, 0.0, 0.0, 0.5]).all()            # cell 0 against itself
