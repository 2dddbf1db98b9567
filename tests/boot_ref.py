"""A pure-numpy reference of the bootstrap entry points cm_boot_means / cm_boot_quantiles (include/commarl.h): Philox4x32-10 in
uint64 arithmetic, the index stream, the sequential column sums, the keys through the package's own host functions (_named,
_comm_keys, _value_keys) and the four outputs through np.sort / np.std / counts.  A helper, not a test; it needs neither the
oracle nor a device."""
import math

import numpy as np

SITE_BOOT = 10
M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays (or scalars) of counters and keys that broadcast -> four uint64 arrays holding the 32-bit words."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(np.asarray(x, np.uint64) & M32 for x in (c0, c1, c2, c3, k0, k1)))
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2        # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def indices(n, R, seed=0):
    """-> int64 [R, n]: idx[r][j] = (w_j * n) >> 32, w_j component j & 3 of philox(r, j >> 2, SITE_BOOT, 0; seed lo, seed hi)."""
    r = np.arange(R, dtype=np.uint64)[:, None]
    q = np.arange((n + 3) // 4, dtype=np.uint64)[None, :]
    words = philox4x32_10(r, q, SITE_BOOT, 0, int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    w = np.stack(words, axis=-1).reshape(R, -1)[:, :n]                          # [R, 4 * ceil(n / 4)]: draw j at column j
    return ((w * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def means(table, R, seed=0):
    """table [cells, n, cols] -> [cells, R, cols]: per resample the column sums, sequential in ascending j, divided once."""
    table = np.asarray(table, np.float64)
    cells, n, cols = table.shape
    idx = indices(n, R, seed)
    s = np.zeros((cells, R, cols))
    for j in range(n):                                                          # one add per j, in order: no pairwise summation
        s = s + table[:, idx[:, j], :]
    return s / float(n)


def ranks(level, n_boot):
    lo = min(math.floor((1 - level) / 2 * n_boot), (n_boot - 1) // 2)
    return lo, n_boot - 1 - lo


def key_names(kind, cols):
    from com_marl_amd import evaluate as ev
    if kind == "comm":
        return list(ev.COMM_KEYS)
    if kind == "value":
        return list(ev.VALUE_KEYS)
    return [f"c{i}" for i in range(cols)]


def key_values(m, kind):
    """Resampled means [cells, R, cols] -> [keys, cells, R] through the package's host functions."""
    from com_marl_amd import evaluate as ev
    cols = np.moveaxis(np.asarray(m, np.float64), 2, 0)                         # [cols, cells, R]
    fn = {"comm": ev._comm_keys, "value": ev._value_keys}.get(kind) or ev._named(key_names("columns", len(cols)))
    with np.errstate(all="ignore"):
        d = fn(cols)
    assert list(d) == key_names(kind, len(cols))
    return np.stack([np.broadcast_to(np.asarray(v, np.float64), cols[0].shape) for v in d.values()])


def quantiles(m, lo_rank, hi_rank, kind="columns", ref_cell=None):
    """Resampled means [cells, R, cols] -> ([cells, keys, 4]: lo, hi, se, p_gt; the values v [cells, keys, R] behind them)."""
    v = np.moveaxis(key_values(m, kind), 0, 1)                                  # [cells, keys, R]
    if ref_cell is not None:
        v = v - v[np.asarray(ref_cell, np.int64)]
    R = v.shape[-1]
    srt = np.sort(v, axis=-1)
    p_gt = ((v > 0).sum(-1) + 0.5 * (v == 0).sum(-1)) / R
    return np.stack([srt[..., lo_rank], srt[..., hi_rank], np.std(v, axis=-1, ddof=1), p_gt], axis=-1), v


def bootstrap(table, level, n_boot=2000, seed=0, kind="columns", ref_cell=None):
    """envs.bootstrap's twin -> [cells, keys, 4]."""
    return quantiles(means(table, n_boot, seed), *ranks(level, n_boot), kind, ref_cell)[0]


def mixed_table(rng, cells, n, cols):
    """A table whose columns cycle through four kinds: random doubles, small integers (many ties), 0/1, one constant."""
    t = np.empty((cells, n, cols))
    for c in range(cols):
        kind = c % 4
        t[:, :, c] = (rng.normal(size=(cells, n)) * 3.0 if kind == 0 else rng.integers(0, 4, (cells, n)) if kind == 1 else
                      rng.integers(0, 2, (cells, n)) if kind == 2 else 2.5)
    return t


ULP8 = 8 * 2.0 ** -52


def check_out(got, want, v, derived, what=""):
    """The comparison rules of the bootstrap tests, got / want [cells, keys, 4], v [cells, keys, R] the reference's values:
    lo, hi, p_gt == for keys that are columns (or their differences); for the `derived` key indices (a division or a root per
    value) within 8 ulps of max(1, |x|); se against np.std(ddof=1) with rtol 1e-9, atol 1e-12 max(1, max |v|)."""
    keys = got.shape[1]
    for k in range(keys):
        for col, name in ((0, "lo"), (1, "hi"), (3, "p_gt")):
            g, w = got[:, k, col], want[:, k, col]
            if k in derived and col != 3:
                assert (np.abs(g - w) <= ULP8 * np.maximum(1.0, np.abs(w))).all(), (what, k, name, g, w)
            elif k in derived:                                                  # a count: only a value within ulps of 0 may change sides
                assert (np.abs(g - w) <= (np.abs(v[:, k]) <= ULP8).sum(-1) / v.shape[-1]).all(), (what, k, name, g, w)
            else:
                assert (g == w).all(), (what, k, name, g, w)
        atol = 1e-12 * np.maximum(1.0, np.abs(v[:, k]).max(-1))
        assert (np.abs(got[:, k, 2] - want[:, k, 2]) <= atol + 1e-9 * np.abs(want[:, k, 2])).all(), (what, k, "se", got[:, k, 2], want[:, k, 2])
