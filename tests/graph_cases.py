"""Not a test: the graphs the cm_graph_diameter tests share - crafted ones with the answer written next to them, and seeded
G(N, p) draws near the connectivity threshold.  Every matrix is float32 [N, N] as the env records dist_adj."""
import numpy as np


def _empty(n):
    return np.zeros((n, n), np.float32)


def _join(a, i, j, w=1.0, both=True):
    a[i, j] = w
    if both:
        a[j, i] = w


def path(n, both=True, lower=False):
    a = _empty(n)
    for i in range(n - 1):
        _join(a, i + 1, i, both=both) if lower else _join(a, i, i + 1, both=both)
    return a


def path_over(order):
    """The path that visits the vertices in `order`."""
    a = _empty(len(order))
    for u, v in zip(order[:-1], order[1:]):
        _join(a, u, v)
    return a


def ring(n, weights=(1.0,)):
    a = _empty(n)
    for i in range(n):
        _join(a, i, (i + 1) % n, w=weights[i % len(weights)])
    return a


def star(n, centre):
    a = _empty(n)
    for i in range(n):
        if i != centre:
            _join(a, centre, i)
    return a


def complete(n):
    return np.ones((n, n), np.float32) - np.eye(n, dtype=np.float32)


def complete_but(n, lone):
    """Every vertex joined to every other, except `lone`, which has no edge at all."""
    a = complete(n)
    a[lone, :] = 0
    a[:, lone] = 0
    return a


def two_components(n, cut):
    a = _empty(n)
    for i in range(n - 1):
        if i + 1 != cut:
            _join(a, i, i + 1)
    return a


def crafted():
    """[(name, adj, diameter)]: the answers are written down here, not computed (tests hold graph_ref AND the kernel to them)."""
    cases = [("n1", _empty(1), 0), ("n2_joined", path(2), 1), ("n2_apart", _empty(2), 0)]
    cases += [(f"path{n}", path(n), n - 1) for n in (5, 64, 65, 128, 129, 255)]     # the level bound and every word boundary
    # both ends among the first 64 vertices: the sources of the later passes all have smaller eccentricities
    cases += [("path70_ends_0_1", path_over([0] + list(range(2, 70)) + [1]), 69),
              ("path200_ends_5_6", path_over([5] + [v for v in range(200) if v not in (5, 6)] + [6]), 199)]
    cases += [("ring65", ring(65), 32), ("star130", star(130, 77), 2), ("complete24", complete(24), 1),
              ("two_components10", two_components(10, 4), 0), ("two_components200", two_components(200, 128), 0),
              ("lone0_n130", complete_but(130, 0), 0), ("lone64_n130", complete_but(130, 64), 0),
              ("lone_last_n130", complete_but(130, 129), 0), ("lone_last_n24", complete_but(24, 23), 0),
              ("one_way_up70", path(70, both=False), 69), ("one_way_down70", path(70, both=False, lower=True), 69),
              ("one_way_up4", path(4, both=False), 3),
              ("weights_ring9", ring(9, weights=(0.5, -2.0)), 4), ("weights_ring140", ring(140, weights=(0.5, -2.0, 1e-30)), 70)]
    out = []
    for name, a, d in cases:                                   # the diagonal is ignored: all zero and all one, the same answers
        out.append((name + "_diag0", a, d))
        b = a.copy()
        np.fill_diagonal(b, 1.0)
        out.append((name + "_diag1", b, d))
    return out


RANDOM_N = (4, 24, 72, 200)
RANDOM_SEEDS = tuple(range(16))


def random_p(n):
    """Near the threshold: G(N, (ln N + c) / N) is connected with probability -> exp(-exp(-c)), 0.55 at c = 0.5 (less at these
    sizes), so both classes turn up.  N = 4: the formula is of no use at this size; 0.5 gives 38 connected graphs in 64."""
    return 0.5 if n == 4 else float((np.log(n) + 0.5) / n)


def random_graph(n, seed):
    """G(n, p) whose edges are recorded in one direction or both, with weights that are not 1, and a random diagonal."""
    rng = np.random.default_rng(1000 * n + seed)
    up = np.triu(rng.random((n, n)) < random_p(n), 1)
    way = rng.integers(0, 3, (n, n))                           # 0: [i][j] only, 1: [j][i] only, 2: both
    w = rng.choice(np.asarray([1.0, 0.5, -2.0], np.float32), (n, n))
    a = np.where(up & (way != 1), w, 0).astype(np.float32)
    a += np.where(up & (way != 0), w, 0).astype(np.float32).T
    a[np.diag_indices(n)] = rng.integers(0, 2, n)
    return a


def random_batch(n):
    return np.stack([random_graph(n, s) for s in RANDOM_SEEDS])
