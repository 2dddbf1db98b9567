"""Not a test: the semantics of cm_graph_diameter restated in numpy (a level-synchronous BFS from every source), what the
new tests hold the kernel, the engine's diameter slots and the wrappers to.

Vertices i != j are joined when adj[i][j] != 0 or adj[j][i] != 0 (the undirected graph networkx builds from a matrix; any
non-zero value is an edge), the diagonal is ignored.  A connected graph gives its largest shortest-path hop count (0 for one
vertex), a disconnected one 0 - get_graph's calc_diameter branch of the reference (env_communication.py:235-241)."""
import numpy as np


def edges(adj):
    a = np.asarray(adj)
    assert a.ndim == 2 and a.shape[0] == a.shape[1]
    e = (a != 0) | (a.T != 0)
    np.fill_diagonal(e, False)
    return e


def diameter(adj):
    e = edges(adj)
    N = e.shape[0]
    ef = e.astype(np.float32)
    reach = np.eye(N, dtype=bool)                       # reach[s]: what source s has reached so far
    frontier = reach.copy()
    ecc = np.zeros(N, np.int64)
    for level in range(1, N):                           # a shortest path has at most N - 1 hops
        nxt = ((frontier.astype(np.float32) @ ef) > 0) & ~reach
        grew = nxt.any(axis=1)
        if not grew.any():
            break
        ecc[grew] = level
        reach |= nxt
        frontier = nxt
    return int(ecc.max()) if reach.all() else 0


def diameters(adj, n=None):
    """[..., N, N] - or, with n given, flattened graphs [..., n*n] as the path dicts hold them - -> int64 [...]."""
    a = np.asarray(adj)
    if n is not None:
        assert a.shape[-1] == n * n
        a = a.reshape(a.shape[:-1] + (n, n))
    lead = a.shape[:-2]
    flat = a.reshape((-1,) + a.shape[-2:])
    return np.asarray([diameter(g) for g in flat], np.int64).reshape(lead)
