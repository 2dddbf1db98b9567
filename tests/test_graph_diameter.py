"""cm_graph_diameter on the GPU against tests/graph_ref.py: the crafted graphs (every word boundary of the bitmask rows, the
level bound, lone vertices, one-way edges, odd weights, both diagonals), seeded G(N, p) draws near the connectivity threshold,
launches ragged against four graphs per workgroup with guarded output buffers, and a side stream."""
import numpy as np
import pytest

from tests import graph_cases, graph_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need the MI355X")
    return torch


def _run(torch, adj):
    from com_marl_amd.envs import graph_diameter
    out = graph_diameter(torch.as_tensor(np.ascontiguousarray(adj, np.float32)).to("cuda:0"))
    return out.cpu().numpy()


def test_crafted_graphs(torch_cuda):
    got = {}
    for name, adj, want in graph_cases.crafted():
        d = _run(torch_cuda, adj[None])
        assert d.shape == (1,) and d.dtype == np.int32
        got[name] = (int(d[0]), want)
    bad = {k: v for k, v in got.items() if v[0] != v[1]}
    assert not bad, f"(kernel, expected): {bad}"


@pytest.mark.parametrize("n", graph_cases.RANDOM_N)
def test_random_graphs_near_the_connectivity_threshold(torch_cuda, n):
    batch = graph_cases.random_batch(n)
    want = graph_ref.diameters(batch)
    np.testing.assert_array_equal(_run(torch_cuda, batch), want)
    # leading axes are the caller's: [slots, envs, N, N] as the engine holds them
    np.testing.assert_array_equal(_run(torch_cuda, batch.reshape(4, 4, n, n)), want.reshape(4, 4))


@pytest.mark.parametrize("n", [24, 72])
@pytest.mark.parametrize("S", [1, 5, 37])
def test_ragged_launches_write_exactly_S_ints(torch_cuda, S, n):
    """Four graphs per workgroup: S = 1, 5, 37 leave one to three waves of the last workgroup without a graph.  The output is
    prefilled with -1 and sits between guard elements."""
    torch = torch_cuda
    from com_marl_amd.envs import graph_diameter
    adj = np.stack([graph_cases.random_graph(n, s % 16) if s % 3 else graph_cases.path(n) for s in range(S)])
    want = graph_ref.diameters(adj)
    guard = 8
    buf = torch.full((S + 2 * guard,), -7, dtype=torch.int32, device="cuda:0")
    buf[guard:guard + S] = -1
    graph_diameter(torch.as_tensor(adj).to("cuda:0"), out=buf[guard:guard + S])
    h = buf.cpu().numpy()
    np.testing.assert_array_equal(h[guard:guard + S], want)
    assert (h[:guard] == -7).all() and (h[guard + S:] == -7).all()


def test_side_stream(torch_cuda):
    torch = torch_cuda
    from com_marl_amd.envs import graph_diameter
    batch = graph_cases.random_batch(72)
    dev = torch.as_tensor(batch).to("cuda:0")
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):
        out = graph_diameter(dev)
    side.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), graph_ref.diameters(batch))
