"""cm_graph_diameter (csrc/cm_graph_diam.hip), the part that needs no GPU: the symbol is declared, bound and exported; argument
errors come back as codes before anything is launched; the ISA of the new unit has no private segment, no spill and no flat
or scratch addressing; and the numpy restatement the GPU tests compare against (tests/graph_ref.py) gives the written-down
answers of the crafted graphs, agrees with networkx where that is importable, and sees both classes in the random draws."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import graph_cases, graph_ref, isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_bound_and_exported():
    from com_marl_amd import _lib as L
    assert "cm_graph_diameter" in L.EXPORTED
    assert hasattr(L.lib(), "cm_graph_diameter")
    assert "cm_graph_diameter(" in open(os.path.join(ROOT, "include", "commarl.h")).read()
    assert "cm_graph_diam" in isa.units()


def test_argument_errors_answer_without_a_gpu():
    from com_marl_amd import _lib as L
    lib = L.lib()
    p = C.c_void_p(16)                                          # plausible, never dereferenced: the checks precede the launch
    for bad in (lambda: lib.cm_graph_diameter(1, 0, p, p, None), lambda: lib.cm_graph_diameter(1, 256, p, p, None),
                lambda: lib.cm_graph_diameter(1, 4, None, p, None), lambda: lib.cm_graph_diameter(1, 4, p, None, None)):
        assert bad() == -1                                      # CM_ERR_ARG
        assert b"cm_graph_diameter" in lib.cm_last_error()
    assert lib.cm_graph_diameter(0, 4, None, None, None) == 0   # S = 0: nothing to do, nothing launched


def test_kernels_have_no_private_segment_no_spill_and_address_lds_by_offset():
    ks = isa.kernels(isa.listing("cm_graph_diam"))
    assert len(ks) == 4 and all("graph_diameter_kernel" in k.name for k in ks), [k.name for k in ks]   # 1 .. 4 words per row
    for k in ks:
        assert k.private_segment_fixed_size == 0, k.name
        assert k.vgpr_spill_count == 0, k.name
        assert not k.has_flat_or_scratch, k.name
        assert k.count("ds_") >= 1, k.name


def test_graph_ref_gives_the_written_down_answers():
    for name, adj, want in graph_cases.crafted():
        assert graph_ref.diameter(adj) == want, name


def test_random_draws_hold_both_classes():
    """At least a quarter connected and a quarter disconnected graphs per size, or the random cases would test one answer."""
    for n in graph_cases.RANDOM_N:
        d = graph_ref.diameters(graph_cases.random_batch(n))
        k = len(d)
        assert d.shape == (len(graph_cases.RANDOM_SEEDS),)
        if n > 1:
            assert 4 * int((d > 0).sum()) >= k and 4 * int((d == 0).sum()) >= k, (n, d.tolist())


def test_graph_ref_equals_networkx():
    nx = pytest.importorskip("networkx")
    graphs = [(name, adj) for name, adj, _ in graph_cases.crafted()]
    graphs += [(f"random{n}_{s}", graph_cases.random_graph(n, s)) for n in graph_cases.RANDOM_N for s in graph_cases.RANDOM_SEEDS]
    for name, adj in graphs:
        G = nx.from_numpy_array(adj)                            # the undirected graph networkx builds from a matrix
        want = nx.diameter(G) if nx.is_connected(G) else 0
        assert graph_ref.diameter(adj) == want, name
