"""Records tests/golden/graph_diameter.npz from the reference's OWN get_graph(..., calc_diameter=True)
(custom_implement/env_communication.py:218-243, loaded through oracle/ref_loader.py): fixed agent positions, the dist_adj it
builds from them and the diameter it reports.  Host only; needs the reference tree and a networkx that still has
from_numpy_matrix (get_graph calls it; networkx 3 removed it).  Where get_graph cannot run, NOTHING is recorded and the exit
status is 1 - the pins are then tests/graph_ref.py and networkx's own functions.  No test reads the file yet:
whoever records it adds, in new test files, the not-gpu test that holds tests/graph_ref.py to it and the gpu test that holds
cm_graph_diameter to it; until then the file pins nothing."""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "graph_diameter.npz")

# (n_agents, grid side, Rcom): teams and ranges of the bench configs, and one across a word boundary of the kernel's rows
CASES = [(4, 10, 2), (4, 10, 3), (24, 20, 3), (24, 20, 5), (72, 30, 5), (72, 30, 8), (130, 40, 6)]
DRAWS = 6


def main():
    try:
        import networkx as nx
    except ImportError:
        sys.exit("networkx is not importable: get_graph(calc_diameter=True) cannot run, nothing recorded")
    if not hasattr(nx, "from_numpy_matrix"):
        sys.exit(f"networkx {nx.__version__} has no from_numpy_matrix: get_graph(calc_diameter=True) cannot run, nothing recorded")
    from oracle.ref_loader import load_reference
    get_graph = load_reference().env_communication.get_graph
    out = {}
    for n, grid, rcom in CASES:
        rng = np.random.default_rng(100 * n + rcom)
        th = np.float32(np.sqrt(2.0) * rcom)                       # env_communication.py:73-75
        pos, adj, diam = [], [], []
        for _ in range(DRAWS):
            p = rng.integers(0, grid, (n, 2))
            a, _, d = get_graph(rcom, th, n, {i: [int(p[i, 0]), int(p[i, 1])] for i in range(n)}, True)
            pos.append(p)
            adj.append(np.asarray(a, np.float32))
            diam.append(int(d))
        key = f"n{n}_r{rcom}"
        out[key + ".pos"], out[key + ".dist_adj"], out[key + ".diameter"] = np.asarray(pos, np.int32), np.stack(adj), np.asarray(diam, np.int64)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(CASES)} cases x {DRAWS} draws")


if __name__ == "__main__":
    main()
