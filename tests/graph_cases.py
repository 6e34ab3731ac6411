"""Graphs the graph-search tests share (tests/test_graph_host.py, tests/test_gpu_graph.py)."""
import numpy as np


def ring(lo, hi, n):
    """neighbors int32 [n, 8]: inside [lo, hi) row i -> i +- 1 .. 4 around the ring; the other rows have no edge."""
    nb = np.full((n, 8), -1, np.int32)
    m = hi - lo
    for i in range(lo, hi):
        nb[i] = [lo + (i - lo + d) % m for d in (1, -1, 2, -2, 3, -3, 4, -4)]
    return nb
