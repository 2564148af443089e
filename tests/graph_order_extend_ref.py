"""A pure-Python restatement of velo_graph_order_extend's rule (include/velo_hip.h) on top of graph_order_ref.py, written from the
header's text -- NOT from the library's code.  Test infrastructure only.

The rule: the extended order is perm_old followed by the new nodes in ascending number; the first dirty row p is the smallest position
among the ends of the new edges and the new nodes (n when nothing is new); the fresh order is graph_order_ref.order's, reversed as a
whole when that moves node n - 1 from the first half of the positions to the second and the reversed order's work is within RATIO of
the unreversed one's; the extended order is kept iff its work is <= max_work and <= RATIO times the fresh order's, otherwise the result
is the fresh order and p = 0.  stats = (widest row, blocks, work, components, p, rebuilt, reversed, the fresh order's work)."""
import numpy as np

import graph_order_ref as O

RATIO = 2                                                              # VELO_GRAPH_RETAIN_REBUILD_RATIO


def fresh(n, a, b):
    """(perm, first, (widest, blocks, work), components, reversed): graph_order_ref's order, oriented"""
    perm, first, (widest, blocks, work, components) = O.order(n, a, b)
    if n == 0:
        return perm, first, (widest, blocks, work), components, False
    nb = O.neighbours(n, a, b)
    at = int(np.nonzero(perm == n - 1)[0][0])
    if 2 * at < n and 2 * (n - 1 - at) >= n:
        back = perm[::-1].copy()
        bfirst, bstats = O.stats_of(nb, back)
        if bstats[2] <= RATIO * work:
            return back, bfirst, bstats, components, True
    return perm, first, (widest, blocks, work), components, False


def order_extend(n_old, perm_old, n, a, b, first_new_edge, max_work):
    """(perm, first, stats[8]) for the graph on nodes 0 .. n - 1 whose first n_old nodes were ordered as perm_old"""
    nb = O.neighbours(n, a, b)
    fperm, ffirst, fstats, components, reversed_ = fresh(n, a, b)
    perm = np.array(list(perm_old) + list(range(n_old, n)), dtype=np.int64)
    pos = np.empty(n, dtype=np.int64)
    pos[perm] = np.arange(n)
    touched = [int(pos[int(v)]) for e in range(first_new_edge, len(a)) for v in (a[e], b[e])] + ([n_old] if n_old < n else [])
    p = min(touched) if touched else n
    first, stats = O.stats_of(nb, perm)
    old_nb = O.neighbours(n_old, a[:first_new_edge], b[:first_new_edge])
    old_first, _ = O.stats_of(old_nb, np.asarray(perm_old, dtype=np.int64))
    assert np.array_equal(first[:min(p, n_old)], old_first[:min(p, n_old)])      # the rows before p keep their first
    if stats[2] <= max_work and stats[2] <= RATIO * fstats[2]:
        return perm, first, (*stats, components, p, 0, 0, fstats[2])
    return fperm, ffirst, (*fstats, components, 0, 1, int(reversed_), fstats[2])
