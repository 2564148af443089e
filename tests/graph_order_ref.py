"""A pure-Python restatement of velo_graph_order's rule (include/velo_hip.h), written from its text -- NOT from the library's
code -- so that the library's order has something independent to equal.  Test infrastructure only.

The rule: degree = the number of distinct neighbours; components in ascending order of their smallest node; the start node of a
component is George-Liu's pseudo-peripheral node (begin at the node of least degree, lowest index on a tie; build the breadth-first
level structure; take from its last level the node of least degree, lowest index on a tie; go on from that node while the number
of levels strictly grows); Cuthill-McKee appends a dequeued node's unvisited neighbours in ascending (degree, index); the sequence of
all components is reversed as a whole.  first[k] is the smallest position among k and its neighbours; stats = (widest row, envelope
blocks sum (w + 1), work sum w (w + 1) / 2, components), w = k - first[k]."""
import numpy as np


def neighbours(n, a, b):
    nb = [set() for _ in range(n)]
    for u, v in zip(a, b):
        nb[int(u)].add(int(v))
        nb[int(v)].add(int(u))
    return [sorted(s) for s in nb]


def level_structure(nb, root):
    levels, seen = [[root]], {root}
    while True:
        nxt = []
        for u in levels[-1]:
            for v in nb[u]:
                if v not in seen:
                    seen.add(v)
                    nxt.append(v)
        if not nxt:
            return levels
        levels.append(nxt)


def stats_of(nb, perm):
    """first and stats from a permutation, by definition"""
    n = len(perm)
    pos = np.empty(n, dtype=np.int64)
    pos[np.asarray(perm, dtype=np.int64)] = np.arange(n)
    first = np.array([min([k] + [int(pos[v]) for v in nb[int(perm[k])]]) for k in range(n)], dtype=np.int64)
    w = np.arange(n) - first
    return first, (int(w.max()) if n else 0, int((w + 1).sum()), int((w * (w + 1) // 2).sum()))


def order(n, a, b):
    """(perm, first, stats[4]) of the graph on nodes 0 .. n - 1 with the edges (a[e], b[e])"""
    nb = neighbours(n, a, b)
    deg = [len(x) for x in nb]
    key = lambda v: (deg[v], v)                               # noqa: E731
    placed, sequence, components = [False] * n, [], 0
    for s in range(n):
        if placed[s]:
            continue
        components += 1
        members = [v for level in level_structure(nb, s) for v in level]
        root = min(members, key=key)
        levels = level_structure(nb, root)
        while True:
            far = min(levels[-1], key=key)
            far_levels = level_structure(nb, far)
            if len(far_levels) <= len(levels):
                break
            root, levels = far, far_levels
        queue, head = [root], 0
        placed[root] = True
        while head < len(queue):
            u = queue[head]
            head += 1
            fresh = sorted((v for v in nb[u] if not placed[v]), key=key)
            for v in fresh:
                placed[v] = True
            queue.extend(fresh)
        sequence.extend(queue)
    perm = np.array(sequence[::-1], dtype=np.int64)
    first, (widest, blocks, work) = stats_of(nb, perm)
    return perm, first, (widest, blocks, work, components)
