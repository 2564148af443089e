"""The graphs of the envelope solver's tests beyond pose_graph_ref.FIXTURES, chosen for where its factorisation can go wrong; all
seeded, each small enough for the restatement's dense `direct` solve.  Test infrastructure only.

  chain250        250 nodes, dframe 1..2, one closing loop edge (130, 247) between free nodes: many elimination steps, an envelope that
                  widens at the closure, a `first` that is not monotone
  chain250_split  the same chain with frames 125 and 126 fixed as well: a dframe-2 edge bridges ONE fixed frame, so it takes two adjacent
                  ones to cut the chain; two components (1..124 and 127..249), one of them ordered after the other's end
  lap454          454 poses on a circle of 300 frames, dframe 1..4, loop edges by lap_edges' integer rule, a dead-reckoned start
  free1, free2    one and two free nodes
"""
import numpy as np

import pose_graph_ref as G

ENV_FIXTURES = ("chain250", "chain250_split", "lap454", "free1", "free2")
LAP_N, LAP = 454, 300


def lap_edges(n=LAP_N, lap=LAP, dframes=(1, 2, 3, 4)):
    """(odometry, loops): (i, i + d) for every d; (i - k, i) for k = 100, 110, ... whenever (i - k) mod lap and i mod lap are
    within 12 on the circle"""
    odometry = [(i, i + d) for d in dframes for i in range(n - d)]
    loops = []
    for i in range(n):
        for k in range(100, i + 1, 10):
            gap = abs((i - k) % lap - i % lap)
            if min(gap, lap - gap) <= 12:
                loops.append((i - k, i))
    return odometry, loops


def lap_graph(seed=454):
    rng = np.random.default_rng(seed)
    radius = LAP * 0.8 / (2.0 * np.pi)
    truth = []
    for i in range(LAP_N):                                         # heading about the camera's y axis, forward along its z
        a = 2.0 * np.pi * i / LAP
        T = G.pose_mat(np.array([0.0, a, 0.0, radius * (1.0 - np.cos(a)), 0.0, radius * np.sin(a)]))
        truth.append(G.pose_vec(T @ G.pose_mat(np.concatenate([5e-3 * rng.normal(size=3), 0.1 * rng.normal(size=3)]))))
    odometry, loops = lap_edges()
    edges = [(a, b, G._noisy(rng, G.relative(truth[a], truth[b]), 1e-3, 0.02), 1.0) for a, b in odometry]
    edges += [(a, b, G._noisy(rng, G.relative(truth[a], truth[b]), 1e-4, 0.002), 1.0) for a, b in loops]
    poses = G._dead_reckoning(truth[0], [e[2] for e in edges[:LAP_N - 1]])
    return dict(poses={i: p for i, p in enumerate(poses)}, edges=edges, fixed=[0], truth=truth)


def fixture(name):
    if name in ("chain250", "chain250_split"):
        g = G.chain_graph(411, 250, (1, 2), loops=[(130, 247, 1.0)])
        if name == "chain250_split":
            g["fixed"] = [0, 125, 126]
        return g
    if name == "lap454":
        return lap_graph()
    if name in ("free1", "free2"):
        g = G.chain_graph(412, 3, (1, 2))
        if name == "free1":                                           # the dead reckoning satisfies both edges of node 1: move it off them
            g["fixed"] = [0, 2]
            g["poses"][1] = g["poses"][1] + np.array([0.02, -0.01, 0.015, 0.1, -0.05, 0.08])
        return g
    raise KeyError(name)


def free_graph(g):
    """what velo_graph_optimize hands to velo_graph_order: (n_free, a, b) over the free nodes in ascending frame order, the edges that
    touch a fixed node dropped"""
    prob = G.problem_of(g)
    pairs = [(prob.slot[a], prob.slot[b]) for a, b, _, _ in g["edges"] if a in prob.slot and b in prob.slot]
    return prob.n_free, [p[0] for p in pairs], [p[1] for p in pairs]
