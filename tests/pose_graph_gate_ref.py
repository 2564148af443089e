"""A numpy restatement of velo_graph_edge_gate and velo_graph_loop_candidates (include/velo_hip.h) on top of the restatements that exist:
Sigma = (J^T J)^-1 from pose_graph_cov_ref.by_inverse / by_qr, and r, A, B of a pair from pose_graph_ref.edge_eval(..., info=1).  For a
pair (a, b) with measurement z and information W:

    rel        pose_vec(T_a^-1 T_b)                       z = rel where none is given
    Sigma_rel  A S_aa A^T + A S_ab B^T + B S_ba A^T + B S_bb B^T      (the S blocks zero for a fixed frame)
    S          Sigma_rel + W^-1                           (Sigma_rel without W)
    chi2       r^T S^-1 r through numpy's Cholesky factor; -1 where S is not positive definite

and for the candidates of a query q: dist_i = |t(T_i^-1 T_q)|, sigma_i = sqrt(trace(Sigma_rel(i, q)[3:, 3:])) at z = rel, selected when
dist <= radius + k_sigma sigma.  Test infrastructure only.  What is deliberately different from the kernels: everything
pose_graph_ref.py and pose_graph_cov_ref.py list, Sigma is the dense inverse (no envelope, no column solves), the products are matrix
products and W^-1 is np.linalg.inv.

Three graphs beyond those of the covariance tests:
  chain12_tree   12 nodes, dframe 1 only, a random SPD W of condition 1e3 per edge: on a tree Sigma_rel across an edge is W_e^-1
  ring70_open    ring70_outliers_trivial with its |from - to| > 4 edges HELD BACK: the true closing edge (69, 0) and three gross outliers
  lap454_open    lap454's odometry with W = diag(1e6 x3, 2500 x3), the inverse covariance of its noise; its 462 loop measurements held
                 back, with diag(1e8 x3, 2.5e5 x3)
"""
from __future__ import annotations

import numpy as np

import pose_graph_cov_ref as R
import pose_graph_env_fixtures as F
import pose_graph_ref as G
import pose_graph_weighted_ref as W

OPEN_FIXTURES = ("chain12_tree", "ring70_open", "lap454_open")
LAP_ODO_INFO = np.diag([1e6] * 3 + [2500.0] * 3)               # lap_graph's odometry noise: 1e-3 rad, 0.02 m
LAP_LOOP_INFO = np.diag([1e8] * 3 + [2.5e5] * 3)               # its loop noise: 1e-4 rad, 0.002 m


def fixture(name):
    """(graph, problem); the open graphs carry `held`: the edges (from, to, z, W) kept out of the graph"""
    if name == "chain12_tree":
        g = G.chain_graph(5, 12, (1,))
        rng = np.random.default_rng(5012)
        g["edges"] = [(a, b, z, W.spd(rng, 50.0, 1e3), 0.0) for a, b, z, _ in g["edges"]]
        g["held"] = []
        return g, W.problem_of(g)
    if name == "ring70_open":
        g = W.fixture("ring70_outliers_trivial")
        far = [abs(e[0] - e[1]) > 4 for e in g["edges"]]
        g["held"] = [e[:4] for e, f in zip(g["edges"], far) if f]
        g["edges"] = [e for e, f in zip(g["edges"], far) if not f]
        g["true_held"] = [k for k, e in enumerate(g["held"]) if (e[0], e[1]) == (69, 0)]
        for key in ("split", "edge_capacity", "outliers"):
            g.pop(key, None)
        return g, W.problem_of(g)
    if name == "lap454_open":
        g = F.lap_graph()
        n_odo = len(F.lap_edges()[0])
        g["held"] = [(a, b, z, LAP_LOOP_INFO) for a, b, z, _ in g["edges"][n_odo:]]
        g["edges"] = [(a, b, z, LAP_ODO_INFO, 0.0) for a, b, z, _ in g["edges"][:n_odo]]
        return g, W.problem_of(g)
    return R.fixture(name)


def at_poses(g, prob, poses):
    """the problem of g at other poses: {frame: pose6}"""
    return type(prob)(poses, g["edges"], g["fixed"])


def block(S, prob, a, b):
    """Sigma_ab for FRAMES a, b; zero where one of them is fixed"""
    if a not in prob.slot or b not in prob.slot:
        return np.zeros((6, 6))
    return R.block_of(S, prob.slot[a], prob.slot[b])


def relative(xa, xb):
    """pose_vec(T_a^-1 T_b) with pose_graph_ref's own rotation and logarithm"""
    Ra = G.rot(np.asarray(xa[:3], dtype=np.float64))
    return np.concatenate([G.log_rot(Ra.T @ G.rot(np.asarray(xb[:3], dtype=np.float64))), Ra.T @ (np.asarray(xb[3:]) - np.asarray(xa[3:]))])


def pair_terms(poses, a, b, z=None):
    """(rel, z, r, A, B) of the pair (a, b) at `poses`"""
    rel = relative(poses[a], poses[b])
    zp = rel if z is None else np.asarray(z, dtype=np.float64)
    r, A, B = G.edge_eval(np.asarray(poses[a]), np.asarray(poses[b]), zp, 1.0)
    return rel, zp, r, A, B


def sigma_rel(S, prob, a, b, A, B):
    Saa, Sab, Sbb = block(S, prob, a, a), block(S, prob, a, b), block(S, prob, b, b)
    return A @ Saa @ A.T + A @ Sab @ B.T + B @ Sab.T @ A.T + B @ Sbb @ B.T


def chi2_of(S, r):
    try:
        L = np.linalg.cholesky(S)
    except np.linalg.LinAlgError:
        return -1.0
    y = np.linalg.solve(L, r)
    return float(y @ y)


def gate(S, prob, poses, frm, to, z=None, info=None):
    """what velo_graph_edge_gate returns: (rel [n, 6], r [n, 6], S [n, 6, 6], chi2 [n]) with Sigma = S of `prob` at `poses`"""
    n = len(frm)
    rel, res, cov, chi2 = np.zeros((n, 6)), np.zeros((n, 6)), np.zeros((n, 6, 6)), np.zeros(n)
    for p, (a, b) in enumerate(zip(frm, to)):
        rel[p], _, res[p], A, B = pair_terms(poses, int(a), int(b), None if z is None else z[p])
        cov[p] = sigma_rel(S, prob, int(a), int(b), A, B)
        if info is not None:
            cov[p] = cov[p] + np.linalg.inv(np.asarray(info[p], dtype=np.float64))
        chi2[p] = chi2_of(cov[p], res[p])
    return rel, res, cov, chi2


def candidates(S, prob, poses, query, min_gap, radius, k_sigma):
    """(frames, dist, sigma, margin): the considered frames ascending with their distance and sigma (0 for k_sigma == 0), and per frame
    |dist - threshold| / threshold -- how far the frame is from changing sides"""
    frames, dist, sigma = [], [], []
    for i in sorted(poses):
        if abs(i - query) < min_gap:
            continue
        rel, _, _, A, B = pair_terms(poses, i, query)
        frames.append(i)
        dist.append(float(np.linalg.norm(rel[3:])))
        sigma.append(float(np.sqrt(max(np.trace(sigma_rel(S, prob, i, query, A, B)[3:, 3:]), 0.0))) if k_sigma > 0.0 else 0.0)
    frames, dist, sigma = np.asarray(frames), np.asarray(dist), np.asarray(sigma)
    thresh = radius + k_sigma * sigma
    return frames, dist, sigma, np.abs(dist - thresh) / np.maximum(thresh, 1e-300)


def rel_spread(A, B):
    """max |A_ij - B_ij| / (sigma_i sigma_j) over one 6 x 6, sigma from A's diagonal"""
    s = np.sqrt(np.diag(A))
    return float(np.max(np.abs(A - B) / np.outer(s, s)))


def tested_pairs(name, g, prob, outside=None):
    """(from, to, z | None, info | None): the pairs both test files ask for on graph `name`.  Every edge of the graph in the tangent at
    its own z, then -- where the graph holds edges back -- those with their z, then pairs measured by the relative pose of the graph's
    LOADED state: the fixed frames against the last frame, `outside` (pairs outside the envelope; default: by the restatement of the
    order) in both directions, and what the graph is there for."""
    frames = sorted(g["poses"])
    frm, to = [e[0] for e in g["edges"]], [e[1] for e in g["edges"]]
    z = [np.asarray(e[2], dtype=np.float64) for e in g["edges"]]
    frm += [e[0] for e in g.get("held", [])]
    to += [e[1] for e in g.get("held", [])]
    z += [np.asarray(e[2], dtype=np.float64) for e in g.get("held", [])]
    extra = [(f, frames[-1]) for f in g["fixed"] if f != frames[-1]]
    outside = outside_frames(g, prob) if outside is None else list(outside)
    extra += outside + [(b, a) for a, b in outside]
    if name == "chain250_split":
        extra += [(100, 200), (200, 100), (125, 126)]                  # across the components; both ends fixed
    if name == "free1":
        extra += [(0, 2)]                                              # both ends fixed
    if name == "hub140":
        extra += [(5, 77), (77, 0), (130, 3)]
    frm += [p[0] for p in extra]
    to += [p[1] for p in extra]
    rel = [relative(g["poses"][a], g["poses"][b]) for a, b in extra]
    return frm, to, np.array(z + rel).reshape(-1, 6), None


def outside_frames(g, prob, count=3):
    """pairs of FRAMES outside the envelope of the library's order, by pose_graph_cov_ref.outside_pairs"""
    import graph_order_ref as O
    ea, eb = R.free_edges(g, prob)
    perm, first, _ = O.order(prob.n_free, ea, eb)
    return [(prob.free[a], prob.free[b]) for a, b in R.outside_pairs(perm, first, count)]
