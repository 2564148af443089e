"""A numpy restatement of velo_graph_covariance (include/velo_hip.h) over pose_graph_ref.Problem / pose_graph_weighted_ref.Problem:
H = J^T J from the dense J of `evaluate(x)`, and Sigma = H^-1 by three routes that share nothing but J:

  inverse    np.linalg.inv(H)
  qr         the R of np.linalg.qr(J): Sigma = R^-1 R^-T, which never forms H
  takahashi  the Jacobi-scaled H in graph_order_ref.order's order, its Cholesky factor, and the Takahashi recursion over the block
             envelope: Z(i,j) = -(sum_{k in S_j} Z(i,k) L(k,j)) L(j,j)^-1, Z(j,j) = (L(j,j)^-T - sum_k Z(k,j)^T L(k,j)) L(j,j)^-1 with
             S_j = { i > j : first(i) <= j }, columns descending.  Only blocks inside the envelope exist; a read outside is counted.

Test infrastructure only.  What is deliberately different from the kernels: the factor comes from LAPACK on the dense matrix, the
sums are matrix products, and the other two routes do not know the order at all."""
from __future__ import annotations

import numpy as np
import scipy.linalg as sla

import graph_order_ref as O
import pose_graph_env_fixtures as F
import pose_graph_ref as G
import pose_graph_weighted_ref as W

# the graphs of the covariance tests and what each is there for (tests/test_gpu_pose_graph_covariance.py)
FIXTURES = ("free1", "free2", "chain5", "large_rotation", "ring70", "chain250", "chain250_split", "lap454", "hub140", "ring70_outliers",
            "chain5_mixed")


def fixture(name):
    """(graph, problem): `hub140` is pose_graph_ref's hub with its edgeless frame 140 fixed as well"""
    if name in ("ring70_outliers", "chain5_mixed"):
        g = W.fixture(name)
        return g, W.problem_of(g)
    if name == "hub140":
        g = G.fixture("hub")
        g["fixed"] = [1, 2, 140]
    elif name in F.ENV_FIXTURES:
        g = F.fixture(name)
    else:
        g = G.fixture(name)
    return g, G.problem_of(g)


def free_edges(g, prob):
    """(a, b) in free indices of the edges between two free nodes: what the library hands to velo_graph_order"""
    pairs = [(prob.slot[e[0]], prob.slot[e[1]]) for e in g["edges"] if e[0] in prob.slot and e[1] in prob.slot]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def dense_jacobian(prob, x=None):
    return prob.evaluate(prob.x0() if x is None else x)[2].toarray()


def by_inverse(J):
    return np.linalg.inv(J.T @ J)


def by_qr(J):
    R = np.linalg.qr(J, mode="r")
    Ri = sla.solve_triangular(R, np.eye(R.shape[0]), lower=False)
    return Ri @ Ri.T


class Takahashi:
    """the selected inverse of the scaled H in the envelope order; block(a, b) is Sigma_ab for free indices a, b inside the envelope"""

    def __init__(self, J, n_free, ea, eb):
        H = J.T @ J
        self.n = n = n_free
        self.c = 1.0 / (1.0 + np.sqrt(np.diag(H)))                     # the library's Jacobi scaling
        perm, first, stats = O.order(n, ea, eb)
        self.perm, self.first, self.stats = perm, first, stats
        self.pos = np.empty(n, dtype=np.int64)
        self.pos[perm] = np.arange(n)
        idx = (6 * perm[:, None] + np.arange(6)[None, :]).ravel()
        Hs = (H * self.c[:, None] * self.c[None, :])[np.ix_(idx, idx)]
        L = np.linalg.cholesky(Hs)
        blk = lambda M, i, j: M[6 * i:6 * i + 6, 6 * j:6 * j + 6]       # noqa: E731
        self.outside_reads = 0
        Z = {}

        def read(i, k):                                                # Z(i,k) from the lower triangle
            hi, lo = max(i, k), min(i, k)
            if first[hi] > lo:
                self.outside_reads += 1
                return np.zeros((6, 6))
            return Z[(hi, lo)] if i >= k else Z[(hi, lo)].T

        rows_of = [[] for _ in range(n)]                               # S_j
        for i in range(n):
            for j in range(int(first[i]), i):
                rows_of[j].append(i)
        for j in range(n - 1, -1, -1):
            S = rows_of[j]
            Li = sla.solve_triangular(blk(L, j, j), np.eye(6), lower=True)
            for i in S:
                acc = np.zeros((6, 6))
                for k in S:
                    acc += read(i, k) @ blk(L, k, j)
                Z[(i, j)] = -acc @ Li
            acc = Li.T.copy()
            for k in S:
                acc -= Z[(k, j)].T @ blk(L, k, j)
            D = acc @ Li
            Z[(j, j)] = 0.5 * (D + D.T)
        self.Z = Z

    def inside(self, a, b):
        hi, lo = max(self.pos[a], self.pos[b]), min(self.pos[a], self.pos[b])
        return self.first[hi] <= lo

    def block(self, a, b):
        pa, pb = int(self.pos[a]), int(self.pos[b])
        Zb = self.Z[(pa, pb)] if pa >= pb else self.Z[(pb, pa)].T
        return Zb * self.c[6 * a:6 * a + 6, None] * self.c[None, 6 * b:6 * b + 6]


def cov_spread(A, B, sigma_a, sigma_b):
    """max |A_ij - B_ij| / (sigma_i sigma_j) over one 6 x 6 block; sigma: the standard deviations of route `inverse`"""
    return float(np.max(np.abs(A - B) / (sigma_a[:, None] * sigma_b[None, :])))


def block_of(S, a, b):
    return S[6 * a:6 * a + 6, 6 * b:6 * b + 6]


def outside_pairs(perm, first, count=3):
    """up to `count` pairs (a, b) of free indices outside the envelope of the order (perm, first): from the last rows that leave
    columns out, the column 0, the one just before the row's first, and the middle one; the second pair with the earlier node first.
    Fewer (or none) where the envelope is full."""
    out = []
    for hi in range(len(perm) - 1, 0, -1):
        f = int(first[hi])
        if f == 0 or len(out) >= count:
            continue
        lo = (0, f - 1, f // 2)[len(out)]
        pair = (int(perm[hi]), int(perm[lo]))
        out.append(pair[::-1] if len(out) == 1 else pair)
    return out
