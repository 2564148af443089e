"""The numpy restatement of the pose graph with a 6 x 6 information per edge and a Cauchy loss (velo_graph_add_edges_weighted,
velo_graph_edge_stats, velo_graph_edge_information), on top of tests/pose_graph_ref.py: a subclass of its Problem whose `evaluate`
returns the robustified cost, the whitened and corrected residual and its sparse Jacobian, so that pose_graph_ref.solve runs on it
unmodified.  Test infrastructure only.

For edge e let r be the unweighted residual pose_vec(Z^-1 T_from^-1 T_to) and A, B its Jacobians (pose_graph_ref.edge_eval with
info 1).  W = L L^T is the edge's information, s = |L^T r|^2 = r^T W r, the cost term rho(s) / 2 with rho(s) = s (loss 0) or
b ln(1 + s / b), b = a^2 (Cauchy(a), ceres::CauchyLoss).  Ceres' corrector for rho'' <= 0: residual and Jacobian scaled by
sqrt(rho'), so J^T J = rho' A^T W A and J^T r = rho' A^T W r.

What is deliberately different from the kernels: everything pose_graph_ref.py lists, and the whitening is a matrix product
(L.T @ A) where the kernel sums rows in place.  What is deliberately the SAME: the Cholesky factor is formed by the host's loop
(`chol6`), entry by entry, because s is DEFINED through L and LAPACK's factor differs from that loop's in the last bits."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

import pose_graph_ref as G

IU = np.triu_indices(6)


def chol6(W):
    """W = L L^T, column by column with every sum in ascending k: the loop of the library's host side"""
    W = np.asarray(W, dtype=np.float64)
    L = np.zeros((6, 6))
    for j in range(6):
        dj = W[j, j]
        for k in range(j):
            dj -= L[j, k] * L[j, k]
        if not (dj > 0.0 and np.isfinite(dj)):
            raise np.linalg.LinAlgError("not positive definite")
        L[j, j] = np.sqrt(dj)
        for i in range(j + 1, 6):
            acc = W[i, j]
            for k in range(j):
                acc -= L[i, k] * L[j, k]
            L[i, j] = acc / L[j, j]
    return L


def rho(s, a):
    """(rho(s), rho'(s)): trivial for a == 0, Cauchy(a) otherwise"""
    if a > 0.0:
        b = a * a
        t = 1.0 + s / b
        return b * np.log(t), 1.0 / t
    return s, 1.0


def info21(W):
    return np.asarray(W, dtype=np.float64)[IU]


class Problem(G.Problem):
    def __init__(self, poses, edges, fixed):
        """edges: (from, to, z[6], W, loss_scale); W a positive number (info . I, what the scalar entry stores) or a 6 x 6"""
        super().__init__(poses, [(a, b, z, 1.0) for a, b, z, _, _ in edges], fixed)
        self.L = [np.sqrt(float(W)) * np.eye(6) if np.ndim(W) == 0 else chol6(W) for _, _, _, W, _ in edges]
        self.loss = [float(e[4]) for e in edges]

    def _edge(self, P, e, jac):
        a, b, z, _ = self.edges[e]
        Lt = self.L[e].T
        if jac:
            r, A, B = G.edge_eval(P[a], P[b], z, 1.0)
        else:
            r, A, B = G.edge_eval(P[a], P[b], z, 1.0, False), None, None
        rw = Lt @ r
        s = float(rw @ rw)
        value, w = rho(s, self.loss[e])
        return s, value, w, rw, (Lt @ A if jac else None), (Lt @ B if jac else None)

    def evaluate(self, x, jac=True):
        """cost = sum rho(s) / 2, the corrected residual sqrt(rho') L^T r [6 E] and its sparse Jacobian [6 E, N]"""
        P = self.poses_of(x)
        r = np.zeros(6 * self.n_edges)
        cost = 0.0
        rows, cols, vals = [], [], []
        base = np.repeat(np.arange(6), 6), np.tile(np.arange(6), 6)
        for e, (a, b, _, _) in enumerate(self.edges):
            _, value, w, rw, A, B = self._edge(P, e, jac)
            cost += 0.5 * value
            c = np.sqrt(w)
            r[6 * e:6 * e + 6] = c * rw
            if jac:
                for node, M in ((a, A), (b, B)):
                    if node in self.slot:
                        rows.append(6 * e + base[0]); cols.append(6 * self.slot[node] + base[1]); vals.append((c * M).ravel())
        if not jac:
            return cost, r
        if rows:
            J = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(6 * self.n_edges, self.N))
        else:
            J = sp.csr_matrix((6 * self.n_edges, self.N))
        return cost, r, J

    def edge_stats(self, x=None):
        """(chi2 [E], weight [E]) at x (default: the stored state): s and rho'(s)"""
        P = self.poses_of(self.x0() if x is None else x)
        out = [self._edge(P, e, False) for e in range(self.n_edges)]
        return np.array([o[0] for o in out]), np.array([o[2] for o in out])


def edge_information(z, H):
    """W = Bz^-T ((H + H^T) / 2) Bz^-1, Bz = blockdiag(Rz^T J_l(w_z), Rz^T): the Jacobian of pose_vec(Z^-1 X) in x at x = z"""
    z = np.asarray(z, dtype=np.float64)
    H = np.asarray(H, dtype=np.float64).reshape(6, 6)
    Rz = G.rot(z[:3])
    Bz = np.zeros((6, 6))
    Bz[:3, :3] = Rz.T @ G.left_jacobian(z[:3])
    Bz[3:, 3:] = Rz.T
    Bi = np.linalg.inv(Bz)
    return Bi.T @ (0.5 * (H + H.T)) @ Bi


def spd(rng, lo=1.0, cond=1e3):
    """a symmetric positive definite 6 x 6 of eigenvalues lo .. lo cond in a random orientation"""
    Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
    W = (Q * (lo * np.logspace(0.0, np.log10(cond), 6))) @ Q.T
    return 0.5 * (W + W.T)


NOISE_INFO = np.diag([1.0 / 2e-3 ** 2] * 3 + [1.0 / 0.02 ** 2] * 3)      # chain_graph's rot_sigma and trans_sigma
OUTLIERS = ((5, 40), (12, 55), (20, 63))
CAUCHY = 2.0


def _ring70_outliers(loss):
    g = G.chain_graph(403, 70, (1, 2, 3, 4), loops=[(69, 0, 1000.0)], ring=True)
    rng = np.random.default_rng(4231)
    edges = []
    for a, b, z, _ in g["edges"]:
        closing = abs(a - b) > 4                                     # measured with a tenth of the noise
        edges.append((a, b, z, (100.0 if closing else 1.0) * NOISE_INFO, loss if closing else 0.0))
    for a, b in OUTLIERS:                                             # gross: 2.7 .. 4.3 m and 0.2 rad off, an information of its own
        z = G.relative(g["truth"][a], g["truth"][b])
        d = rng.normal(size=3)
        z[3:] += rng.uniform(2.7, 4.3) * d / np.linalg.norm(d)
        d = rng.normal(size=3)
        z[:3] += 0.2 * d / np.linalg.norm(d)
        Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
        W = Q @ NOISE_INFO @ Q.T
        edges.append((a, b, z, 0.5 * (W + W.T), loss))
    order = np.random.default_rng(4232).permutation(len(edges))
    g["edges"] = [edges[i] for i in order]
    g["outliers"] = [int(np.flatnonzero(order == len(edges) - 3 + k)[0]) for k in range(3)]
    g["split"], g["edge_capacity"] = 97, 128                         # the second call grows the arrays with the weighted columns present
    return g


def fixture(name):
    """dict(poses, edges (from, to, z, W, loss), fixed, ...).  An edge whose W is a number goes through the scalar entry
    (velo_graph_add_edges), every other one through velo_graph_add_edges_weighted; consecutive edges of one kind share a call."""
    if name == "pair_w":                                     # ends at T_0 . Z and cost 0 whatever W is
        g = G.fixture("pair")
        g["edges"] = [(a, b, z, spd(np.random.default_rng(4211)), 0.0) for a, b, z, _ in g["edges"]]
        return g
    if name == "chain5_w":                                   # every edge its own W, trivial loss
        g = G.fixture("chain5")
        rng = np.random.default_rng(4212)
        g["edges"] = [(a, b, z, spd(rng), 0.0) for a, b, z, _ in g["edges"]]
        return g
    if name == "chain5_scalar":                              # chain5 through the weighted entry: W = info . I, trivial loss
        g = G.fixture("chain5")
        g["edges"] = [(a, b, z, info * np.eye(6), 0.0) for a, b, z, info in g["edges"]]
        return g
    if name == "chain5_mixed":                               # scalar odometry first, then the contradicting loop edge with Cauchy
        g = G.fixture("chain5")
        rng = np.random.default_rng(4213)
        g["edges"] = [(a, b, z, info, 0.0) for a, b, z, info in g["edges"][:-1]] + [g["edges"][-1][:3] + (spd(rng, 0.01), CHAIN5_MIXED_A)]
        return g
    if name == "ring70_outliers":
        return _ring70_outliers(CAUCHY)
    if name == "ring70_outliers_trivial":
        return _ring70_outliers(0.0)
    raise KeyError(name)


# The loop edge of chain5_mixed: information of eigenvalues 0.01 .. 10 against the odometry's 1, so that neither side wins outright, and
# Cauchy(0.2), with which the edge's weight is 0.23 at the start and 0.84 at the end on this restatement (strictly inside 0.05 .. 0.95)
CHAIN5_MIXED_A = 0.2
FIXTURES = ("pair_w", "chain5_w", "chain5_mixed", "ring70_outliers", "ring70_outliers_trivial")


def problem_of(g):
    return Problem(g["poses"], g["edges"], g["fixed"])


def position_error(g, poses):
    """the largest distance of a node's position from the truth"""
    return max(float(np.linalg.norm(np.asarray(poses[f])[3:] - g["truth"][f][3:])) for f in poses)
