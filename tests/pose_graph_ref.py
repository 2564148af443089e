"""A numpy restatement of the batch pose-graph optimisation (velo_graph_*), written from the reference's statement of the problem
(main.cpp:190-204 the prior, main.cpp:516-536 the Pose3d_Pose3d factors, main.cpp:416-424 the form of the residual) and from
SURVEY.md Appendix B1 -- NOT from the kernels -- so that velo_graph_optimize has something independent to be compared with.  Test
infrastructure only.

A node is the 6 doubles (angle-axis, translation) of a frame's world pose T; an edge (from, to, z, info) states T_to = T_from Z and
its residual is sqrt(info) * pose_vec(Z^-1 T_from^-1 T_to): the angle-axis of the rotation, then the translation.  Fixed nodes are
constants.  The unknowns are the free nodes that have a pose, in ascending frame order; a free node no edge touches is an unknown
with an empty column block.

What is deliberately different from the kernels:
  * derivatives: the closed forms of the SO(3) Jacobians (J_l(w) = I + (1 - cos) / t^2 K + (t - sin) / t^3 K^2 and the inverse right
    Jacobian of the residual's angle-axis); the kernels take J_l from the dual-number rotation of velo_device_math.h;
  * the logarithm: atan2(|vee(R - R^T)| / 2, (tr R - 1) / 2) on the matrix, the kernels go through the quaternion as Ceres does;
  * the linear algebra: one sparse Jacobian, J^T J formed as a matrix product, and either a direct solve of the damped normal
    equations (`direct`: dense below 3,000 unknowns, SuperLU above) or the same block-Jacobi preconditioned CG as the kernels, written
    on whole vectors (`pcg`); the model change row by row, -(J s).(r + J s / 2).
"""
from __future__ import annotations

import time

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from ba_ref import (ACCEPTED, DBL_MIN, EPS, FUNCTION, GRADIENT, INVALID, LM_DEFAULTS, PARAMETER, REJECTED, STATUS_NAMES,  # noqa: F401
                    T_FAILURE, T_MAX_ITERATIONS, T_RADIUS, closest_margin, skew)

CG_DEFAULTS = dict(cg_tol=1e-10, cg_max=2000)            # velo_default_graph_params


def rot(w):
    """AngleAxisToRotationMatrix: Rodrigues above theta^2 = DBL_EPSILON, first order below"""
    t2 = float(w @ w)
    K = skew(w)
    if t2 > EPS:
        t = np.sqrt(t2)
        return np.eye(3) + (np.sin(t) / t) * K + ((1.0 - np.cos(t)) / t2) * (K @ K)
    return np.eye(3) + K


def left_jacobian(w):
    """R(w + d) = Exp(J_l(w) d) R(w) to first order"""
    t2 = float(w @ w)
    K = skew(w)
    if t2 > EPS:
        t = np.sqrt(t2)
        return np.eye(3) + ((1.0 - np.cos(t)) / t2) * K + ((t - np.sin(t)) / (t2 * t)) * (K @ K)
    return np.eye(3) + 0.5 * K


def log_rot(R):
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = float(np.linalg.norm(v)), 0.5 * (np.trace(R) - 1.0)
    if s > 1e-12:
        return v * (np.arctan2(s, c) / s)
    return v


def right_jacobian_inverse(phi):
    """Log(R Exp(e)) = phi + J_r^-1(phi) e to first order"""
    t2 = float(phi @ phi)
    K = skew(phi)
    if t2 > 1e-6:
        t = np.sqrt(t2)
        coef = 1.0 / t2 - np.cos(0.5 * t) / (2.0 * t * np.sin(0.5 * t))
    else:
        coef = 1.0 / 12.0 + t2 / 720.0
    return np.eye(3) + 0.5 * K + coef * (K @ K)


def edge_eval(xf, xt, z, info, jac=True):
    """the residual [6] of one edge and its Jacobians [6, 6] with respect to the `from` and the `to` node"""
    Rf, Rt, Rz = rot(xf[:3]), rot(xt[:3]), rot(z[:3])
    d = xt[3:] - xf[3:]
    Q = Rz.T @ Rf.T
    phi = log_rot(Q @ Rt)
    s = np.sqrt(info)
    r = s * np.concatenate([phi, Q @ d - Rz.T @ z[3:]])
    if not jac:
        return r
    Ji = right_jacobian_inverse(phi)
    Jlf, Jlt = left_jacobian(xf[:3]), left_jacobian(xt[:3])
    A, B = np.zeros((6, 6)), np.zeros((6, 6))
    A[:3, :3] = -Ji @ Rt.T @ Jlf
    A[3:, :3] = Q @ skew(d) @ Jlf
    A[3:, 3:] = -Q
    B[:3, :3] = Ji @ Rt.T @ Jlt                              # J_r(w) = R(w)^T J_l(w)
    B[3:, 3:] = Q
    return r, s * A, s * B


class Problem:
    def __init__(self, poses, edges, fixed):
        """poses: {frame: pose6}; edges: list of (from, to, z[6], info); fixed: frames that are constants"""
        self.poses0 = {int(f): np.asarray(p, dtype=np.float64).copy() for f, p in poses.items()}
        self.edges = [(int(a), int(b), np.asarray(z, dtype=np.float64), float(i)) for a, b, z, i in edges]
        self.fixed = sorted(set(int(f) for f in fixed))
        self.free = [f for f in sorted(self.poses0) if f not in self.fixed]
        self.slot = {f: k for k, f in enumerate(self.free)}
        self.n_nodes, self.n_free, self.n_edges = len(self.poses0), len(self.free), len(self.edges)
        self.N = 6 * self.n_free

    def x0(self):
        return np.concatenate([self.poses0[f] for f in self.free]) if self.free else np.zeros(0)

    def poses_of(self, x):
        P = dict(self.poses0)
        for k, f in enumerate(self.free):
            P[f] = x[6 * k:6 * k + 6]
        return P

    def evaluate(self, x, jac=True):
        """cost = sum |r|^2 / 2, r [6 E] and the sparse Jacobian [6 E, N], edges in the order they were added"""
        P = self.poses_of(x)
        r = np.zeros(6 * self.n_edges)
        rows, cols, vals = [], [], []
        base = np.repeat(np.arange(6), 6), np.tile(np.arange(6), 6)
        for e, (a, b, z, info) in enumerate(self.edges):
            if not jac:
                r[6 * e:6 * e + 6] = edge_eval(P[a], P[b], z, info, False)
                continue
            r[6 * e:6 * e + 6], A, B = edge_eval(P[a], P[b], z, info)
            for node, M in ((a, A), (b, B)):
                if node in self.slot:
                    rows.append(6 * e + base[0]); cols.append(6 * self.slot[node] + base[1]); vals.append(M.ravel())
        cost = 0.5 * float(r @ r)
        if not jac:
            return cost, r
        if rows:
            J = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(6 * self.n_edges, self.N))
        else:
            J = sp.csr_matrix((6 * self.n_edges, self.N))
        return cost, r, J

    def system(self, x=None):
        """cost, J^T r [N] and the diagonal blocks of J^T J [n_free, 6, 6] at x (default: the stored state)"""
        cost, r, J = self.evaluate(self.x0() if x is None else x)
        H = (J.T @ J).toarray()
        return cost, J.T @ r, np.array([H[6 * k:6 * k + 6, 6 * k:6 * k + 6] for k in range(self.n_free)]).reshape(-1, 6, 6)


def step_direct(A, b, o):
    if A.shape[0] <= 3000:
        return np.linalg.solve(A.toarray(), b), 0, 0.0
    return spla.spsolve(A.tocsc(), b), 0, 0.0


def step_pcg(A, b, o):
    """block-Jacobi preconditioned CG from y = 0: stops before iteration k when rho_k <= tol^2 rho_0, rho = r^T M^-1 r, or at the cap"""
    n = A.shape[0] // 6
    Ad = A.toarray() if A.shape[0] <= 3000 else None
    chol = [np.linalg.cholesky(Ad[6 * i:6 * i + 6, 6 * i:6 * i + 6] if Ad is not None else A[6 * i:6 * i + 6, 6 * i:6 * i + 6].toarray()) for i in range(n)]

    def precondition(v):
        out = np.empty_like(v)
        for i in range(n):
            L = chol[i]
            out[6 * i:6 * i + 6] = np.linalg.solve(L.T, np.linalg.solve(L, v[6 * i:6 * i + 6]))
        return out
    y, r = np.zeros_like(b), b.copy()
    z = precondition(r)
    rho0 = rho = float(r @ z)
    p = np.zeros_like(b)
    rho_prev, k = 1.0, 0
    while k < o["cg_max"]:
        if rho <= o["cg_tol"] ** 2 * rho0:
            break
        p = z + ((rho / rho_prev) if k > 0 else 0.0) * p
        q = A @ p
        sigma = float(p @ q)
        if not (sigma > 0.0 and np.isfinite(sigma)):
            raise np.linalg.LinAlgError("CG broke down")
        alpha = rho / sigma
        y += alpha * p
        r -= alpha * q
        z = precondition(r)
        rho_prev, rho = rho, float(r @ z)
        k += 1
    return y, k, (np.sqrt(rho / rho0) if rho0 > 0.0 else 0.0)


def solve(prob, linear="pcg", **kw):
    """SURVEY.md Appendix B1 over the free nodes.  Returns dict(x, termination, trace, iterations, evaluations, initial_cost,
    final_cost); trace = one dict per iteration with status, cost, candidate_cost, radius, model_change, step_norm, cg_iterations,
    cg_residual and the margins of every decision taken."""
    o = dict(LM_DEFAULTS)
    o.update(CG_DEFAULTS)
    o.update(kw)
    stepper = step_pcg if linear == "pcg" else step_direct
    x = prob.x0()
    cost, r, J = prob.evaluate(x)
    out = dict(initial_cost=cost, evaluations=1, iterations=0, trace=[], linear_seconds=0.0)      # linear_seconds: inside the linear solver

    def done(label):
        out.update(x=x, termination=label, final_cost=cost)
        return out
    g = J.T @ r
    if prob.N == 0 or np.max(np.abs(g)) <= o["g_tol"]:
        return done("gradient")
    c = 1.0 / (1.0 + np.sqrt(np.asarray(J.multiply(J).sum(axis=0)).ravel()))     # Jacobi scaling, ONCE
    mu, nu, bad = o["radius0"], 2.0, 0
    d = None
    k = 0
    while True:
        k += 1
        if k > o["max_iterations"]:
            return done(T_MAX_ITERATIONS)
        if mu < o["radius_min"]:
            return done(T_RADIUS)
        out["iterations"] = k
        Js = J @ sp.diags(c)
        H = (Js.T @ Js).tocsr()
        if d is None:
            d = np.clip(H.diagonal(), o["d_lo"], o["d_hi"])
        n_cg, cg_rel = 0, 0.0
        try:
            t0 = time.perf_counter()
            step, n_cg, cg_rel = stepper(H + sp.diags(d / mu), -(Js.T @ r), o)
            out["linear_seconds"] += time.perf_counter() - t0
            Jd = Js @ step
            model = -float(np.dot(Jd, r + 0.5 * Jd))
            ok = bool(np.all(np.isfinite(step)) and model > 0.0)
        except np.linalg.LinAlgError:
            ok, model = False, 0.0
        row = dict(iteration=k, cost=cost, radius=mu, model_change=model, candidate_cost=0.0, step_norm=0.0, cg_iterations=n_cg, cg_residual=cg_rel, margins=[])
        out["trace"].append(row)
        if not ok:
            bad += 1
            row.update(status=INVALID, model_change=0.0)
            if bad >= o["max_invalid"]:
                return done(T_FAILURE)
            mu, nu = mu / nu, 2.0 * nu
            continue
        bad = 0
        delta = step * c
        x_c = x + delta
        cost_c, r_c, J_c = prob.evaluate(x_c)
        out["evaluations"] += 1
        dn, lim = float(np.linalg.norm(delta)), o["p_tol"] * (float(np.linalg.norm(x)) + o["p_tol"])
        row.update(candidate_cost=cost_c, step_norm=dn)
        row["margins"].append(("step_norm", dn, lim))
        if dn <= lim:
            row.update(status=PARAMETER)
            return done("parameter")
        change = cost - cost_c
        row["margins"].append(("function", abs(change), o["f_tol"] * cost))
        if abs(change) <= o["f_tol"] * cost:
            row.update(status=FUNCTION)
            return done("function")
        q = change / model
        row["margins"].append(("decrease", q, o["eta"]))
        if q > o["eta"]:
            x, cost, r, J = x_c, cost_c, r_c, J_c
            row.update(status=ACCEPTED)
            if np.max(np.abs(J.T @ r)) <= o["g_tol"]:
                row.update(status=GRADIENT)
                return done("gradient")
            mu = min(o["radius_max"], mu / max(1.0 / 3.0, 1.0 - (2.0 * q - 1.0) ** 3))
            nu = 2.0
            d = None
        else:
            row.update(status=REJECTED)
            mu, nu = mu / nu, 2.0 * nu


def spread(a, b):
    """between two solves of one problem: the largest difference in cost / candidate cost along the trace, relative to the solve's
    INITIAL cost, and the largest absolute difference in the unknowns.

    Why not relative to each cost itself: a graph whose edges agree (fixture `pair`) ends at cost 0, and a cost c = |r|^2 / 2 near 0
    is known only to |r| x (the rounding of the poses): its relative error grows without bound as |r| falls, whoever computes it.
    The initial cost is the scale at which every sum of the solve is formed, and it is the same number for both solves."""
    return cost_spread(a, b["trace"], b["initial_cost"], b["final_cost"]), (float(np.max(np.abs(a["x"] - b["x"]))) if len(b["x"]) else 0.0)


def cost_spread(a, trace, initial_cost, final_cost):
    """a: a solve of this file; trace: records with cost and candidate_cost (dicts) of the other solve"""
    scale = max(initial_cost, DBL_MIN)
    rel = abs(a["initial_cost"] - initial_cost) / scale
    for p, q in zip(a["trace"], trace):
        for key in ("cost", "candidate_cost"):
            rel = max(rel, abs(p[key] - q[key]) / scale)
    return max(rel, abs(a["final_cost"] - final_cost) / scale)


# ---- poses as matrices (fixture generation only) --------------------------------------------------------------------------------
def pose_mat(x):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rot(np.asarray(x[:3], dtype=np.float64)), x[3:]
    return T


def pose_vec(T):
    from scipy.spatial.transform import Rotation
    return np.concatenate([Rotation.from_matrix(T[:3, :3]).as_rotvec(), T[:3, 3]])


def relative(xa, xb):
    """Z with T_b = T_a Z"""
    return pose_vec(np.linalg.inv(pose_mat(xa)) @ pose_mat(xb))


def compose(xa, z):
    return pose_vec(pose_mat(xa) @ pose_mat(z))


def _noisy(rng, z, rot_sigma, trans_sigma):
    return compose(z, np.concatenate([rot_sigma * rng.normal(size=3), trans_sigma * rng.normal(size=3)]))


def _trajectory(rng, n, base=None, turn=0.05, stride=1.0):
    """a smooth drive of n poses from `base`: about `stride` metres forward and `turn` radians of heading change per frame"""
    truth = [np.asarray(base if base is not None else [0.02, -0.01, 0.03, 0.5, -0.2, 0.1], dtype=np.float64)]
    for _ in range(n - 1):
        truth.append(compose(truth[-1], np.array([0.01 * rng.normal(), turn + 0.01 * rng.normal(), 0.005 * rng.normal(),
                                                  0.05 * rng.normal(), 0.02 * rng.normal(), stride + 0.05 * rng.normal()])))
    return truth


def _dead_reckoning(first, odometry):
    poses = [np.asarray(first, dtype=np.float64)]
    for z in odometry:
        poses.append(compose(poses[-1], z))
    return poses


def chain_graph(seed, n, dframes, loops=(), base=None, turn=0.05, rot_sigma=2e-3, trans_sigma=0.02, ring=False):
    """n nodes; one edge (i, i + d) per d in dframes measured with noise; the initial poses are the dead reckoning of the d = 1
    edges from the first (fixed) node, so every other edge contradicts them; loops: (from, to, info) measured from the truth"""
    rng = np.random.default_rng(seed)
    turn = 2.0 * np.pi / n if ring else turn
    truth = _trajectory(rng, n, base, turn)
    edges = []
    for d in dframes:
        for i in range(n - d):
            edges.append((i, i + d, _noisy(rng, relative(truth[i], truth[i + d]), rot_sigma, trans_sigma), 1.0))
    for a, b, info in loops:
        edges.append((a, b, _noisy(rng, relative(truth[a], truth[b]), 0.1 * rot_sigma, 0.1 * trans_sigma), info))
    poses = _dead_reckoning(truth[0], [e[2] for e in edges[:n - 1]])
    return dict(poses={i: p for i, p in enumerate(poses)}, edges=edges, fixed=[0], truth=truth)


def fixture(name):
    """the graphs of the pose-graph tests (ISSUE section 5); dict(poses, edges, fixed, ...), all seeded"""
    if name == "pair":                                      # 1: two nodes, one edge
        rng = np.random.default_rng(401)
        t0 = np.array([0.3, -0.2, 0.5, 1.0, 2.0, -0.5])
        z = np.array([0.05, 0.1, -0.02, 0.1, -0.05, 1.2])
        start = compose(t0, z) + np.concatenate([0.02 * rng.normal(size=3), 0.1 * rng.normal(size=3)])
        return dict(poses={0: t0, 1: start}, edges=[(0, 1, z, 1.0)], fixed=[0], want={1: compose(t0, z)})
    if name == "chain5":                                    # 2: dframe 1, 2 and a loop edge that contradicts the chain
        g = chain_graph(402, 5, (1, 2))
        z = relative(g["truth"][0], g["truth"][4])
        z[3:] += np.array([0.15, -0.1, 0.2])
        g["edges"].append((0, 4, z, 1.0))
        return g
    if name == "ring70":                                    # 3: crosses a 64-lane boundary; shuffled, added in two calls
        g = chain_graph(403, 70, (1, 2, 3, 4), loops=[(69, 0, 1000.0)], ring=True)
        order = np.random.default_rng(4030).permutation(len(g["edges"]))
        g["edges"] = [g["edges"][i] for i in order]
        g["split"] = 97                                     # the first call's edges
        return g
    if name == "hub":                                       # 4: one node with 130 incident edges, two fixed nodes
        rng = np.random.default_rng(404)
        n = 131
        truth = [np.array([0.1, 0.2, -0.1, 0.0, 0.0, 0.0])]
        for i in range(1, n):
            a = 2.0 * np.pi * i / (n - 1)
            truth.append(np.concatenate([0.3 * rng.normal(size=3), [5.0 * np.cos(a), 0.5 * rng.normal(), 5.0 * np.sin(a)]]))
        edges = []
        for i in range(1, n):                               # the hub is node 0, alternately the `from` and the `to` end
            a, b = (0, i) if i % 2 else (i, 0)
            edges.append((a, b, _noisy(rng, relative(truth[a], truth[b]), 2e-3, 0.02), 1.0))
        for i in range(1, n - 1, 7):                        # rim edges, so that the spokes are over-determined
            edges.append((i, i + 1, _noisy(rng, relative(truth[i], truth[i + 1]), 2e-3, 0.02), 1.0))
        edges.append((1, 2, _noisy(rng, relative(truth[1], truth[2]), 2e-3, 0.02), 1.0))       # between the two fixed nodes
        edges.append(edges[4])                              # a duplicate
        poses = {i: truth[i] + np.concatenate([5e-3 * rng.normal(size=3), 0.05 * rng.normal(size=3)]) for i in range(n)}
        poses[1], poses[2] = truth[1], truth[2]
        poses[140] = np.array([0.7, -0.3, 0.2, 9.0, 8.0, 7.0])       # a free node without edges
        return dict(poses=poses, edges=edges, fixed=[1, 2], truth=truth)
    if name == "large_rotation":                            # 6: global rotation angles above 3 rad
        g = chain_graph(406, 6, (1, 2), base=[3.05 * 0.6, 3.05 * 0.0, 3.05 * 0.8, 0.5, 0.1, -0.3], turn=0.02)
        z = relative(g["truth"][0], g["truth"][5])
        z[3:] += np.array([0.1, 0.05, -0.1])
        g["edges"].append((0, 5, z, 4.0))
        return g
    raise KeyError(name)


FIXTURES = ("pair", "chain5", "ring70", "hub", "large_rotation")


def problem_of(g):
    return Problem(g["poses"], g["edges"], g["fixed"])
