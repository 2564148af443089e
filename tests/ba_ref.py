"""A numpy restatement of the windowed bundle adjustment over a LandmarkBook, written from the functors bundle2D / bundle3D
(costfunctions.h:222-286) and from SURVEY.md Appendix B1 -- NOT from the kernels -- so that velo_landmarks_adjust has something
independent to be compared with.  Test infrastructure only.

The unknowns are, in this order, the 6 doubles (angle-axis, centre) of every FREE frame of the window and the 3 doubles of every
participating landmark.  A landmark takes part if it is added, has at least 2 observations in window frames and at least one of
them in a free frame.  Its residual blocks come in the order of velo.h:1049-1122 restricted to the window: 3-D first, then 2-D,
each camera-major and frame-ascending.

What is deliberately different from the kernels:
  * derivatives: the closed form of d(R(w) q)/dw (Gallego & Yezzi 2015, eq. 8), the kernels use dual numbers;
  * the rotation: the matrix form on the un-normalised vector with numpy's sin / cos;
  * the linear algebra: a dense Jacobian and either an SVD of the augmented system [J; D] or a Schur complement on the dense
    normal equations; the model change row by row, -(J s).(r + J s / 2).
"""
from __future__ import annotations

import numpy as np

EPS = np.finfo(np.float64).eps
DBL_MIN = np.finfo(np.float64).tiny

ACCEPTED, REJECTED, INVALID, PARAMETER, FUNCTION, GRADIENT = 0, 1, 2, 3, 4, 5      # velo_ba_iteration.status
STATUS_NAMES = {ACCEPTED: "accepted", REJECTED: "rejected", INVALID: "invalid", PARAMETER: "parameter", FUNCTION: "function", GRADIENT: "gradient"}
T_MAX_ITERATIONS, T_RADIUS, T_FAILURE = "max_iterations", "radius", "failure"

LM_DEFAULTS = dict(max_iterations=50, radius0=1e4, eta=1e-3, f_tol=1e-6, g_tol=1e-10, p_tol=1e-8, d_lo=1e-6, d_hi=1e32,
                   radius_min=1e-32, radius_max=1e16, max_invalid=5)


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def rotate_with_derivative(w, q):
    """AngleAxisRotatePoint: R(w) q, d/dw [3, 3], d/dq [3, 3]."""
    t2 = float(w @ w)
    if t2 > EPS:
        t = np.sqrt(t2)
        K = skew(w)
        R = np.eye(3) + (np.sin(t) / t) * K + ((1.0 - np.cos(t)) / t2) * (K @ K)
        dw = -R @ skew(q) @ (np.outer(w, w) + (R.T - np.eye(3)) @ K) / t2
        return R @ q, dw, R
    return q + np.cross(w, q), -skew(q), np.eye(3) + skew(w)      # first-order branch


class Problem:
    """The window's problem taken from a LandmarkBook: who takes part, and every residual block in order."""

    def __init__(self, book, poses, cam_trans, frames, n_fixed, weight_3d=1.0, loss_a=0.01, loss_w=10.0, require_free=True):
        self.frames = [int(f) for f in frames]
        self.n_fixed, self.n_free = int(n_fixed), len(frames) - int(n_fixed)
        self.poses0 = np.array([poses[f] for f in self.frames], dtype=np.float64)
        self.cam_trans = np.asarray(cam_trans, dtype=np.float32).astype(np.float64)
        self.weight_3d, self.loss_a, self.loss_w = float(weight_3d), float(loss_a), float(loss_w)
        widx = {f: k for k, f in enumerate(self.frames)}
        seen = set()
        for cam in range(book.num_cams):
            for f in self.frames:
                seen |= set(book.keypoint_ids.get(cam, {}).get(f, []))
        self.ids, self.blocks, self.first_block = [], [], [0]        # blocks: (landmark index, kind, window index, cam, s[3])
        for id in sorted(seen):
            if not book.keypoint_added[id]:
                continue
            rows = []
            for cam in range(book.num_cams):
                for f in sorted(book.keypoint_obs3[id][cam]):
                    if f in widx:
                        rows.append((0, widx[f], cam, np.asarray(book.keypoint_obs3[id][cam][f], dtype=np.float32).astype(np.float64)))
            for cam in range(book.num_cams):
                for f in sorted(book.keypoint_obs2[id][cam]):
                    if f in widx:
                        p = np.asarray(book.keypoint_obs2[id][cam][f], dtype=np.float32).astype(np.float64)
                        rows.append((1, widx[f], cam, np.array([p[0], p[1], 0.0])))
            if len(rows) < 2 or (require_free and not any(r[1] >= self.n_fixed for r in rows)):
                continue
            l = len(self.ids)
            self.ids.append(int(id))
            self.blocks += [(l,) + r for r in rows]
            self.first_block.append(len(self.blocks))
        self.L = len(self.ids)
        self.points0 = np.array([book.landmarks[id] for id in self.ids], dtype=np.float32).astype(np.float64).reshape(-1, 3)
        self.n_blocks = len(self.blocks)
        self.n_residuals = sum(3 if b[1] == 0 else 2 for b in self.blocks)
        self.N = 6 * self.n_free + 3 * self.L

    def x0(self):
        return np.concatenate([self.poses0[self.n_fixed:].ravel(), self.points0.ravel()])

    def poses_of(self, x):
        P = self.poses0.copy()
        P[self.n_fixed:] = x[:6 * self.n_free].reshape(-1, 6)
        return P

    def points_of(self, x):
        return x[6 * self.n_free:].reshape(-1, 3)

    def evaluate(self, x, robust=True):
        """cost = sum rho / 2 and the (robustified) rows r, J [rows, N] in block order"""
        P, X = self.poses_of(x), self.points_of(x)
        r = np.zeros(self.n_residuals)
        J = np.zeros((self.n_residuals, self.N))
        cost, row = 0.0, 0
        nf6 = 6 * self.n_free
        for (l, kind, k, cam, s) in self.blocks:
            cam6 = P[k]
            M, dw, R = rotate_with_derivative(-cam6[:3], X[l] - cam6[3:])
            d_cam = np.hstack([-dw, -R])                              # rot = -camera[0:3], M_original = point - camera[3:6]
            if kind == 0:                                             # bundle3D, TrivialLoss
                res, Jp, Jc = self.weight_3d * (M - s), self.weight_3d * R, self.weight_3d * d_cam
                rho, d1 = float(res @ res), 1.0
            else:                                                     # bundle2D, ScaledLoss(CauchyLoss(a), w)
                Mc = M + self.cam_trans[cam]
                A = np.array([[1.0, 0.0, -s[0]], [0.0, 1.0, -s[1]]])
                res, Jp, Jc = A @ Mc, A @ R, A @ d_cam
                sq = float(res @ res)
                if robust:
                    b = self.loss_a * self.loss_a
                    rho, d1 = self.loss_w * b * np.log1p(sq / b), self.loss_w * max(DBL_MIN, 1.0 / (1.0 + sq / b))
                else:
                    rho, d1 = sq, 1.0
            cost += 0.5 * rho
            sq1 = np.sqrt(d1)
            d = len(res)
            r[row:row + d] = res * sq1
            J[row:row + d, nf6 + 3 * l:nf6 + 3 * l + 3] = Jp * sq1
            if k >= self.n_fixed:
                c0 = 6 * (k - self.n_fixed)
                J[row:row + d, c0:c0 + 6] = Jc * sq1
            row += d
        return cost, r, J

    def system(self, x=None):
        """cost, the pose part of J^T r and the pose diagonal blocks of J^T J at x (default: the stored state)"""
        cost, r, J = self.evaluate(self.x0() if x is None else x)
        nf6 = 6 * self.n_free
        g = J[:, :nf6].T @ r
        H = J[:, :nf6].T @ J[:, :nf6]
        return cost, g, np.array([H[6 * k:6 * k + 6, 6 * k:6 * k + 6] for k in range(self.n_free)]).reshape(-1, 6, 6)


def step_lstsq(Js, r, d, mu, n_pose):
    A = np.vstack([Js, np.diag(np.sqrt(d / mu))])
    b = np.concatenate([-r, np.zeros(Js.shape[1])])
    step, *_ = np.linalg.lstsq(A, b, rcond=None)
    return step


def step_schur(Js, r, d, mu, n_pose):
    """the Schur complement on the landmark blocks of the normal equations (H + D / mu) s = -g"""
    H = Js.T @ Js + np.diag(d / mu)
    g = Js.T @ r
    U, W, V = H[:n_pose, :n_pose], H[:n_pose, n_pose:], H[n_pose:, n_pose:]
    L = V.shape[0] // 3
    Vi = np.zeros_like(V)
    for l in range(L):
        sl = slice(3 * l, 3 * l + 3)
        Vi[sl, sl] = np.linalg.inv(V[sl, sl])
    Y = W @ Vi
    S = U - Y @ W.T
    sc = np.linalg.solve(S, -g[:n_pose] + Y @ g[n_pose:])
    sp = Vi @ (-g[n_pose:] - W.T @ sc)
    return np.concatenate([sc, sp])


def solve(prob, linear="schur", robust=True, **kw):
    """SURVEY.md Appendix B1 over all unknowns.  Returns dict(x, termination, trace, iterations, evaluations, initial_cost,
    final_cost); trace = one dict per iteration with status, cost, candidate_cost, radius, model_change, step_norm and the
    margins of every decision taken."""
    o = dict(LM_DEFAULTS)
    o.update(kw)
    stepper = step_schur if linear == "schur" else step_lstsq
    n_pose = 6 * prob.n_free
    x = prob.x0()
    cost, r, J = prob.evaluate(x, robust)
    out = dict(initial_cost=cost, evaluations=1, iterations=0, trace=[])

    def done(label):
        out.update(x=x, termination=label, final_cost=cost)
        return out
    g = J.T @ r
    if np.max(np.abs(g)) <= o["g_tol"]:
        return done("gradient")
    c = 1.0 / (1.0 + np.sqrt(np.sum(J * J, axis=0)))              # Jacobi scaling, ONCE
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
        Js = J * c
        if d is None:
            d = np.clip(np.sum(Js * Js, axis=0), o["d_lo"], o["d_hi"])
        try:
            step = stepper(Js, r, d, mu, n_pose)
            Jd = Js @ step
            model = -float(np.dot(Jd, r + 0.5 * Jd))
            ok = bool(np.all(np.isfinite(step)) and model > 0.0)
        except np.linalg.LinAlgError:
            ok, model = False, 0.0
        row = dict(iteration=k, cost=cost, radius=mu, model_change=model, candidate_cost=0.0, step_norm=0.0, margins=[])
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
        cost_c, r_c, J_c = prob.evaluate(x_c, robust)
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


def closest_margin(trace):
    """the smallest relative distance of a decision quantity from its threshold along a trace"""
    m = np.inf
    for row in trace:
        for _, value, limit in row["margins"]:
            m = min(m, abs(value - limit) / max(abs(limit), DBL_MIN))
    return m


def spread(a, b):
    """between two solves of one problem: the largest relative difference in cost / candidate cost along the trace, the largest
    absolute difference in the poses and in the points"""
    rel = 0.0
    for p, q in zip(a["trace"], b["trace"]):
        for key in ("cost", "candidate_cost"):
            rel = max(rel, abs(p[key] - q[key]) / max(abs(q[key]), DBL_MIN))
    return rel, float(np.max(np.abs(a["x"] - b["x"])))


def triangulate_book(book, poses, cam_trans, frames, loss_a=0.01, loss_w=10.0):
    """a stand-in for triangulatePoint on the CPU: every id with at least 3 observations seen in `frames` gets the minimiser of
    its own 3-unknown problem (all poses constant) from (0, 0, 10), stored as float and marked added"""
    ids = sorted({id for f in frames for id in book.ids_to_triangulate(f)})
    all_frames = sorted({f for cam in book.keypoint_ids for f in book.keypoint_ids[cam]})
    for id in ids:
        book.landmarks[id] = np.array([0.0, 0.0, 10.0], dtype=np.float32)
        book.keypoint_added[id] = True
    for id in ids:
        one = _OneLandmark(book, poses, cam_trans, all_frames, id, loss_a, loss_w)
        res = solve(one, "lstsq")
        book.landmarks[id] = res["x"].astype(np.float32)


class _OneLandmark(Problem):
    def __init__(self, book, poses, cam_trans, frames, id, loss_a, loss_w):
        only = _BookView(book, id)
        super().__init__(only, poses, cam_trans, frames, len(frames), 1.0, loss_a, loss_w, require_free=False)   # every frame is a constant here


class _BookView:
    """a LandmarkBook that shows one id only"""

    def __init__(self, book, id):
        self.num_cams = book.num_cams
        self.keypoint_added, self.landmarks = book.keypoint_added, book.landmarks
        self.keypoint_obs2, self.keypoint_obs3 = book.keypoint_obs2, book.keypoint_obs3
        self.keypoint_ids = {cam: {f: [i for i in ids if i == id] for f, ids in per.items()} for cam, per in book.keypoint_ids.items()}


# ---- the fixtures of the bundle adjustment tests --------------------------------------------------------------------------------
FIXTURES = {"A": dict(seed=301, n_frames=4, n_ids=12), "B": dict(seed=302, n_frames=6, n_ids=40), "C": dict(seed=303, n_frames=11, n_ids=60)}


def perturbed_sequence(seed, n_frames, ids, n_cams=2, n_fixed=1, first_frame=None, **kw):
    """landmarks_ref.sequence(...) with every id alive through the whole window (unless first_frame says otherwise) and the poses
    after the first n_fixed perturbed by a seeded 3 cm / 2 mrad; seq["truth"] keeps the unperturbed ones"""
    import landmarks_ref as LR
    ids = list(ids)
    ff = {id: (id % 3, n_frames) for id in ids}
    ff.update(first_frame or {})
    seq = LR.sequence(seed, n_frames, n_cams, ids, first_frame=ff, **kw)
    rng = np.random.default_rng(seed + 1000)
    seq["truth"] = seq["poses"].copy()
    seq["poses"] = seq["poses"].copy()
    seq["poses"][n_fixed:, :3] += 2e-3 * rng.normal(size=(n_frames - n_fixed, 3))
    seq["poses"][n_fixed:, 3:] += 0.03 * rng.normal(size=(n_frames - n_fixed, 3))
    return seq


def fixture_sequence(name):
    f = FIXTURES[name]
    return perturbed_sequence(f["seed"], f["n_frames"], range(f["n_ids"]))


def book_of(seq):
    import landmarks_ref as LR
    book = LR.LandmarkBook(seq["n_cams"])
    for f, per_cam in enumerate(seq["frames"]):
        book.observe_frame(f, [c[1] for c in per_cam], [c[0] for c in per_cam], [c[2] for c in per_cam], [c[3] for c in per_cam])
    return book
