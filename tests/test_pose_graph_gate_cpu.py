"""tests/pose_graph_gate_ref.py, the restatement of velo_graph_edge_gate and velo_graph_loop_candidates, checked on its own (no GPU):

  * Sigma_rel = D Sigma D^T with D the central differences of r in the stacked free poses: the formula has the right Jacobians;
  * the gauge property: Sigma_rel with frame 0 fixed against frame 3 fixed, where the marginals differ in the first digit;
  * the tree property: on chain12_tree Sigma_rel across an edge, in the tangent at its z, is the inverse of that edge's information;
  * the chi-square separation of true and false held-back edges on the two open graphs after pose_graph_ref.solve(..., "direct");
  * SPREAD_REL: the inverse-against-QR spread of Sigma_rel over the pairs the GPU test asks for, which it derives its tolerances from.

Also what of the new entries needs no device: the refusal of a null context and the two forms of Context.graph_edge_gate's `info`."""
import ctypes as C
import functools

import numpy as np
import pytest

import pose_graph_cov_ref as R
import pose_graph_gate_ref as Q
import pose_graph_ref as G
import velo_amd  # noqa: F401
from velo_amd import api, build

# Measured here, recorded as measured: per graph the largest difference of Sigma_rel between Sigma by the inverse and Sigma by the QR of J
# over Q.tested_pairs, in units of sigma_i sigma_j (the square roots of Sigma_rel's diagonal); "lap454_open/chi2": the largest relative
# difference of chi2 between the two routes over the held edges of the open graph after the solve.
SPREAD_REL = {"free1": 2.3e-16, "free2": 7.0e-16, "chain5": 8.2e-16, "large_rotation": 9.9e-16, "chain12_tree": 1.0e-9,
              "chain250_split": 3.7e-9, "hub140": 1.9e-13, "ring70_open": 9.1e-14, "lap454_open": 1.4e-12, "lap454_open/chi2": 7.0e-13,
              "ring70_open/chi2": 2.3e-14}
# (chain12_tree and chain250_split: long chains whose J^T J has a condition number above 1e6, which the explicit inverse pays in full and
# the QR of J only half of; against W_e^-1, which is exact, the QR route is right to 1.8e-13 on chain12_tree and the inverse to 1.0e-9)
# The figures the feature's plan states for the gauge and the tree property, and holds to 100 x: Sigma_rel with frame 0 fixed against frame 3
# fixed, and Sigma_rel across an edge of chain12_tree against W_e^-1.  They are the plan's measurements, on its own choice of pairs and
# seeds, kept as the bounds' base; this file's own, printed by the tests: 1.5e-15 / 2.1e-12 / 3.3e-15 on GAUGE_PAIRS, and 1.8e-13.
GAUGE = {"chain5": 1.9e-15, "ring70": 9.5e-13, "large_rotation": 2.5e-15}
GAUGE_PAIRS = {"chain5": [(1, 4), (2, 4), (1, 2), (4, 2)], "ring70": [(5, 40), (12, 55), (20, 63), (69, 1)],
               "large_rotation": [(1, 5), (2, 4), (1, 2), (5, 2)]}
TREE = 5.3e-13
MOVED = np.array([0.0, 0.0, 0.0, 3.0, 0.0, 0.0])                                 # a true loop measurement moved 3 m off


@functools.lru_cache(maxsize=None)
def loaded(name):
    """(graph, problem, poses, J) at the loaded state"""
    g, prob = Q.fixture(name)
    return g, prob, prob.poses_of(prob.x0()), R.dense_jacobian(prob)


@functools.lru_cache(maxsize=None)
def solved(name):
    """(graph, problem at the optimum, its poses, J there) after pose_graph_ref.solve(..., "direct")"""
    g, prob = Q.fixture(name)
    out = G.solve(prob, "direct")
    poses = prob.poses_of(out["x"])
    at = Q.at_poses(g, prob, poses)
    return g, at, poses, R.dense_jacobian(at)


def measure(name):
    """the inverse-against-QR spread of Sigma_rel over the tested pairs, at the loaded state"""
    g, prob, poses, J = loaded(name)
    S1, S2 = R.by_inverse(J), R.by_qr(J)
    frm, to, z, info = Q.tested_pairs(name, g, prob)
    _, _, c1, _ = Q.gate(S1, prob, poses, frm, to, z)
    _, _, c2, _ = Q.gate(S2, prob, poses, frm, to, z)
    worst = 0.0
    for a, b in zip(c1, c2):
        if np.all(a == 0.0):                                           # both ends fixed
            assert np.all(b == 0.0)
            continue
        worst = max(worst, Q.rel_spread(a, b))
    return worst, len(frm)


@pytest.mark.parametrize("name", [k for k in SPREAD_REL if "/" not in k and k != "lap454_open"])
def test_the_two_routes_agree_on_sigma_rel(name):
    worst, n = measure(name)
    print(f"{name}: Sigma_rel, inverse against QR over {n} pairs: {worst:.2e} sigma_i sigma_j (record {SPREAD_REL[name]:.1e})")
    assert worst <= 3 * SPREAD_REL[name]                               # the record is what was measured, to a factor of 3 (LAPACK builds differ)


@pytest.mark.parametrize("name", ["chain5", "large_rotation", "chain12_tree"])
def test_sigma_rel_is_the_first_order_covariance_of_r(name):
    g, prob, poses, J = loaded(name)
    S = R.by_inverse(J)
    frm, to, z, _ = Q.tested_pairs(name, g, prob)
    x0, h = prob.x0(), 1e-6
    worst = 0.0
    for p, (a, b) in enumerate(zip(frm, to)):
        _, zp, _, A, B = Q.pair_terms(poses, a, b, None if z is None else z[p])
        D = np.zeros((6, prob.N))
        for k in range(prob.N):                                        # central differences of r in the stacked free poses
            e = np.zeros(prob.N)
            e[k] = h
            Pp, Pm = prob.poses_of(x0 + e), prob.poses_of(x0 - e)
            D[:, k] = (G.edge_eval(Pp[a], Pp[b], zp, 1.0, False) - G.edge_eval(Pm[a], Pm[b], zp, 1.0, False)) / (2.0 * h)
        worst = max(worst, Q.rel_spread(Q.sigma_rel(S, prob, a, b, A, B), D @ S @ D.T))
    print(f"{name}: Sigma_rel against D Sigma D^T by central differences over {len(frm)} pairs: {worst:.2e}")
    # the differences carry h^2 |r'''| / 6 ~ 1e-12 of truncation and eps / h ~ 1e-10 of rounding per entry of D; twice that in the product,
    # amplified by the conditioning of the 6 x 6 (sigma_i sigma_j against its off-diagonal entries): 1e-7 leaves two digits
    assert worst <= 1e-7


@pytest.mark.parametrize("name", sorted(GAUGE))
def test_sigma_rel_does_not_depend_on_the_fixed_frame(name):
    g = G.fixture(name)
    out, marg = [], []
    for fixed in (0, 3):
        prob = G.Problem(g["poses"], g["edges"], [fixed])
        poses = prob.poses_of(prob.x0())
        S = R.by_inverse(R.dense_jacobian(prob))
        frm, to = zip(*GAUGE_PAIRS[name])
        out.append(Q.gate(S, prob, poses, frm, to)[2])
        marg.append(np.array([Q.block(S, prob, a, a) for a in frm]))
    worst = max(Q.rel_spread(a, b) for a, b in zip(*out))
    moved = float(np.max(np.abs(marg[0] - marg[1])))
    print(f"{name}: Sigma_rel, frame 0 fixed against frame 3 fixed: {worst:.2e} sigma_i sigma_j (record {GAUGE[name]:.1e}); the marginals differ by {moved:.2f}")
    assert worst <= 100 * GAUGE[name]
    assert moved > 1e-3                                                # the marginals do depend on the gauge


def test_on_a_tree_sigma_rel_across_an_edge_is_the_inverse_of_its_information():
    g, prob, poses, J = loaded("chain12_tree")
    S = R.by_qr(J)                                                     # (the route that never forms J^T J; see SPREAD_REL)
    frm, to, z = [e[0] for e in g["edges"]], [e[1] for e in g["edges"]], [e[2] for e in g["edges"]]
    cov = Q.gate(S, prob, poses, frm, to, z)[2]
    worst = max(Q.rel_spread(np.linalg.inv(e[3]), c) for e, c in zip(g["edges"], cov))
    print(f"chain12_tree: Sigma_rel across an edge against W_e^-1: {worst:.2e} (record {TREE:.1e})")
    assert len(frm) == 11 and worst <= 100 * TREE


def held_chi2(name, route=R.by_inverse):
    g, prob, poses, J = solved(name)
    S = route(J)
    frm, to = [e[0] for e in g["held"]], [e[1] for e in g["held"]]
    z, info = np.array([e[2] for e in g["held"]]), [e[3] for e in g["held"]]
    return g, S, prob, poses, frm, to, z, info


def test_chi2_separates_the_true_closing_edge_of_ring70_open_from_the_outliers():
    g, S, prob, poses, frm, to, z, info = held_chi2("ring70_open")
    chi2 = Q.gate(S, prob, poses, frm, to, z, info)[3]
    true = [k in g["true_held"] for k in range(len(frm))]
    print("ring70_open: chi2 of the held edges " + ", ".join(f"({a}, {b}) {c:.1f}" for a, b, c in zip(frm, to, chi2)))
    assert sum(true) == 1 and len(frm) == 4
    other = Q.gate(R.by_qr(solved("ring70_open")[3]), prob, poses, frm, to, z, info)[3]
    rel = float(np.max(np.abs(other - chi2) / chi2))
    print(f"ring70_open: inverse against QR: chi2 {rel:.2e} relative (record {SPREAD_REL['ring70_open/chi2']:.1e})")
    assert rel <= 3 * SPREAD_REL["ring70_open/chi2"]
    assert all(c < 30.0 for c, t in zip(chi2, true) if t) and all(c > 300.0 for c, t in zip(chi2, true) if not t)
    # at the dead-reckoned start the covariance does not belong to the estimate: the true edge does not pass
    g0, prob0, poses0, J0 = loaded("ring70_open")
    k = g["true_held"][0]
    start = Q.gate(R.by_inverse(J0), prob0, poses0, frm[k:k + 1], to[k:k + 1], z[k:k + 1], info[k:k + 1])[3][0]
    print(f"ring70_open: the true edge before optimising: {start:.1f}")
    assert start > 30.0


def test_chi2_separates_the_loop_measurements_of_lap454_open_from_moved_ones():
    g, S, prob, poses, frm, to, z, info = held_chi2("lap454_open")
    chi2 = Q.gate(S, prob, poses, frm, to, z, info)[3]
    off = Q.gate(S, prob, poses, frm, to, z + MOVED, info)[3]
    print(f"lap454_open: {len(frm)} held loop measurements: chi2 median {np.median(chi2):.1f}, max {chi2.max():.1f}; moved 3 m off: min {off.min():.1f}")
    assert len(frm) == 462 and chi2.min() >= 0.0
    assert chi2.max() < 30.0 and off.min() > 300.0
    other = Q.gate(R.by_qr(solved("lap454_open")[3]), prob, poses, frm, to, z, info)
    rel = float(np.max(np.abs(other[3] - chi2) / chi2))
    worst = max(Q.rel_spread(a, b) for a, b in zip(Q.gate(S, prob, poses, frm, to, z)[2], Q.gate(R.by_qr(solved("lap454_open")[3]), prob, poses, frm, to, z)[2]))
    print(f"lap454_open: inverse against QR: chi2 {rel:.2e} relative (record {SPREAD_REL['lap454_open/chi2']:.1e}), Sigma_rel {worst:.2e} (record {SPREAD_REL['lap454_open']:.1e})")
    assert rel <= 3 * SPREAD_REL["lap454_open/chi2"] and worst <= 3 * SPREAD_REL["lap454_open"]


def test_candidates_of_the_restatement_widen_with_k_sigma():
    g, S, prob, poses, *_ = held_chi2("lap454_open")
    for query in (320, 453):
        f0, d0, s0, _ = Q.candidates(S, prob, poses, query, 50, 3.0, 0.0)
        f3, d3, s3, _ = Q.candidates(S, prob, poses, query, 50, 3.0, 3.0)
        sel0, sel3 = set(f0[d0 <= 3.0].tolist()), set(f3[d3 <= 3.0 + 3.0 * s3].tolist())
        print(f"lap454_open, query {query}: {len(sel0)} frames within 3 m, {len(sel3)} within 3 m + 3 sigma (sigma {s3.min():.3f} .. {s3.max():.3f} m)")
        assert np.all(s0 == 0.0) and np.all(s3 > 0.0) and sel0 < sel3
        assert all(abs(i - query) >= 50 for i in f0)


@pytest.fixture(scope="module")
def lib():
    return C.CDLL(build.build_hip())


def test_refusals_that_need_no_device(lib):
    one = (C.c_int32 * 1)(0)
    out = (C.c_double * 36)(*([7.0] * 36))
    found = C.c_int32(7)
    lib.velo_last_error.restype = C.c_char_p
    lib.velo_graph_edge_gate.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32] + [C.c_void_p] * 8
    lib.velo_graph_loop_candidates.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_int32] + [C.c_void_p] * 4
    assert lib.velo_graph_edge_gate(None, one, 1, None, 1, one, one, None, None, out, out, out, out) == -1 and b"null ctx" in lib.velo_last_error()
    assert lib.velo_graph_loop_candidates(None, one, 1, None, 0, 1, 1.0, 0.0, 1, one, out, out, C.byref(found)) == -1 and b"null ctx" in lib.velo_last_error()
    assert all(v == 7.0 for v in out) and found.value == 7 and one[0] == 0


class _Recorder:
    """stands in for a context: keeps what Context.graph_edge_gate hands to the C-ABI"""

    def __init__(self):
        self._h, self.calls = None, []
        self._lib = self
        self._graph_params = api.Context._graph_params

    def _check(self, status):
        assert status == 0

    def velo_graph_edge_gate(self, h, fixed, n_fixed, params, n, a, b, z, info, rel, r, cov, chi2):
        arr = lambda p, t, m: None if not p else np.ctypeslib.as_array(C.cast(p, C.POINTER(t)), (m,)).copy()   # noqa: E731
        self.calls.append(dict(fixed=arr(fixed, C.c_int32, n_fixed), a=arr(a, C.c_int32, n), b=arr(b, C.c_int32, n), z=arr(z, C.c_double, 6 * n),
                               info=arr(info, C.c_double, 21 * n), params=params))
        np.ctypeslib.as_array(C.cast(chi2, C.POINTER(C.c_double)), (max(n, 1),))[:] = 5.0
        return 0


def test_the_two_forms_of_info():
    ctx = _Recorder()
    rng = np.random.default_rng(7)
    Ws = np.array([Q.W.spd(rng), Q.W.spd(rng)])
    z = rng.normal(size=(2, 6))
    rel, r, cov, chi2 = api.Context.graph_edge_gate(ctx, [3, 5], [9, 1], z, Ws, fixed=(0, 2))
    full = ctx.calls[-1]
    assert rel.shape == r.shape == (2, 6) and cov.shape == (2, 6, 6) and np.all(chi2 == 5.0)
    assert np.array_equal(full["a"], [3, 5]) and np.array_equal(full["b"], [9, 1]) and np.array_equal(full["fixed"], [0, 2]) and full["params"] is None
    assert np.array_equal(full["z"], z.ravel())
    api.Context.graph_edge_gate(ctx, [3, 5], [9, 1], z, np.array([Q.W.info21(w) for w in Ws]), max_work=9)
    packed = ctx.calls[-1]
    assert np.array_equal(packed["info"], full["info"]) and packed["info"][1] == Ws[0][0, 1] and packed["info"][6] == Ws[0][1, 1]
    assert packed["params"] is not None
    api.Context.graph_edge_gate(ctx, [3], [9])                         # neither: both pointers NULL
    assert ctx.calls[-1]["z"] is None and ctx.calls[-1]["info"] is None
    bad = Ws.copy()
    bad[0, 0, 1] += 1e-9
    for info in (bad, np.zeros((2, 20)), np.zeros((2, 6, 5))):
        with pytest.raises(ValueError):
            api.Context.graph_edge_gate(ctx, [3, 5], [9, 1], z, info)
    with pytest.raises(ValueError):
        api.Context.graph_edge_gate(ctx, [3, 5], [9], z, Ws)
    ctx.graph_edge_gate = lambda frm, to, z, info, fixed: api.Context.graph_edge_gate(ctx, frm, to, z, info, fixed)
    rel, cov = api.Context.graph_relative_covariance(ctx, [[4, 8], [8, 4]], fixed=(1,))
    assert rel.shape == (2, 6) and cov.shape == (2, 6, 6) and np.array_equal(ctx.calls[-1]["a"], [4, 8]) and np.array_equal(ctx.calls[-1]["b"], [8, 4])
    for bad_pairs in ([1, 2, 3], [[1.5, 2.0]]):
        with pytest.raises(ValueError):
            api.Context.graph_relative_covariance(ctx, bad_pairs)
