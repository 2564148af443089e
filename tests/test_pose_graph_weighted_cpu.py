"""tests/pose_graph_weighted_ref.py, the restatement of the pose graph with a 6 x 6 information per edge and a Cauchy loss, checked
on its own (no GPU): its robustified gradient against central differences of its cost, W = s . I with the trivial loss against
pose_graph_ref.Problem, its two linear solvers against each other on every fixture of the GPU test, and what a robust loss is for
-- three gross loop closures that bend the trivial-loss solve are switched off.  The spreads measured here are what
tests/test_gpu_pose_graph_weighted.py derives its tolerances from.  Also what of the new entries needs no device:
velo_graph_edge_information against the numpy formula and its meaning, and the refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

import pose_graph_ref as G
import pose_graph_weighted_ref as W
import velo_amd  # noqa: F401
from velo_amd import api, build


@functools.lru_cache(maxsize=None)
def solves(name):
    g = W.fixture(name)
    prob = W.problem_of(g)
    return g, prob, G.solve(prob, "direct"), G.solve(prob, "pcg")


def test_robustified_gradient_against_central_differences_of_the_cost():
    g = W.fixture("chain5_mixed")
    rng = np.random.default_rng(21)
    # every kind of edge at once: scalar, full W, Cauchy scales that put the weights anywhere between 0.02 and 1
    g["edges"] = [(a, b, z, Wm if k % 2 else W.spd(rng), (0.0, 0.05, 0.5)[k % 3]) for k, (a, b, z, Wm, _) in enumerate(g["edges"])]
    prob = W.problem_of(g)
    x = prob.x0() + 0.01 * rng.normal(size=prob.N)
    cost, r, J = prob.evaluate(x)
    weights = prob.edge_stats(x)[1]
    assert weights.min() < 0.1 and weights.max() == 1.0
    grad = J.T @ r
    h, worst = 1e-6, 0.0
    for j in range(prob.N):
        e = np.zeros(prob.N)
        e[j] = h
        worst = max(worst, abs((prob.evaluate(x + e, False)[0] - prob.evaluate(x - e, False)[0]) / (2 * h) - grad[j]))
    # central differences of step h: truncation ~ h^2 |c'''| / 6 and rounding ~ eps |c| / h, against a gradient of order |grad|
    assert worst < 1e-6 * max(1.0, np.abs(grad).max()), (worst, np.abs(grad).max())
    assert cost == pytest.approx(0.5 * sum(W.rho(s, a)[0] for s, a in zip(prob.edge_stats(x)[0], prob.loss)), rel=1e-14)


@pytest.mark.parametrize("name", G.FIXTURES)
def test_scalar_information_and_trivial_loss_is_the_scalar_problem(name):
    g = G.fixture(name)
    scalar = G.problem_of(g)
    both = [W.Problem(g["poses"], [(a, b, z, info * np.eye(6), 0.0) for a, b, z, info in g["edges"]], g["fixed"]),
            W.Problem(g["poses"], [(a, b, z, info, 0.0) for a, b, z, info in g["edges"]], g["fixed"])]
    c0, r0, J0 = scalar.evaluate(scalar.x0())
    H0 = (J0.T @ J0).toarray()
    for prob in both:
        c, r, J = prob.evaluate(prob.x0())
        H = (J.T @ J).toarray()
        assert abs(c - c0) <= 1e-12 * c0
        assert np.abs(J.T @ r - J0.T @ r0).max() <= 1e-12 * np.abs(J0.T @ r0).max()
        assert np.abs(H - H0).max() <= 1e-12 * np.abs(H0).max()
        chi2, weight = prob.edge_stats()
        assert np.all(weight == 1.0) and 0.5 * chi2.sum() == pytest.approx(c0, rel=1e-12)


# Measured on this restatement between `direct` and `pcg` (cost: relative to the initial cost along the trace; unknowns: absolute);
# the GPU test allows 100 x these.  Where the two solvers agree to below one unit of the format -- `pair_w` has one free node, so
# block-Jacobi CG IS a direct solve (measured 4.0e-20, 2.8e-17); `chain5_w` converges in 24 CG iterations to 1.2e-17, 5.6e-17 --
# the entry is one unit of the format instead, as for `pair` in test_pose_graph_cpu.py: DBL_EPSILON in cost, and DBL_EPSILON x the
# power of two above the largest pose component (2.0 -> 4, 4.6 -> 8) in the unknowns.
SPREAD = {"pair_w": (2.3e-16, 8.9e-16), "chain5_w": (2.3e-16, 1.8e-15), "chain5_mixed": (3.3e-15, 8.9e-15),
          "ring70_outliers": (5.9e-14, 8.0e-14), "ring70_outliers_trivial": (5.7e-13, 1.7e-12)}
STATUSES = {"pair_w": [0, 0, 0, 3], "chain5_w": [0, 0, 0, 4], "chain5_mixed": [0, 0, 0, 0, 0, 4], "ring70_outliers": [0, 0, 0, 0, 0, 4],
            "ring70_outliers_trivial": [0, 0, 0, 4]}


@pytest.mark.parametrize("name", W.FIXTURES)
def test_the_two_solvers_take_the_same_decisions(name):
    g, prob, a, b = solves(name)
    assert [r["status"] for r in a["trace"]] == [r["status"] for r in b["trace"]] == STATUSES[name]
    assert a["termination"] == b["termination"] and a["iterations"] == b["iterations"] and a["evaluations"] == b["evaluations"]
    margin = min(G.closest_margin(a["trace"]), G.closest_margin(b["trace"]))
    assert margin > 1e-6, margin                                     # no decision lies near its threshold: rounding cannot flip one
    sc, sx = G.spread(a, b)
    print(f"{name}: spread {sc:.2e} of the initial cost, {sx:.2e} absolute in the unknowns; closest decision margin {margin:.2e}; "
          f"CG iterations {[r['cg_iterations'] for r in b['trace']]}, cap {G.CG_DEFAULTS['cg_max']}")
    assert max(r["cg_iterations"] for r in b["trace"]) < G.CG_DEFAULTS["cg_max"]
    assert sc <= 3 * SPREAD[name][0] and sx <= 3 * SPREAD[name][1]   # what was measured, to a factor of 3 (LAPACK builds differ)
    x = prob.poses_of(a["x"])
    if name == "pair_w":                                             # T_0 . Z and cost 0 whatever W is
        assert np.abs(x[1] - g["want"][1]).max() <= 10 * 1e-8 * np.linalg.norm(g["want"][1])
        assert a["final_cost"] <= G.EPS * a["initial_cost"]
    if name == "chain5_mixed":                                       # the loop edge is neither kept whole nor switched off
        for s in (a, b):
            assert 0.05 < prob.edge_stats(s["x"])[1][-1] < 0.95
        assert [np.ndim(e[3]) for e in g["edges"]] == [0] * 7 + [2]  # scalar odometry first, the weighted edge behind it


def test_cauchy_switches_gross_loop_closures_off():
    g, prob, _, robust = solves("ring70_outliers")
    gt, probt, _, trivial = solves("ring70_outliers_trivial")
    out = g["outliers"]
    assert sorted((g["edges"][k][0], g["edges"][k][1]) for k in out) == sorted(W.OUTLIERS) and len(g["edges"]) == 274
    assert all(g["edges"][k][4] == (W.CAUCHY if abs(g["edges"][k][0] - g["edges"][k][1]) > 4 else 0.0) for k in range(274))
    assert all(e[4] == 0.0 for e in gt["edges"])
    chi2, weight = prob.edge_stats(robust["x"])
    start = W.position_error(g, g["poses"])
    err, err_trivial = W.position_error(g, prob.poses_of(robust["x"])), W.position_error(gt, probt.poses_of(trivial["x"]))
    print(f"outlier weights {weight[out]}, smallest other weight {np.delete(weight, out).min():.3f}; largest position error: start {start:.3f} m, "
          f"Cauchy {err:.3f} m, trivial {err_trivial:.3f} m")
    assert np.all(weight[out] < 1e-2)
    assert np.delete(weight, out).min() > 0.5
    assert err <= 0.25 * err_trivial
    assert err_trivial > start


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return api.load_library()


def _z(rng, angle):
    axis = rng.normal(size=3)
    return np.concatenate([angle * axis / np.linalg.norm(axis), rng.normal(size=3)])


@pytest.mark.parametrize("angle", [0.3, 0.0, 3.0])
def test_edge_information_equals_the_numpy_formula(lib, angle):
    rng = np.random.default_rng(31)
    z = _z(rng, angle)
    H = W.spd(rng) + 0.1 * rng.normal(size=(6, 6))                   # not symmetric: the entry symmetrises first
    got, want = api.graph_edge_information(z, H), W.edge_information(z, H)
    assert np.array_equal(got, got.T)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_edge_information_means_the_registrations_quadratic():
    """r(z + t d)^T W r(z + t d) is t^2 d^T H d up to the residual's linearisation error, which falls linearly in t"""
    rng = np.random.default_rng(32)
    z, H, d = _z(rng, 0.3), W.spd(rng), rng.normal(size=6)
    Wm = W.edge_information(z, H)
    ident = np.zeros(6)

    def mismatch(t):
        r = G.edge_eval(ident, z + t * d, z, 1.0, False)
        want = t * t * float(d @ H @ d)
        return abs(float(r @ Wm @ r) - want) / want
    m3, m4, m5 = mismatch(1e-3), mismatch(1e-4), mismatch(1e-5)
    print(f"relative mismatch at t = 1e-3, 1e-4, 1e-5: {m3:.2e}, {m4:.2e}, {m5:.2e}")
    assert m3 < 1e-2
    assert 5.0 < m3 / m4 < 20.0 and 5.0 < m4 / m5 < 20.0             # a factor of 10 per decade, to a factor of 2


def test_edge_information_refusals(lib):
    z, H, out = np.zeros(6), np.eye(6).ravel().copy(), np.full(21, 7.0)
    p = lambda a: C.c_void_p(a.ctypes.data)                          # noqa: E731
    assert lib.velo_graph_edge_information(p(z), p(H), p(out)) == 0
    assert np.array_equal(out, W.info21(np.eye(6)))
    for args in ((None, p(H), p(out)), (p(z), None, p(out)), (p(z), p(H), None)):
        assert lib.velo_graph_edge_information(*args) == -1
    for bad in (np.nan, np.inf):
        zz, HH = z.copy(), H.copy()
        zz[2], HH[7] = bad, bad
        out[:] = 7.0
        assert lib.velo_graph_edge_information(p(zz), p(H), p(out)) == -1 and b"z[2]" in lib.velo_last_error()
        assert lib.velo_graph_edge_information(p(z), p(HH), p(out)) == -1 and b"JtJ36[7]" in lib.velo_last_error()
        assert np.all(out == 7.0)
    with pytest.raises(api.VeloError, match="status -1"):
        api.graph_edge_information([0, 0, np.nan, 0, 0, 0], np.eye(6))
    # definiteness is the caller's and velo_graph_add_edges_weighted's business: an indefinite H passes through
    assert lib.velo_graph_edge_information(p(z), p(-H), p(out)) == 0 and out[0] == -1.0


def test_null_arguments_of_the_new_entries(lib):
    one = (C.c_int32 * 1)(0)
    d = (C.c_double * 21)()
    assert lib.velo_graph_add_edges_weighted(None, 0, None, None, None, None, None) == -1 and b"null ctx" in lib.velo_last_error()
    assert lib.velo_graph_add_edges_weighted(None, 1, one, one, d, d, d) == -1 and b"null ctx" in lib.velo_last_error()
    assert lib.velo_graph_edge_stats(None, 0, 0, None, None) == -1 and b"null ctx" in lib.velo_last_error()
    assert lib.velo_graph_edge_stats(None, 0, 1, d, d) == -1 and b"null ctx" in lib.velo_last_error()
