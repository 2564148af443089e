"""tests/ba_ref.py, the numpy restatement of the windowed bundle adjustment, checked on its own (no GPU): its Jacobians against
central differences, its two linear solvers against each other, and its minimum against scipy's.  The spread between the two
solvers measured here is what tests/test_gpu_bundle_adjust.py derives its tolerances from."""
import numpy as np
import pytest

import ba_ref as B
import velo_amd  # noqa: F401


@pytest.fixture(scope="module", params=["A", "B", "C"])
def fixture(request):
    seq = B.fixture_sequence(request.param)
    book = B.book_of(seq)
    F = len(seq["poses"])
    B.triangulate_book(book, seq["poses"], seq["cam_trans"], range(F))
    return request.param, seq, B.Problem(book, seq["poses"], seq["cam_trans"], range(F), 1)


def test_jacobians_against_central_differences(fixture):
    name, seq, prob = fixture
    x = prob.x0()
    _, r, J = prob.evaluate(x, robust=False)
    rng = np.random.default_rng(5)
    cols = np.concatenate([np.arange(6 * prob.n_free), 6 * prob.n_free + rng.choice(3 * prob.L, size=9, replace=False)])
    worst = 0.0
    for j in cols:
        h = 1e-6
        e = np.zeros_like(x)
        e[j] = h
        num = (prob.evaluate(x + e, robust=False)[1] - prob.evaluate(x - e, robust=False)[1]) / (2 * h)
        worst = max(worst, float(np.max(np.abs(num - J[:, j]))))
    # central differences of step h: truncation ~ h^2 |r'''| / 6 and rounding ~ eps |r| / h, both below 1e-7 for residuals of order 1..50
    assert worst < 1e-7, worst
    # the first-order branch at a vanishing rotation joins the Rodrigues branch
    q = np.array([0.3, -1.2, 7.0])
    a = B.rotate_with_derivative(np.array([1e-9, -2e-9, 1e-9]), q)
    b = B.rotate_with_derivative(np.array([1e-7, -2e-7, 1e-7]), q)
    assert np.allclose(a[1], b[1], atol=1e-5) and np.allclose(a[2], b[2], atol=1e-6)


# measured on this restatement (relative in cost along the trace, absolute in the unknowns); the GPU test allows 100 x these
SPREAD = {"A": (5.5e-14, 9.3e-14), "B": (3.0e-14, 2.6e-12), "C": (3.3e-15, 7.2e-14)}
ITERATIONS = {"A": 45, "B": 23, "C": 17}


def test_the_two_solvers_agree(fixture):
    name, seq, prob = fixture
    a, b = B.solve(prob, "lstsq"), B.solve(prob, "schur")
    assert [r["status"] for r in a["trace"]] == [r["status"] for r in b["trace"]]
    assert a["termination"] == b["termination"] == "function" and a["iterations"] == b["iterations"] == ITERATIONS[name]
    assert all(r["status"] == B.ACCEPTED for r in a["trace"][:-1])
    # no decision lies near its threshold: rounding cannot flip one
    margin = min(B.closest_margin(a["trace"]), B.closest_margin(b["trace"]))
    assert margin > 1e-6, margin
    sc, sx = B.spread(a, b)
    print(f"{name}: spread {sc:.2e} relative in cost, {sx:.2e} absolute in the unknowns; closest decision margin {margin:.2e}")
    # the recorded spreads are what was measured, to within a factor of 3 (the SVD is not bit-reproducible across LAPACK builds)
    assert sc <= 3 * SPREAD[name][0] and sx <= 3 * SPREAD[name][1]
    err0 = np.abs(seq["poses"] - seq["truth"]).max()
    err1 = np.abs(prob.poses_of(a["x"]) - seq["truth"]).max()
    if name != "A":
        assert err1 < 0.5 * err0, (err0, err1)


def test_scipy_reaches_the_same_minimum():
    scipy_opt = pytest.importorskip("scipy.optimize")
    seq = B.fixture_sequence("A")
    book = B.book_of(seq)
    B.triangulate_book(book, seq["poses"], seq["cam_trans"], range(4))
    prob = B.Problem(book, seq["poses"], seq["cam_trans"], range(4), 1)
    mine = B.solve(prob, "schur", robust=False, f_tol=1e-14, max_iterations=200)
    ref = scipy_opt.least_squares(lambda x: prob.evaluate(x, robust=False)[1], prob.x0(), jac=lambda x: prob.evaluate(x, robust=False)[2],
                                  method="trf", xtol=1e-15, ftol=1e-15, gtol=1e-12)
    assert abs(mine["final_cost"] - ref.cost) <= 1e-8 * ref.cost, (mine["final_cost"], ref.cost)
    assert np.max(np.abs(mine["x"] - ref.x)) < 1e-5
