"""tests/pose_graph_ref.py, the numpy restatement of the pose-graph optimisation, checked on its own (no GPU): its Jacobians against
central differences, its direct solver against scipy's least squares, its two linear solvers against each other on every fixture of
the GPU test.  The spread between the two solvers measured here is what tests/test_gpu_pose_graph.py derives its tolerances from.
Also the drop-in boundary that needs no device: the structs of include/velo_hip.h against the ctypes mirror, and the refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pose_graph_ref as G
import velo_amd  # noqa: F401
from velo_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_jacobians_against_central_differences():
    rng = np.random.default_rng(11)
    worst = 0.0
    for angle in (0.3, 1.5, 3.1):                                     # the global rotation's angle; the residual's stays small
        for _ in range(4):
            axis = rng.normal(size=3)
            xf = np.concatenate([angle * axis / np.linalg.norm(axis), 3.0 * rng.normal(size=3)])
            xt = G.compose(xf, np.concatenate([0.2 * rng.normal(size=3), rng.normal(size=3)]))
            z = G.relative(xf, xt) + np.concatenate([0.05 * rng.normal(size=3), 0.2 * rng.normal(size=3)])
            _, A, B = G.edge_eval(xf, xt, z, 2.5)
            h = 1e-6
            for j in range(6):
                e = np.zeros(6)
                e[j] = h
                worst = max(worst, np.abs((G.edge_eval(xf + e, xt, z, 2.5, False) - G.edge_eval(xf - e, xt, z, 2.5, False)) / (2 * h) - A[:, j]).max(),
                            np.abs((G.edge_eval(xf, xt + e, z, 2.5, False) - G.edge_eval(xf, xt - e, z, 2.5, False)) / (2 * h) - B[:, j]).max())
    # central differences of step h: truncation ~ h^2 |r'''| / 6 and rounding ~ eps |r| / h, both below 1e-7 for residuals of order 1
    assert worst < 1e-7, worst
    # the series of the inverse right Jacobian joins its closed form, and the first-order rotation joins Rodrigues
    a, b = G.right_jacobian_inverse(np.array([6e-4, -5e-4, 6e-4])), G.right_jacobian_inverse(np.array([6e-4, -5e-4, 6.1e-4]))
    assert np.abs(a - b).max() < 1e-5
    assert np.abs(G.left_jacobian(np.array([1e-9, -2e-9, 1e-9])) - G.left_jacobian(np.array([1e-7, -2e-7, 1e-7]))).max() < 1e-6


def test_the_residual_is_the_relative_rotation_not_a_difference_of_vectors():
    g = G.fixture("large_rotation")
    assert min(np.linalg.norm(p[:3]) for p in g["poses"].values()) > 3.0
    a, b, z, info = g["edges"][0]
    r = G.edge_eval(g["truth"][a], g["truth"][b], z, info, False)
    assert np.linalg.norm(r[:3]) < 0.02                               # the measurement's noise, although both angle-axis vectors are near pi
    # two vectors on either side of pi describe nearly the same rotation: their difference is large, the residual is not
    w = np.array([0.6, 0.0, 0.8])
    xa, xb = np.concatenate([3.13 * w, np.zeros(3)]), np.concatenate([-(2 * np.pi - 3.15) * w, np.zeros(3)])
    assert np.linalg.norm(xa[:3] - xb[:3]) > 6.0
    assert np.linalg.norm(G.edge_eval(xa, xb, np.zeros(6), 1.0, False)[:3]) == pytest.approx(0.02, abs=1e-9)


@pytest.mark.parametrize("name", ["pair", "chain5", "large_rotation"])
def test_scipy_reaches_the_same_minimum(name):
    scipy_opt = pytest.importorskip("scipy.optimize")
    prob = G.problem_of(G.fixture(name))
    mine = G.solve(prob, "direct", f_tol=1e-14, max_iterations=200)
    ref = scipy_opt.least_squares(lambda x: prob.evaluate(x, False)[1], prob.x0(), jac=lambda x: prob.evaluate(x)[2].toarray(),
                                  method="trf", xtol=1e-15, ftol=1e-15, gtol=1e-12)
    assert abs(mine["final_cost"] - ref.cost) <= 1e-8 * max(ref.cost, mine["initial_cost"] * 1e-8), (mine["final_cost"], ref.cost)
    assert np.max(np.abs(mine["x"] - ref.x)) < 1e-5


# Measured on this restatement between `direct` and `pcg` (cost: relative to the initial cost along the trace; unknowns: absolute);
# the GPU test allows 100 x these.  `pair` has one free node, so block-Jacobi CG IS a direct solve and the two agree to the bit: its
# entry is one unit of the format instead: DBL_EPSILON in cost, and DBL_EPSILON x 4 (the power of two above its largest pose
# component, 2.0) in the unknowns.
SPREAD = {"pair": (2.3e-16, 8.9e-16), "chain5": (1.2e-15, 2.5e-14), "ring70": (1.4e-14, 7.7e-13), "hub": (8.5e-15, 2.0e-13),
          "large_rotation": (5.0e-14, 8.5e-14)}
STATUSES = {"pair": [0, 0, 3], "chain5": [0, 0, 4], "ring70": [0, 0, 0, 4], "hub": [0, 0, 4], "large_rotation": [0, 0, 4]}


@pytest.mark.parametrize("name", G.FIXTURES)
def test_the_two_solvers_take_the_same_decisions(name):
    g = G.fixture(name)
    prob = G.problem_of(g)
    a, b = G.solve(prob, "direct"), G.solve(prob, "pcg")
    assert [r["status"] for r in a["trace"]] == [r["status"] for r in b["trace"]] == STATUSES[name]
    assert a["termination"] == b["termination"] and a["iterations"] == b["iterations"] and a["evaluations"] == b["evaluations"]
    # no decision lies near its threshold: rounding cannot flip one
    margin = min(G.closest_margin(a["trace"]), G.closest_margin(b["trace"]))
    assert margin > 1e-6, margin
    sc, sx = G.spread(a, b)
    print(f"{name}: spread {sc:.2e} of the initial cost, {sx:.2e} absolute in the unknowns; closest decision margin {margin:.2e}; "
          f"CG iterations {[r['cg_iterations'] for r in b['trace']]}, cap {G.CG_DEFAULTS['cg_max']}")
    assert max(r["cg_iterations"] for r in b["trace"]) < G.CG_DEFAULTS["cg_max"]
    # the recorded spreads are what was measured, to within a factor of 3 (LAPACK builds differ in their last bits)
    assert sc <= 3 * SPREAD[name][0] and sx <= 3 * SPREAD[name][1]
    x = prob.poses_of(a["x"])
    if name == "pair":                                               # T_0 . Z to the parameter tolerance, cost 0
        assert np.abs(x[1] - g["want"][1]).max() <= 10 * 1e-8 * np.linalg.norm(g["want"][1])
        assert a["final_cost"] <= G.EPS * a["initial_cost"]
    if name == "chain5":                                             # the loop edge's contradiction is spread over the chain
        moved = [np.linalg.norm(x[i][3:] - g["poses"][i][3:]) for i in range(1, 5)]
        assert all(m > 0.01 for m in moved) and moved[3] > moved[0]
    if name == "hub":                                                # the free node without an edge keeps its bytes
        assert x[140].tobytes() == g["poses"][140].tobytes()


PROBE = r'''
#include <stdio.h>
#include <stddef.h>
#include "velo_hip.h"
int main(void) {
  printf("%zu %zu %zu %d\n", sizeof(velo_graph_params), sizeof(velo_graph_iteration), sizeof(velo_graph_summary), VELO_GRAPH_MAX_TRACE);
  printf("%zu %zu %zu\n", offsetof(velo_graph_params, cg_tolerance), offsetof(velo_graph_params, cg_max_iterations), offsetof(velo_graph_params, reserved));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", offsetof(velo_graph_iteration, status), offsetof(velo_graph_iteration, iteration),
         offsetof(velo_graph_iteration, cost), offsetof(velo_graph_iteration, candidate_cost), offsetof(velo_graph_iteration, radius),
         offsetof(velo_graph_iteration, model_change), offsetof(velo_graph_iteration, step_norm), offsetof(velo_graph_iteration, cg_iterations),
         offsetof(velo_graph_iteration, cg_residual));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", offsetof(velo_graph_summary, termination), offsetof(velo_graph_summary, iterations),
         offsetof(velo_graph_summary, evaluations), offsetof(velo_graph_summary, n_nodes), offsetof(velo_graph_summary, n_free),
         offsetof(velo_graph_summary, n_edges), offsetof(velo_graph_summary, n_trace), offsetof(velo_graph_summary, initial_cost),
         offsetof(velo_graph_summary, final_cost), offsetof(velo_graph_summary, trace));
  return 0; }
'''


def test_struct_layouts_match_the_ctypes_mirror(tmp_path):
    cfile, exe = str(tmp_path / "probe.c"), str(tmp_path / "probe")
    open(cfile, "w").write(PROBE)
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), cfile, "-o", exe], check=True)      # the header is plain C
    rows = [[int(v) for v in line.split()] for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()]
    P, I, S = api.VeloGraphParams, api.VeloGraphIteration, api.VeloGraphSummary
    assert rows[0] == [C.sizeof(P), C.sizeof(I), C.sizeof(S), api.GRAPH_MAX_TRACE] == [32, 64, 48 + 50 * 64, 50]
    assert rows[1] == [P.cg_tolerance.offset, P.cg_max_iterations.offset, P.reserved.offset]
    assert rows[2] == [getattr(I, n).offset for n in ("status", "iteration", "cost", "candidate_cost", "radius", "model_change", "step_norm",
                                                      "cg_iterations", "cg_residual")]
    assert rows[3] == [getattr(S, n).offset for n in ("termination", "iterations", "evaluations", "n_nodes", "n_free", "n_edges", "n_trace",
                                                      "initial_cost", "final_cost", "trace")]


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return api.load_library()


def test_default_params_and_null_arguments(lib):
    p = api.VeloGraphParams()
    p.cg_tolerance, p.cg_max_iterations = 7.0, 3
    assert lib.velo_default_graph_params(C.byref(p)) == 0
    assert p.cg_tolerance == G.CG_DEFAULTS["cg_tol"] and p.cg_max_iterations == G.CG_DEFAULTS["cg_max"] and list(p.reserved) == [0] * 5
    assert lib.velo_default_graph_params(None) == -1
    # refused before a context is looked at
    fixed = (C.c_int32 * 1)(0)
    pose = (C.c_double * 6)()
    assert lib.velo_graph_reset(None, 0) == -1
    assert lib.velo_graph_set_pose(None, 0, pose) == -1
    assert lib.velo_graph_set_poses(None, 0, 1, pose) == -1
    assert lib.velo_graph_add_edges(None, 0, None, None, None, None) == -1
    assert lib.velo_graph_optimize(None, fixed, 1, None, None) == -1
    assert lib.velo_graph_get_poses(None, 0, 1, pose) == -1
    assert lib.velo_graph_info(None, None) == -1
    assert lib.velo_graph_system(None, fixed, 1, None, None, None) == -1
    assert b"null ctx" in lib.velo_last_error()
